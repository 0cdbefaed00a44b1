#!/bin/bash
# One GPU-box visit: parity tests, smoke, bench (--full), tuning sweep, rocprofv3 kernel trace.  Everything is wrapped
# in `timeout`; every log lands under the directory given as the first argument.  Run from the repository root.
export TMPDIR=/tmp
mkdir -p "${1:?usage: bash scripts/gpu_round.sh LOG_DIR}"
O=$(cd "$1" && pwd)
R=$(pwd)
rocminfo 2>/dev/null | grep -m2 -E "gfx|Marketing" > $O/device.txt
echo "== smoke" ; timeout 600 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1; echo "smoke rc=$?"; tail -3 $O/smoke.log
echo "== pytest -m gpu"; timeout 1200 python -m pytest tests -m gpu -q -x --timeout 900 > $O/pytest_gpu.log 2>&1; echo "pytest rc=$?"; tail -15 $O/pytest_gpu.log
echo "== bench"; timeout 900 python bench.py --full --steps ${BENCH_STEPS:-5} --warmup 2 > $O/bench.log 2>$O/bench.err; echo "bench rc=$?"; tail -2 $O/bench.log; tail -3 $O/bench.err
if [ "${DO_SWEEP:-1}" = "1" ]; then echo "== sweep"; timeout 900 python scripts/sweep.py ${SWEEP_N:-128} > $O/sweep.log 2>&1; echo "sweep rc=$?"; tail -40 $O/sweep.log; fi
if [ "${DO_PROF:-1}" = "1" ]; then
  echo "== rocprofv3"
  ( cd /tmp && timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof -o bench -- python $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > $O/prof_bench.log 2>&1 ); echo "rocprof rc=$?"
  find $O/prof -name "*stats*" | head; f=$(find $O/prof -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && head -12 "$f"; true
fi
