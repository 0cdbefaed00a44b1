#!/usr/bin/env python
"""Every `file:line` citation of a reference file in the headers, kernels, oracle, tests and documents resolves to a file of the
reference tree and stays within its length.  The reference's file list and line counts are stored in tests/golden/reference_lines.json,
so the check runs without the reference tree (tests/test_docs.py runs it); `--write-fixture REFERENCE_DIR` regenerates that file."""
import os, re, glob, collections, json, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'reference_lines.json')
if len(sys.argv) == 3 and sys.argv[1] == '--write-fixture':
    lines = {}
    for d,_,fs in os.walk(sys.argv[2]):
        for f in fs:
            if f.endswith(('.cpp','.h','.hpp','.cfg','.yaml','.txt','.xml')) or f=='Makefile':
                p = os.path.join(d,f)
                lines[os.path.relpath(p, sys.argv[2])] = sum(1 for _ in open(p, errors='ignore'))
    json.dump(lines, open(FIXTURE, 'w'), indent=0, sort_keys=True); open(FIXTURE, 'a').write('\n')
    sys.exit(0)
ref_lines = json.load(open(FIXTURE))
ref_files = collections.defaultdict(list)
for p in ref_lines:
    ref_files[os.path.basename(p)].append(p)
srcs = glob.glob(ROOT+'/include/**/*.h', recursive=True)+glob.glob(ROOT+'/dvo_slam_amd/csrc/*')+glob.glob(ROOT+'/oracle/*.cpp')+glob.glob(ROOT+'/oracle/*.h')+glob.glob(ROOT+'/oracle/*.py')+glob.glob(ROOT+'/dvo_slam_amd/*.py')+[ROOT+'/DESIGN.md',ROOT+'/HISTORY.md',ROOT+'/INTEGRATION.md',ROOT+'/README.md']+glob.glob(ROOT+'/tests/*.py')
pat = re.compile(r'([A-Za-z0-9_./]+\.(?:cpp|h|hpp|cfg|yaml)):(\d+)(?:-(\d+))?')
bad=[]; n=0
for s in srcs:
    if not os.path.isfile(s): continue
    for ln, line in enumerate(open(s, errors='ignore'), 1):
        for m in pat.finditer(line):
            path, a, b = m.group(1), int(m.group(2)), int(m.group(3) or m.group(2))
            base = os.path.basename(path)
            cands = [p for p in ref_files.get(base, []) if p.endswith(path.lstrip('./'))] or (ref_files.get(base, []) if '/' not in path else [])
            if not cands:
                continue        # one of ours, or an abbreviation
            n+=1
            length = max(ref_lines[p] for p in cands)
            if max(a,b) > length or b < a:
                bad.append("%s:%d cites %s:%s (file has %d lines)" % (os.path.relpath(s,ROOT), ln, path, m.group(0).split(':',1)[1], length))
print(n, "citations checked;", len(bad), "out of range"); print("\n".join(bad[:40]))
