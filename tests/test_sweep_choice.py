"""CPU tier of the sweep choice (dvo_slam_amd/csrc/sweep_choice.h): which of the five sweep kernels runs a level and what follows from it,
compiled for the host (g++ -Wall -Werror) and walked over a grid of options and sizes.

(a) The choice equals the rules it replaced, restated here in Python from the code at commit 82c9bd6 -- the driver's predicates and the
    launcher's ladder SEPARATELY, as they stood there, each quoted with file and line.  They disagreed in one corner (a level of 2^28
    pixels and more whose width the contracted window sweep takes but whose buffers exceed 32-bit offsets): there the choice follows the
    launcher's kernel and tiling, and the planes follow the kernel.  The corner is computed, not listed.
(b) Invariants between the fields of a choice, and between every choice and the allocation predicate."""
import ctypes as C
import functools
import itertools
import os
import subprocess
import tempfile
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dvo_slam_amd", "csrc")

HOST_SOURCE = r"""
#include "sweep_choice.h"
using namespace dvo_hip;
// out: kernel (0 valu, 1 gather, 2 window, 3 fast, 4 small), linear, reads_c, tile_rows, compact, mode, pair_list, operand_store
extern "C" void sweep_choice_of(int variant, int small_sweep, int ref_compat, int ref_order, int compact_residuals, int w, int h, int* out) {
  const SweepChoice c = choose_sweep(SweepOptions{variant, small_sweep, ref_compat, ref_order, compact_residuals}, w, h);
  out[0] = int(c.kernel); out[1] = c.linear; out[2] = c.reads_c; out[3] = c.tile_rows; out[4] = c.compact; out[5] = c.mode; out[6] = c.pair_list;
  out[7] = c.operand_store;
}
extern "C" int sweep_tail_of(int variant, int small_sweep, int ref_compat, int ref_order, int compact_residuals, int w, int h, int rows_per_wave,
                             int rcp_table, int gram_hi_j) {
  const SweepChoice c = choose_sweep(SweepOptions{variant, small_sweep, ref_compat, ref_order, compact_residuals}, w, h);
  return sweep_has_tail(c, rows_per_wave, rcp_table != 0, gram_hi_j != 0);
}
extern "C" int plane_c_possible(int w, int h) { return any_sweep_reads_plane_c(w, h); }
"""

VALU, GATHER, WINDOW, FAST, SMALL = range(5)
Choice = namedtuple("Choice", "kernel linear reads_c tile_rows compact mode pair_list operand_store")
Options = namedtuple("Options", "variant small_sweep ref_compat ref_order compact_residuals")


@functools.lru_cache(maxsize=None)
def host_lib():
    tmp = tempfile.mkdtemp(prefix="sweep_choice_")
    src, out = os.path.join(tmp, "sweep_choice_host.cpp"), os.path.join(tmp, "sweep_choice_host.so")
    with open(src, "w") as f:
        f.write(HOST_SOURCE)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + CSRC, src, "-o", out])
    return C.CDLL(out)


def choice_of(o, w, h):
    out = (C.c_int * 8)()
    host_lib().sweep_choice_of(*o, w, h, out)
    return Choice(out[0], bool(out[1]), bool(out[2]), out[3], bool(out[4]), out[5], bool(out[6]), out[7])


def tail_of(o, w, h, rpw, rcp_table, hi_j):
    return bool(host_lib().sweep_tail_of(*o, w, h, rpw, int(rcp_table), int(hi_j)))


SIZES = [(640, 480), (320, 240), (160, 120), (80, 60), (40, 30), (20, 15),
         (192, 80), (96, 40), (48, 20),
         (170, 66), (85, 33),
         (84, 8), (82, 8), (83, 9), (64, 16), (128, 4), (2, 2),
         (16384, 16384), (16386, 16384), (32768, 4), (32766, 32768)]


def option_grid():
    for variant, small, compat, order, compact in itertools.product((0, 5, 6, 7, 8, 9), (0, 1), (0, 1, 2), (0, 1), (0, 1)):
        if order and variant not in (7, 8):                  # (capi_options.inc:97: "ref_order runs under variant 7 or 8")
            continue
        yield Options(variant, small, compat, order, compact)


# ---- the rules at commit 82c9bd6 ----------------------------------------------------------------------------------------------------------
K_TILE_W, K_WAVES = 64, 4                 # device_types.h:20-21
K_FAST_COLS = 84                          # fast_sweep.h:14
K_SMALL_CELLS = 5376                      # align_small.hip:23
K_COMPACT_TILE_ENTRIES = 1024             # device_types.h:109


def fast_sweep_takes_width(w):            # align_fast.hip:107
    return w >= K_FAST_COLS and w % 2 == 0


def small_sweep_takes(w, h):              # align_small.hip:156-158
    return w % 2 == 0 and w >= 4 and h >= 4 and (w + 2) * (h + 2) <= K_SMALL_CELLS


# the driver's predicates, on (options, w, h)
def level_uses_fast_window(o, w, h):      # capi_frames.inc:171-173
    return o.variant >= 8 and fast_sweep_takes_width(w) and w < 32768 and h < 32768


def level_is_linear(o, w):                # capi_frames.inc:178 (the made-up height 4 is the code's)
    return o.variant >= 5 and w % K_TILE_W != 0 and not level_uses_fast_window(o, w, 4)


def level_uses_window(o, w, h):           # capi_frames.inc:181-183
    return (o.variant >= 6 and w % K_TILE_W == 0 and w < 32768 and h < 32768) or level_uses_fast_window(o, w, h)


def level_uses_small(o, w, h):            # capi_frames.inc:185-187
    return bool(o.small_sweep and o.variant >= 8 and not o.ref_compat and not o.ref_order and not level_uses_window(o, w, h)
                and level_is_linear(o, w) and small_sweep_takes(w, h))


def level_tiles(w, h, rpw, linear):       # capi_frames.inc:158-168
    th = K_WAVES * rpw
    if linear:
        segments = (w * h + K_TILE_W - 1) // K_TILE_W
        return 1, (segments + th - 1) // th
    return (w + K_TILE_W - 1) // K_TILE_W, (h + th - 1) // th


def level_may_read_plane_c(w, h):         # capi_frames.inc:242-244
    return w % K_TILE_W == 0 or fast_sweep_takes_width(w) or small_sweep_takes(w, h)


Geom = namedtuple("Geom", "w h linear small tiles_x tiles_y rcp_table gram_hi_j")


def fast_sweep_supports(g):               # align_fast.hip:109-113
    plane_bytes, packed_bytes = 8 * g.w * g.h, 8 * K_COMPACT_TILE_ENTRIES * g.tiles_x * g.tiles_y
    return (not g.linear and fast_sweep_takes_width(g.w) and g.w < 32768 and g.h < 32768 and plane_bytes < (1 << 31)
            and packed_bytes < (1 << 31))


def window_sweep_supports(g):             # align_window.hip:361
    return not g.linear and g.w % K_TILE_W == 0 and g.w < 32768 and g.h < 32768


def driver_tile_rows(o, w, h):            # capi_frames.inc:215: 4 where a window sweep is expected; elsewhere by the batch (0 here)
    return 4 if level_uses_window(o, w, h) else 0


def driver_geom(o, w, h, rpw, hi_j):      # make_geom, capi_frames.inc:199-208 (gram_hi_j, :205, also depends on options outside the choice)
    linear = level_is_linear(o, w)
    tx, ty = level_tiles(w, h, rpw, linear)
    return Geom(w, h, linear, level_uses_small(o, w, h), tx, ty, o.ref_compat != 0, hi_j)


def driver_compact(o, rpw, g):            # capi_frames.inc:208
    return bool(o.compact_residuals and not o.ref_order and o.variant >= 8 and rpw == 4 and fast_sweep_supports(g))


def driver_reads_c(o, w, h):              # capi_schedule.inc:111
    return level_uses_window(o, w, h) or level_uses_small(o, w, h)


# the launcher's ladder, on (variant, rows_per_wave, g)
def launcher_kernel(variant, rpw, g):     # align_kernels.hip:183-209
    if g.small:
        return SMALL
    if variant >= 8 and rpw == 4 and fast_sweep_supports(g):
        return FAST
    if variant >= 6 and rpw == 4 and window_sweep_supports(g):
        return WINDOW
    return GATHER if variant >= 5 else VALU


def launcher_mode(variant, g):            # align_kernels.hip:199 and align_mfma.hip:124
    mode = 2 if variant >= 8 else 1 if variant >= 7 else 0
    return 1 if mode == 2 and g.rcp_table else mode


def launcher_window_f16(variant):         # align_kernels.hip:195
    return variant >= 7


def launcher_fast_store(variant, g):      # align_fast.hip:148-163
    return 2 if g.rcp_table or variant == 8 else 1


def sweep_fast_has_tail(variant, g):      # align_fast.hip:105
    return variant == 8 and not g.rcp_table and not g.gram_hi_j and fast_sweep_supports(g)


def mfma_sweep_has_tail(variant, rpw, g):  # align_mfma.hip:119
    return variant >= 8 and not g.rcp_table and rpw != 16


def launcher_has_tail(variant, rpw, g):   # align_kernels.hip:168-173
    if g.small:
        return False
    if variant >= 8 and rpw == 4 and fast_sweep_supports(g):
        return sweep_fast_has_tail(variant, g)
    if variant >= 6 and rpw == 4 and window_sweep_supports(g):
        return False
    return variant >= 5 and mfma_sweep_has_tail(variant, rpw, g)


def launcher_takes_pair_list(variant, rpw, g):   # align_kernels.hip:177-181
    if variant < 8 or g.small:
        return False
    if rpw == 4 and fast_sweep_supports(g):
        return True
    return not (rpw == 4 and window_sweep_supports(g))


def rows_the_driver_may_pick(o, w, h):
    """The tile heights a plan can hold for the level at that commit: 4 where the driver expected a window sweep, else any of the kernels' five."""
    return (4,) if driver_tile_rows(o, w, h) else (1, 2, 4, 8, 16)


def in_corner(o, w, h):
    """The driver built plane C alone and fixed the tile height, the launcher ran the gathering sweep (which reads A + B)."""
    g = driver_geom(o, w, h, 4, False)
    return level_uses_window(o, w, h) and launcher_kernel(o.variant, 4, g) == GATHER


def test_the_choice_is_the_launchers_ladder_and_the_drivers_predicates():
    corner = []
    cases = 0
    for o in option_grid():
        for w, h in SIZES:
            c = choice_of(o, w, h)
            if in_corner(o, w, h):
                corner.append((o, w, h))
            for rpw in rows_the_driver_may_pick(o, w, h):
                for hi_j in (False, True):
                    g = driver_geom(o, w, h, rpw, hi_j)
                    what = (o, w, h, rpw, hi_j)
                    # the launcher's restatement
                    kernel = launcher_kernel(o.variant, rpw, g)
                    assert c.kernel == kernel, what
                    assert c.linear == g.linear, what        # (what the launcher is handed: make_geom's, capi_frames.inc:199)
                    if kernel == GATHER:
                        assert c.mode == launcher_mode(o.variant, g), what
                    if kernel == WINDOW:
                        assert (c.mode >= 1) == launcher_window_f16(o.variant), what
                    if kernel == FAST:
                        assert c.operand_store == launcher_fast_store(o.variant, g), what
                    assert c.pair_list == launcher_takes_pair_list(o.variant, rpw, g), what
                    assert tail_of(o, w, h, rpw, g.rcp_table, hi_j) == launcher_has_tail(o.variant, rpw, g), what
                    # the driver's restatement
                    if in_corner(o, w, h):
                        continue
                    assert c.reads_c == driver_reads_c(o, w, h), what
                    assert (c.kernel == SMALL) == g.small, what
                    assert c.compact == driver_compact(o, rpw, g), what
                    assert c.tile_rows == driver_tile_rows(o, w, h), what
                    cases += 1
    assert cases > 10000
    # the corner: only levels of 2^28 pixels and more; there the planes follow the launcher's kernel and the driver picks the tile height
    assert corner and {(w, h) for _, w, h in corner} == {(16386, 16384)}
    for o, w, h in corner:
        assert w * h >= 1 << 28 and o.variant >= 8
        c = choice_of(o, w, h)
        assert c.kernel == GATHER and not c.linear and not c.reads_c and c.tile_rows == 0 and not c.compact


def test_invariants_of_a_choice():
    for o in option_grid():
        for w, h in SIZES:
            c = choice_of(o, w, h)
            what = (o, w, h, c)
            assert c.reads_c == (c.kernel in (WINDOW, FAST, SMALL)), what
            if c.reads_c:
                assert host_lib().plane_c_possible(w, h), what
            if c.kernel in (WINDOW, FAST):
                assert not c.linear and c.tile_rows == 4, what
            else:
                assert c.tile_rows == 0, what
            if c.compact:
                assert c.kernel == FAST, what
            if c.kernel == SMALL:
                assert c.linear, what
            if c.pair_list:
                assert o.variant >= 8 and c.kernel != SMALL, what


def test_the_allocation_predicate_is_the_one_it_replaced():
    for w, h in SIZES:
        assert bool(host_lib().plane_c_possible(w, h)) == level_may_read_plane_c(w, h), (w, h)
