"""Every window instance of the stream tick and of the level kernel: the case lists of tests/test_gpu_lk_instances.py and the
instance sets tests/test_lk_instances_plan.py expects them to reach.  NumPy only, no GPU; not a test module and not a conftest.

The LK launches are compiled once per window radius (csrc/lk_inst.h: dispatch_radius), and each radius is a kernel of its own: its
tile width (TileGeom<R>), its unrolled window loops, its register allocation and LDS size.  The lists below hold one case per
instance of

    stream_kernel   112 = lk_inst_stream_{c,f,fast}.hip (WOUT 0, plain and deep; compat_cpu at radii 1..12, lk_float at 1..11)
                          + lk_inst_stream_{fw,fastw}.hip (WOUT 3) + lk_inst_stream_{fwr,fastwr}.hip (WOUT 5), plain only
    lk_level_kernel  57 = compat_cpu and lk_float with and without sums, lk_float_fast without
    lk_iter_kernel   88 = ITER 1..4, lk_float and lk_float_fast, plain; and the same 88 in the deep-fetch form (DMA = true), reached in
                          child processes started with OFX_ITER_DMA=1: tests/deep_child.py, whose groups A, E and R run T5 and the
                          cases of iter_hard at every radius (the census: tests/test_deep_plan.py)

The geometry is that of tests/iter_hard.py (_c, _case, hard_pair, tile_out_w, pair_out_w), not restated."""
from collections import namedtuple

import iter_hard as ih

MODE_ID = {"compat_cpu": 0, "lk_float": 1, "lk_float_fast": 2}      # OFX_MODE_* (include/ofx.h)
MAX_RADIUS = {"compat_cpu": 12, "lk_float": 11, "lk_float_fast": 11}   # lk_max_radius (csrc/lk_plan.h)
WOUT_SET, WOUT_WARP, WOUT_ROWS = 0, 3, 5                          # stream_kernel's WOUT: kIterSet, kIterSetWarp, kIterSetWarpRows
TODAY = (3, 9, 15)                                                   # the windows other modules run already: first in every list


def windows(mode):
    """every window of a mode, those that run elsewhere first: a failure at a new instance comes after the known ones passed"""
    rest = [w for w in range(3, 2 * MAX_RADIUS[mode] + 2, 2) if w not in TODAY]
    return list(TODAY) + rest


def seam(win):
    """the tile a streamed case's level 1 is one column wider than: the fused launch's up to 9x9 (iter_hard._c), the tile of the
    level kernel and of the accumulating launches above"""
    r = win >> 1
    return ih.pair_out_w(r) if r <= 4 else ih.tile_out_w(r)


def batch(win, flip=False):
    """B alternates with the radius (the other way round with flip): ticks of one pair (many = 0) and of two (many = 1) in every list"""
    return 1 + (((win >> 1) + int(flip)) & 1)


# ---- T0: the plain tick (WOUT 0), one iteration, 2 B + 1 hard frames --------------------------------------------------------------
Tick = namedtuple("Tick", "id case mode deep")      # deep: Session(deep_fetch=+1 / -1)


def _t0(win, mode, deep):
    c = ih._c(win, seam(win) + 1, 1, batch(win, flip=deep > 0))     # test_gpu_deep_iter._tick_case
    return Tick(f"{c.id}-{mode}-{'deep' if deep > 0 else 'plain'}", c, mode, deep)


T0_CASES = [_t0(win, mode, deep) for mode in ("lk_float", "compat_cpu", "lk_float_fast") for deep in (-1, 1) for win in windows(mode)]

# ---- T3: the tick that also warps (WOUT 3): two iterations are one tick and one ITER 1 launch -------------------------------------
# (B = 2 at the even radii: with B = 2 at the odd ones, pair 4 of window 23 has no tap clamped at sx < 0 on level 0, and the census
# of tests/test_iter_hard_ref.py wants every clamp from every pair)
T3_CASES = [ih._c(win, seam(win) + 1, 2, batch(win, flip=True)) for win in windows("lk_float")]
T3_MODES = ("lk_float", "lk_float_fast")

# ---- T5: row windows (WOUT 5, ITER 4 and ITER 1 behind it): three logical ranks on one device -------------------------------------
Rows = namedtuple("Rows", "id w h levels win iters ranks B warp_margin")
T5_MODES = ("lk_float", "lk_float_fast")


def shard_plans(c):
    from cuda_optical_flow_2_amd.parallel import ShardPlan

    return [ShardPlan(c.w, c.h, c.levels, c.win, r, c.ranks, iters=c.iters, warp_margin=c.warp_margin) for r in range(c.ranks)]


def cuts_deep_enough(c):
    """ShardPlan accepts every rank, and wherever a rank's buffer ends inside a level at least R + 2 rows of that level lie beyond
    it (a row window that cuts one row proves little)"""
    try:
        plans = shard_plans(c)
    except ValueError:
        return False
    need = (c.win >> 1) + 2
    for pl in plans:
        for k in range(c.levels):
            above, below = pl.buf[k][0], (c.h >> k) - pl.buf[k][1]
            if (0 < above < need) or (0 < below < need):
                return False
    # every rank but the first is cut above, every rank but the last below, at every level
    return all(pl.buf[k][0] > 0 or pl.rank == 0 for pl in plans for k in range(c.levels)) and \
        all(pl.buf[k][1] < (c.h >> k) or pl.rank == c.ranks - 1 for pl in plans for k in range(c.levels))


def _t5(win):
    """two tile columns and one more pixel per level-1 tile; the smallest height, a multiple of 4, whose cuts are deep enough"""
    w = 2 * (ih.tile_out_w(win >> 1) + 1)
    h = 4
    while not cuts_deep_enough(Rows("", w, h, 2, win, 3, 3, 1, 8)):
        h += 4
    # two pairs per tick at the even radii up to 17x17: above, the oracle's three iterations take seconds per pair
    B = batch(win, flip=True) if win <= 17 else 1
    return Rows(f"R-win{win}-{w}x{h}-B{B}", w, h, 2, win, 3, 3, B, 8)


T5_CASES = [_t5(win) for win in windows("lk_float")]


def rows_frames(c):
    """smooth frames, as deep_child.rows_frames: the huge flows of the hard frames leave a shard's rows and rightly set its status.
    So do the outliers of a 3x3 or 5x5 window on that texture -- bilinear in cells of 8 pixels, a plane to a window inside a cell;
    the oracle puts 1 637 / 96 tap rows of these cases beyond a rank's buffer (warp_margin = 8), and none with cells of 3 pixels:
    tests/test_iter_hard_ref.py asserts on the oracle that no case leaves its rows"""
    from cuda_optical_flow_2_amd import synth

    return [synth.smooth_pair(c.w, c.h, 1.1 * i, 0.6 * i, seed=29, cell=3 if c.win <= 5 else 8)[1] for i in range(2 * c.B + 1)]


# ---- L: the level kernel, one level: two tiles, the second one column wide, an odd width, the flat block across the seam ----------
Level = namedtuple("Level", "id w h win mode sums")


def _l(win, mode, sums):
    ow = ih.tile_out_w(win >> 1)
    return Level(f"L-win{win}-{mode}{'-sums' if sums else ''}", ow + 1, 67, win, mode, sums)


L_CASES = [_l(win, mode, sums) for mode in ("compat_cpu", "lk_float") for sums in (True, False) for win in windows(mode)] + \
          [_l(win, "lk_float_fast", False) for win in windows("lk_float_fast")]


def level_pair(c):
    return ih.hard_pair(c.w, c.h, seam_x=c.w - 1)


# ---- the instance sets, as the lk_inst_*.hip units and lk_inst.h define them ------------------------------------------------------
def radii(mode):
    return range(1, MAX_RADIUS[mode] + 1)


def stream_family():
    """{(MODE, FAST, WOUT, deep, radius)}: the deep fetch for WOUT 0 only (ofx_launch::stream), warped images in lk_float only"""
    out = set()
    for mode, (kernel_mode, fast) in (("compat_cpu", (0, 0)), ("lk_float", (1, 0)), ("lk_float_fast", (1, 1))):
        wouts = (WOUT_SET,) if mode == "compat_cpu" else (WOUT_SET, WOUT_WARP, WOUT_ROWS)
        out |= {(kernel_mode, fast, wout, deep, r) for wout in wouts for deep in ((0, 1) if wout == WOUT_SET else (0,)) for r in radii(mode)}
    return out


def levels_family():
    """{(MODE, FAST, sums, radius)}: lk_inst_levels_{c,f,fast}.hip (the inspection variant does not depend on the solve: no fast one)"""
    return {(0, 0, s, r) for s in (0, 1) for r in radii("compat_cpu")} | {(1, 0, s, r) for s in (0, 1) for r in radii("lk_float")} | \
           {(1, 1, 0, r) for r in radii("lk_float_fast")}


def iter_family(deep=0):
    """{(MODE, FAST, ITER, deep, radius)}: lk_inst_iter_{f,fast}{1,2,3,4}.hip, the plain form (deep = 0) or the deep-fetch one (1)"""
    return {(1, fast, it, deep, r) for fast in (0, 1) for it in (1, 2, 3, 4) for r in radii("lk_float")}


assert (len(stream_family()), len(levels_family()), len(iter_family()), len(iter_family(deep=1))) == (112, 57, 88, 88)
