"""The cases and frames of test_gpu_warp_taps.py (GPU) and test_warp_taps_frames.py (what the frames are meant to provoke, checked on
the CPU with the oracle and the planner).  Not a test module.

Sizes are those of LEVEL 1 of a two-level pyramid -- the stream pipeline downsamples even sizes only, so a level of 231 x 11 is level 1
of a 462 x 22 frame; level 0 runs through the same launches, with twice the tile columns, and is compared too.
  widths   one column short of the fused tile, the tile, one more (a second tile of one column), and two tiles and a few columns:
           9x9 (232 columns) 231 / 232 / 233 / 470, 7x7 and 5x5 (240) 239 / 240 / 241 / 482, 3x3 (248) 247 / 248 / 249 / 498
  heights  2, 11, 12, 17, 33, 70: at 9x9 the second march starts 2R + 3 = 11 joint steps after the first and emits its first row at
           step 3R + 4 = 16; a level of 2 rows is over before the priming is, in one of 11 or 12 the first march has finished when the
           second starts to emit (steps in which A emits nothing while B runs), 17 is one row more than priming and lag
  iters    3: the tick and one fused launch without warped output; 4: the tick, a fused launch with it and a single launch; 5: both
           fused forms
Every (window, iterations, width) occurs once; the heights go round twice per window.
waves: OFX_PAIR_WAVES of the run with the fused launches, chosen (tools/pair_plan_main.cpp, minimum piece 1) so that waves carry two
segments and the cuts between them fall inside tile columns, some of them one or two rows from a level's top or bottom
(test_warp_taps_frames.py checks that with the planner)."""
import numpy as np

from cuda_optical_flow_2_amd import synth

HEIGHTS = [2, 11, 12, 17, 33, 70]
WIDTHS = {9: [231, 232, 233, 470], 7: [239, 240, 241, 482], 5: [239, 240, 241, 482], 3: [247, 248, 249, 498]}
TILE = {9: 232, 7: 240, 5: 240, 3: 248}
LEVELS = 2
NFRAMES = 6   # smooth, smooth, flat blocks, flat blocks, noise, noise: pairs 1 smooth, 3 flat, 5 noise, 2 and 4 mixed


def cases():
    """(window, iters, level-1 width, level-1 height, frames per tick, OFX_PAIR_WAVES)"""
    out = []
    for wi, win in enumerate((9, 7, 5, 3)):
        n = 0
        for iters in (3, 4, 5):
            for lw in WIDTHS[win]:
                lh = HEIGHTS[(n + wi) % len(HEIGHTS)]
                B = 1 + (n % 2)
                columns = sum(-(-w // TILE[win]) for w, _ in items(lw, lh, B))
                out.append((win, iters, lw, lh, B, WAVES.get((win, lw, lh), {3: 2, 5: 3, 6: 4, 16: 12}[columns])))
                n += 1
    return out


def items(lw, lh, B):
    """the (w, h) of a tick's items: per pair the coarsest level first (session_stream.cpp)"""
    return [(lw << k, lh << k) for _ in range(B) for k in range(LEVELS)]


# OFX_PAIR_WAVES: by the number of tile columns of a tick (3, 5, 6 or 16) two thirds to three quarters of them, so that most waves carry
# two segments and some columns are cut; per (window, level-1 width, level-1 height) another count where that one puts a cut one or
# two rows from a column's top or bottom
WAVES = {(9, 231, 33): 3, (5, 239, 12): 3, (3, 247, 17): 3, (9, 233, 33): 5, (5, 241, 12): 5, (3, 249, 17): 5, (3, 249, 11): 5,
         (9, 232, 17): 6, (5, 240, 11): 6, (7, 240, 2): 5, (3, 248, 2): 5, (7, 482, 33): 16, (7, 482, 2): 11, (3, 498, 2): 11,
         (3, 498, 12): 16}


def frame(kind, w, h, i, seed):
    """frame i (0 or 1) of a pair of one kind, h x w uint8"""
    if kind == "smooth":
        return synth.smooth_pair(w, h, 1.5 * i, -0.9 * i, seed=seed)[1]
    if kind == "noise":   # uniform noise: flows of many pixels, taps clamped at every border
        return synth.random_pair(w, h, seed=seed + 11 * i)[i]
    # flat blocks on the smooth texture: a band over the whole height (also where a level has 2 rows: the window is clipped to the
    # image, so a flat band wider than the window and its derivatives is singular there) and, where there is room, a block
    f = synth.smooth_pair(w, h, 1.5 * i, -0.9 * i, seed=seed + 1)[1].copy()
    f[:, w // 4: w // 4 + 56] = 77
    f[h // 3: h // 3 + max(h // 3, 1), (3 * w) // 5: (3 * w) // 5 + 64] = 140
    return f


# Seeds: lw + lh + 1000 * n with the first n for which the oracle finds what the frames are there for (test_warp_taps_frames.py):
# non-finite flows in the flat pair before every warp on both levels, and in the noise pair taps clamped at all four borders of
# level 1 before every warp.  n = 0 except (a level of 2 rows has two pixels on its left and right border):
SEED_N = {(9, 231, 2): 7, (9, 232, 11): 2, (9, 233, 12): 1, (9, 470, 17): 1, (9, 233, 2): 11, (9, 231, 12): 2, (9, 232, 17): 1,
          (7, 240, 12): 1, (7, 240, 2): 8, (7, 241, 11): 1, (7, 482, 2): 6, (5, 239, 12): 2, (5, 239, 2): 5, (5, 241, 2): 13,
          (3, 498, 2): 1, (3, 247, 11): 2, (3, 248, 2): 10, (3, 249, 11): 1}


def seed(win, lw, lh):
    return lw + lh + 1000 * SEED_N.get((win, lw, lh), 0)


def frames(lw, lh, seed):
    w, h = lw << (LEVELS - 1), lh << (LEVELS - 1)
    return [np.ascontiguousarray(frame(kind, w, h, i, seed)) for kind in ("smooth", "flat", "noise") for i in (0, 1)]
