"""Hard frames for the refinement iterations, the case lists of tests/test_gpu_iter_hard.py, and what the oracle alone has to show
on them (tests/test_iter_hard_ref.py): NumPy only, no GPU.

The frames are those of test_fused_warp_of_the_next_iteration_equals_the_warp_launch (tests/test_gpu_parity.py) -- smooth texture
above, uniform noise below, a flat block of value 77 in every frame -- with three additions: bands of nearly singular stripes
(angle 0.3) along the right and the left edge, a band of axis-parallel stripes (exactly singular) in the bottom left corner, and the
flat block placed across a tile seam of the level under test.  Flat windows and axis-parallel stripes leave NaN in the reference's
unguarded solve ("no warp" in the next iteration; a zero determinant ends in 0 * Inf or Inf - Inf on these frames, never in
Inf); noise and the nearly singular bands leave huge finite flows (taps clamped to all four borders)."""
from collections import namedtuple

import numpy as np

from cuda_optical_flow_2_amd import synth

MIN_DET = 5e9   # the threshold of the existing guard tests (test_determinant_guard, test_iteration_pairs_with_the_determinant_guard)


# ---- tile widths -----------------------------------------------------------------------------------------------------------
def tile_out_w(r):
    """TileGeom<R>::OUT_W of cuda_optical_flow_2_amd/csrc/lk_body.h: the output columns of a wave tile of the level kernel and
    of the accumulating launches, restated from the formula there.  A change of the tile moves the seam away from the flat block
    and the census of test_iter_hard_ref.py fails."""
    lo, hi = (r + 1 + 3) // 4, (251 - r) // 4
    return (hi - lo + 1) * 4


def pair_out_w(r):
    """TileGeomP<R>::OUT_W of cuda_optical_flow_2_amd/csrc/lk_body_pair.h (two iterations per launch, radii 1..4)"""
    lo = (2 * r + 2 + 3) // 4
    return (63 - lo - lo + 1) * 4


assert [tile_out_w(r) for r in range(1, 12)] == [248] * 3 + [240] * 4 + [232] * 4      # the static asserts of the two headers
assert [pair_out_w(r) for r in range(1, 5)] == [248, 240, 240, 232]


# ---- frames ----------------------------------------------------------------------------------------------------------------
def stripes(w, h, ang, shift):
    """_stripes of tests/test_gpu_parity.py"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    t = np.cos(ang) * xx + np.sin(ang) * yy
    return np.clip(127 + 100 * np.sin((t - shift) * 0.3), 0, 255).astype(np.uint8)


def hard_frames(w, h, nf, seed=None, seam_x=None, level=0, block=(40, 90), band=24, corner=0):
    """nf frames (h, w) u8.  seam_x: the column, at pyramid level `level`, the flat block straddles (default: the block of the
    existing tests, from w // 4 on); with level > 0 a second block straddles column seam_x of level 0 itself.  block: rows and
    columns of the flat block at level 0 (it has to hold a whole window, and the 3x3 derivative taps around it, at every level
    that is to see 0 / 0); band: width of the two stripe bands; corner: side of a black square in the top left corner (pixel 0 of
    every level it reaches has no texture at all: 0 / 0 unguarded, and that NaN is the level's shift vector)."""
    seed = w if seed is None else seed
    bh, bw = block
    y0 = h // 3
    out = []
    for i in range(nf):
        f = synth.random_pair(w, h, seed=seed + 7 * i)[i & 1]
        sm = synth.smooth_pair(w, h, 1.5 * i, -0.9 * i, seed=seed)[1]
        f[: h // 2] = sm[: h // 2]
        f[: h // 4, w - band:] = stripes(w, h, 0.3, 0.7 * i)[: h // 4, w - band:]               # nearly singular, right edge
        f[h // 4: h // 2, :band] = stripes(w, h, -0.3, -0.7 * i)[h // 4: h // 2, :band]         # ... and left edge (the coarser levels
        #                                                                                       have no noise strong enough there)
        f[h - h // 4:, :band] = stripes(w, h, 0.0, 0.7 * i)[h - h // 4:, :band]                 # exactly singular, bottom left
        if seam_x is None:
            f[y0: y0 + bh, w // 4: w // 4 + bw] = 77
        else:
            c = seam_x << level
            f[y0: y0 + bh, max(c - bw // 2, 0): c + bw // 2] = 77
            if level:
                f[y0: y0 + bh, max(seam_x - 45, 0): seam_x + 45] = 77
        f[:corner, :corner] = 0
        out.append(f)
    return out


def hard_pair(w, h, seed=None, seam_x=None, **kw):
    p, n = hard_frames(w, h, 2, seed, seam_x, **kw)
    return p, n


# ---- census ----------------------------------------------------------------------------------------------------------------
CENSUS_KEYS = ("no_warp", "sx_lo", "sx_hi", "sy_lo", "sy_hi", "last_col", "last_row")


def warp_census(flow, w, h, scale):
    """What orc_warp_bilinear_u8 (oracle/ofx_oracle.c) does with `flow`, in its own float arithmetic: the number of pixels that
    take the "no warp" branch, that have sx < 0, sx > w - 1, sy < 0, sy > h - 1 (clamped), and that have a tap in the last column
    / the last row."""
    flow = np.asarray(flow, np.float32)
    s = np.float32(scale)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        sx = xx + s * flow[..., 0]
        sy = yy + s * flow[..., 1]
        big = np.float32(1e9)
        warped = (sx >= -big) & (sx <= big) & (sy >= -big) & (sy <= big)
        cx = np.clip(np.where(warped, sx, 0), 0, np.float32(w - 1))
        cy = np.clip(np.where(warped, sy, 0), 0, np.float32(h - 1))
    x1 = np.minimum(cx.astype(np.int64) + 1, w - 1)
    y1 = np.minimum(cy.astype(np.int64) + 1, h - 1)
    return {"no_warp": int((~warped).sum()),
            "sx_lo": int((warped & (sx < 0)).sum()), "sx_hi": int((warped & (sx > np.float32(w - 1))).sum()),
            "sy_lo": int((warped & (sy < 0)).sum()), "sy_hi": int((warped & (sy > np.float32(h - 1))).sum()),
            "last_col": int((warped & (x1 == w - 1)).sum()), "last_row": int((warped & (y1 == h - 1)).sum())}


def oracle_chain(orc, prev, nxt, levels, win, iters, min_det=0.0):
    """The oracle's iteration chain, level by level: [{"prev", "next" (globally shifted), "flows": [F_1 .. F_iters]}].  F_j is the
    flow after j iterations (orc_lk_iter_level with iters = j: a prefix of the longer chain); F_iters is flow_pair_iter's result."""
    pp = orc.gauss_pyramid(synth.to_3ch(prev), levels)
    npyr = orc.gauss_pyramid(synth.to_3ch(nxt), levels)
    h, w = prev.shape
    first = [np.zeros((h >> k, w >> k, 2), np.float32) for k in range(levels)]
    out = [None] * levels
    for k in range(levels - 1, -1, -1):
        n3 = npyr[k] if k == levels - 1 else orc.shift_back_pyramid(npyr[k], k, levels, first)
        p1, n1 = np.ascontiguousarray(pp[k][:, :, 0]), np.ascontiguousarray(n3[:, :, 0])
        flows = [orc.lk_iter_level(p1, n1, win, j, min_det)[0] for j in range(1, iters + 1)]
        first[k] = flows[0]
        out[k] = {"prev": p1, "next": n1, "flows": flows}
    return out


def level_census(orc, lv, win, seam_x):
    """Summed over the flows that enter a warp at this level (after 1 .. iters - 1 iterations): warp_census, and "seam": the
    non-finite pixels within R + 1 columns of seam_x (None where the level has no such column)."""
    h, w = lv["prev"].shape
    r = win >> 1
    tot = dict.fromkeys(CENSUS_KEYS, 0)
    tot["seam"] = 0 if seam_x is not None and seam_x < w else None
    for f in lv["flows"][:-1]:
        for k, v in warp_census(f, w, h, orc.ITER_SCALE).items():
            tot[k] += v
        if tot["seam"] is not None:
            near = f[:, max(seam_x - r - 1, 0): seam_x + r + 2]
            tot["seam"] += int((~np.isfinite(near).all(axis=-1)).sum())
    return tot


def guarded_mask(orc, prev1, win, min_det):
    """The pixels of a level the determinant guard zeroes, from the oracle's own sums (include/ofx.h, ofx_lk_desc.min_det)"""
    s = orc.level_planes(synth.to_3ch(prev1), synth.to_3ch(prev1), win, 1, exact_sums=True)[3]
    det = (s[0] * s[1] - s[2] * s[2]).astype(np.float32)       # float-valued 24-bit sums: exact products, one rounding, then float
    return ~(det >= np.float32(min_det))


# ---- lk_float_fast, step by step -------------------------------------------------------------------------------------------
def fast_exempt(orc, prev1, warped1, win):
    """(h, w, 2) bool: the pixel-steps csrc/lk_solve.h excepts from its 1-ulp bound -- a numerator that cancels -- and the bound
    they get instead, from the ORACLE's sums of the step (exact sums rounded to float; integer arithmetic):
        det != 0  and  |num| < 2^-24 (|term1| + |term2|)      with u: num = -Syy Sxt + Sxy Syt,  v: num = Sxy Sxt - Sxx Syt
    and for those  |got - want| <= 8 * 2^-53 (|term1| + |term2|) / |det|  (+ one float ulp of want, added by the caller)."""
    s = orc.level_planes(synth.to_3ch(prev1), synth.to_3ch(warped1), win, 1, exact_sums=True)[3]
    a, d, b, xt, yt = (np.asarray(x, np.float64).astype(np.int64) for x in s)   # integers below 2^33; products below 2^62
    det = a * d - b * b
    ex = np.zeros(a.shape + (2,), bool)
    bound = np.zeros(a.shape + (2,), np.float64)
    for c, (t1, t2) in enumerate(((-(d * xt), b * yt), (b * xt, -(a * yt)))):
        num = t1 + t2
        mag = np.abs(t1).astype(object) + np.abs(t2).astype(object)             # Python integers: the comparison is exact
        small = np.abs(num).astype(object) * (1 << 24) < mag
        ex[..., c] = (det != 0) & small.astype(bool)
        with np.errstate(divide="ignore", invalid="ignore"):
            bound[..., c] = 8.0 * 2.0 ** -53 * mag.astype(np.float64) / np.abs(det).astype(np.float64)
    return ex, bound


def check_fast_step(orc, prev1, next1, win, f_j, f_j1, what):
    """One accumulating iteration of an lk_float_fast session against the oracle's step from the session's own F_j: W = warp(next,
    F_j), D = the unguarded exact solve of (prev, W); F_{j+1} must have the NaN / Inf of F_j + D and lie, where finite, in the closed
    interval spanned by float32(F_j + d), d in {D - 1 ulp, D, D + 1 ulp} (lk_solve.h: "within 1 float ulp"); the
    pixel-steps of fast_exempt take its bound instead.  Returns (pixel-steps, exempt ones)."""
    f_j, f_j1 = np.asarray(f_j, np.float32), np.asarray(f_j1, np.float32)
    w1 = orc.warp_bilinear_u8(next1, f_j)
    dd = orc.lk_iter_level(prev1, w1, win, 1)[0]
    with np.errstate(invalid="ignore", over="ignore"):
        want = f_j + dd
        cand = np.stack([f_j + np.nextafter(dd, np.float32(-np.inf)), want, f_j + np.nextafter(dd, np.float32(np.inf))])
    assert np.array_equal(np.isnan(f_j1), np.isnan(want)), f"{what}: NaN positions differ"
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(f_j1), inf) and np.array_equal(f_j1[inf], want[inf]), f"{what}: Inf positions or signs differ"
    fin = np.isfinite(want)
    ex, bound = fast_exempt(orc, prev1, w1, win)
    ex &= fin
    with np.errstate(invalid="ignore"):
        cand = np.where(np.isfinite(cand), cand, np.nan)
        lo, hi = np.fmin.reduce(cand, axis=0), np.fmax.reduce(cand, axis=0)
        inside = (f_j1 >= lo) & (f_j1 <= hi)
        ulp = np.spacing(np.abs(want)).astype(np.float64)
        loose = np.abs(f_j1.astype(np.float64) - want.astype(np.float64)) <= bound + ulp
    bad = fin & ~np.where(ex, loose, inside)
    assert not bad.any(), f"{what}: {int(bad.sum())} values outside the 1-ulp interval, first at {np.argwhere(bad)[:3].tolist()}"
    return int(fin.sum()), int(ex.sum())


# ---- cases -----------------------------------------------------------------------------------------------------------------
# kind "pair": engine.flow_pair (pair at a time); "stream": a streamed session of 2 B + 1 frames.  w, h: level 0.  seam_x, level,
# block: hard_frames.  env: OFX_* variables the session is created under.
Case = namedtuple("Case", "id kind w h levels win iters B seam_x level block env corner")


def _case(id, kind, w, h, levels, win, iters, B=0, seam_x=None, level=0, block=(40, 90), env=(), corner=0):
    return Case(id, kind, w, h, levels, win, iters, B, seam_x, level, block, tuple(env), corner)


def _a1(win):
    """A: two tiles of the accumulating launch, the second one column wide, an odd width"""
    ow = tile_out_w(win >> 1)
    return _case(f"A-win{win}", "pair", ow + 1, 67, 1, win, 3, seam_x=ow)


def _a2(win):
    """... and as level 1 of a pair twice as large (the block doubled, so that level 1 sees whole flat windows)"""
    ow = tile_out_w(win >> 1)
    return _case(f"A2-win{win}", "pair", 2 * (ow + 1), 132, 2, win, 3, seam_x=ow, level=1, block=(80, 180))


def _c(win, w1, iters, B, env=(), tag=""):
    """C: level-1 width w1 around the tile of the fused launch (windows up to 9x9; above, the accumulating launch's), height 33"""
    r = win >> 1
    seam = pair_out_w(r) if r <= 4 else tile_out_w(r)
    return _case(f"C-win{win}-w{w1}-it{iters}-B{B}{tag}", "stream", 2 * w1, 66, 2, win, iters, B, seam_x=min(seam, w1 - 1), level=1,
                 block=(44, 180), env=env)


A_CASES = [_a1(win) for win in range(3, 24, 2)] + [_a2(win) for win in (11, 13, 17, 19, 21, 23)]
_P9 = pair_out_w(4)
C_CASES = [
    _c(9, _P9 - 1, 4, 1), _c(9, _P9 + 1, 5, 2), _c(9, 2 * _P9 + 1, 4, 2), _c(9, 2 * _P9 + 1, 5, 1),
    _c(3, pair_out_w(1) + 1, 5, 1), _c(5, pair_out_w(2) + 1, 4, 2), _c(7, pair_out_w(3) + 1, 5, 2),
    _c(9, _P9 + 1, 5, 1, env=(("OFX_PAIR_PACK", "1"), ("OFX_PAIR_WAVES", "3")), tag="-packed"),
    _c(11, tile_out_w(5) + 1, 4, 1), _c(15, tile_out_w(7) + 1, 5, 2),
]
_BY_ID = {c.id: c for c in A_CASES + C_CASES}
# D: the determinant guard (MIN_DET) on two cases of A and two of C, and a three-level streamed case (the guarded pixel 0 of a
# coarse level feeds the shift: a black corner of 48 pixels leaves pixel 0 of levels 1 and 2 without texture -- NaN unguarded, a
# shift out of the image; (0, 0) guarded, no shift -- which test_census_of_the_guarded_cases asserts); the block is 56 rows so
# that level 2 (116 x 34) still holds flat 11 x 11 windows
D_CASES = [_BY_ID["A-win9"], _BY_ID["A-win15"], _BY_ID[f"C-win9-w{_P9 + 1}-it5-B2"], _BY_ID[f"C-win5-w{pair_out_w(2) + 1}-it4-B2"],
           _case("D-3level", "stream", 464, 136, 3, 9, 5, 1, seam_x=_P9, block=(56, 120), corner=48)]
# E: lk_float_fast step by step: every window pair at a time (the fast ITER 3, 2 and 1 of every radius; the windows that were here
# first come first), and two streamed cases
E_CASES = [_BY_ID[f"A-win{win}"] for win in (3, 9, 15, 23, 5, 7, 11, 13, 17, 19, 21)] + [_BY_ID[f"C-win9-w{_P9 + 1}-it5-B2"], _BY_ID[f"C-win5-w{pair_out_w(2) + 1}-it4-B2"]]
# B: tiny and degenerate shapes, synth.random_pair, no census
B_SHAPES = [(5, 3, 3), (2, 2, 9), (1, 1, 3), (9, 4, 23), (37, 21, 5)]


def n_frames(case):
    return 2 if case.kind == "pair" else 2 * case.B + 1


def case_frames(case):
    return hard_frames(case.w, case.h, n_frames(case), seam_x=case.seam_x, level=case.level, block=case.block, corner=case.corner)


def level_seam(case, k):
    """the seam column the census looks at on level k: the case's tile boundary, where the level is wide enough to have it"""
    return case.seam_x if case.seam_x is not None and case.seam_x < (case.w >> k) else None
