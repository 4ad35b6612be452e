"""Referee of the coarse-to-fine dense flow (ofx_flow_prolong, ofx_session_run_flow_dense, engine.flow_pair_dense,
engine.video_displacement_dense, engine.video_interpolate_dense): the block "coarse-to-fine propagation" of include/ofx.h restated
in plain NumPy float32, every operation spelled out and rounded once, the pair's dense flow composed from existing oracle calls,
and the scenes and the score of the quality experiment.  Not a test module and not a conftest: tests import it.

tests/test_dense_ref.py pins prolong() on hand-made fields and measures the quality on the oracle alone."""
import functools

import numpy as np

import interp_ref as IR

F32 = np.float32
ITER_SCALE = IR.ITER_SCALE


# ---- "coarse-to-fine propagation" -----------------------------------------------------------------------------------------------

def sanitise(coarse, scale, max_px):
    """a coarse vector becomes (0, 0) when a component is not finite or, with max_px > 0, when |scale * component| > max_px (the
    product rounded once to float32)"""
    c = np.array(coarse, F32)                                  # (a copy)
    assert c.ndim == 3 and c.shape[2] == 2
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        bad = ~np.isfinite(c).all(axis=2)
        if max_px > 0:
            bad |= (np.abs((F32(scale) * c).astype(F32)) > F32(max_px)).any(axis=2)   # (`>` is false for a NaN)
    c[bad] = F32(0)
    return c


def _half(c, n, axis):
    """the rule along one axis: fine position i reads coarse i / 2 -- tap i0 itself at even i, a + 0.5 * (b - a) at odd i"""
    nc = c.shape[axis]
    i = np.arange(n)
    i0 = np.minimum(i >> 1, nc - 1)
    i1 = np.minimum(i0 + 1, nc - 1)
    a, b = np.take(c, i0, axis=axis), np.take(c, i1, axis=axis)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        mid = (a + (F32(0.5) * (b - a).astype(F32)).astype(F32)).astype(F32)
    odd = (i & 1).astype(bool).reshape([-1 if d == axis else 1 for d in range(c.ndim)])
    return np.where(odd, mid, a).astype(F32)


def prolong(coarse, w, h, scale=ITER_SCALE, max_px=0.0):
    """fine float32 [h, w, 2] of the coarse field [hc, wc, 2]: sanitise, sample at (x / 2, y / 2) horizontally first, times 2"""
    c = sanitise(coarse, scale, max_px)
    hc, wc = c.shape[:2]
    assert w in (2 * wc, 2 * wc + 1) and h in (2 * hc, 2 * hc + 1), (w, h, wc, hc)
    v = _half(_half(c, w, 1), h, 0)
    with np.errstate(invalid="ignore", over="ignore"):
        return (F32(2.0) * v).astype(F32)


def same_bits(got, want):
    """bool array: the float32 values have the same bits.  Two NaNs count as the same: the definition makes a NaN only by
    Inf - Inf of huge unsanitised vectors (max_px = 0), and IEEE 754 leaves such a NaN's sign and payload to the hardware (x86
    sets the sign, gfx950 does not)."""
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    assert got.shape == want.shape, (got.shape, want.shape)
    return (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))


# ---- a pair's dense flow, from the oracle's calls -------------------------------------------------------------------------------

def _pyr1(orc, img1, levels):
    return [np.ascontiguousarray(p[:, :, 0]) for p in orc.gauss_pyramid(np.repeat(np.asarray(img1, np.uint8)[:, :, None], 3, 2), levels)]


def dense_pair(orc, prev1, next1, levels, window, iters, min_det=0.0, max_px=None, trace=None):
    """The flow pyramid of the definition, lk_float: the top level as the session runs it (iteration 1 the reference's level, then
    iters - 1 refinement iterations); every level below starts from the prolonged flow of the level above and runs `iters`
    accumulating iterations on the UNSHIFTED next image.  max_px None: the window.  trace (a list): receives (level, prolonged
    flow, its warped image) of every level below the top."""
    iters = max(int(iters), 1)
    max_px = float(window) if max_px is None else float(max_px)
    pp, npyr = _pyr1(orc, prev1, levels), _pyr1(orc, next1, levels)
    flow = [None] * levels
    flow[levels - 1] = orc.lk_iter_level(pp[-1], npyr[-1], window, iters, min_det)[0]
    for k in range(levels - 2, -1, -1):
        h, w = pp[k].shape
        f = prolong(flow[k + 1], w, h, ITER_SCALE, max_px)
        warped = orc.warp_bilinear_u8(npyr[k], f)
        if trace is not None:
            trace.append((k, f.copy(), warped.copy()))
        for i in range(iters):
            with np.errstate(invalid="ignore", over="ignore"):
                f = (f + orc.lk_iter_level(pp[k], warped, window, 1, min_det)[0]).astype(F32)
            if i + 1 < iters:
                warped = orc.warp_bilinear_u8(npyr[k], f)
        flow[k] = f
    return flow


def dense_displacement(orc, prev1, next1, levels, window, iters, min_det=0.0, max_px=None, level=0):
    """the level's displacement in pixels: OFX_ITER_SCALE * flow_k, as ofx_flow_displacement returns it with d_uv = NULL"""
    return IR.displacement(dense_pair(orc, prev1, next1, levels, window, iters, min_det, max_px)[level], None, ITER_SCALE)


def existing_displacement(orc, prev1, next1, levels, window, iters, min_det=0.0):
    """the level-0 displacement of the reference's way: floor(uv) + OFX_ITER_SCALE * flow_0, uv the global shift accumulated from
    pixel 0 of the coarser levels' first-iteration flows (cpu::shift_back_pyramid), flow_0 the iterated level-0 flow"""
    pp, npyr = _pyr1(orc, prev1, levels), _pyr1(orc, next1, levels)
    h, w = np.asarray(prev1).shape
    first = [np.zeros((h >> k, w >> k, 2), F32) for k in range(levels)]
    out = [None] * levels
    for k in range(levels - 1, -1, -1):
        n3 = np.repeat(npyr[k][:, :, None], 3, 2)
        nxt = npyr[k] if k == levels - 1 else np.ascontiguousarray(orc.shift_back_pyramid(n3, k, levels, first)[:, :, 0])
        out[k], first[k] = orc.lk_iter_level(pp[k], nxt, window, iters, min_det)
    u = v = F32(0)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(levels - 1, 0, -1):
            u, v = F32(u + F32(F32(1 << k) * first[k][0, 0, 0])), F32(v + F32(F32(1 << k) * first[k][0, 0, 1]))
    return IR.displacement(out[0], (u, v), ITER_SCALE)


# ---- the quality experiment -----------------------------------------------------------------------------------------------------

S_W, S_H, S_LEVELS, S_WIN, S_ITERS, S_MIN_DET = 192, 128, 4, 9, 3, 1.0
S_SEEDS = (41, 7, 3)
SCENES = {"pan": ((9.0, 5.0), (9.0, 5.0)), "split": ((7.0, 3.0), (-6.0, -2.0)), "split2": ((0.0, 0.0), (8.0, -4.0)),
          "small": ((1.2, -0.6), (1.2, -0.6))}
BORDER = SEAM = 20


@functools.lru_cache(maxsize=None)
def scene(name, seed, w=S_W, h=S_H):
    """(prev, next, truth float32 [h, w, 2]): the texture of synth.smooth_pair(w, h, ., ., seed); the left half of `next` has moved
    by dA, the right half by dB"""
    from cuda_optical_flow_2_amd import synth

    dA, dB = SCENES[name]
    prev, na = synth.smooth_pair(w, h, dA[0], dA[1], seed=seed)
    nb = synth.smooth_pair(w, h, dB[0], dB[1], seed=seed)[1]
    nxt = na.copy()
    nxt[:, w // 2:] = nb[:, w // 2:]
    truth = np.empty((h, w, 2), F32)
    truth[:, : w // 2] = dA
    truth[:, w // 2:] = dB
    for a in (prev, nxt, truth):
        a.setflags(write=False)
    return prev, nxt, truth


def score(disp, truth):
    """the share of pixels whose displacement is within 1 px of the truth in both components (a non-finite value is a miss),
    outside a 20 px border and the columns within 20 px either side of the seam at w / 2"""
    disp, truth = np.asarray(disp, F32), np.asarray(truth, F32)
    h, w, _ = truth.shape
    keep = np.zeros((h, w), bool)
    keep[BORDER: h - BORDER, BORDER: w - BORDER] = True
    keep[:, w // 2 - SEAM: w // 2 + SEAM] = False
    with np.errstate(invalid="ignore"):
        hit = (np.abs(disp - truth) <= F32(1.0)).all(axis=2)      # (a NaN or an Inf fails)
    return float(hit[keep].sum()) / float(keep.sum())


def interp_ratios(frames, disp_of):
    """SAD(in-between) / SAD(cross-fade) of the six in-between frames of the clip frames[0], [4], [8] (interp_ref.quality_clip);
    disp_of(i, j): the level-0 displacement of frame i -> frame j"""
    ratios = []
    for i, j in ((0, 4), (4, 8)):
        dab, dba = disp_of(i, j), disp_of(j, i)
        for k in (1, 2, 3):
            t = F32(k / 4)
            got = IR.interpolate(frames[i], frames[j], dab, dba, t)[0]
            ratios.append(IR.sad(got, frames[i + k]) / IR.sad(IR.cross_fade(frames[i], frames[j], t), frames[i + k]))
    return ratios


# ---- the coarse fields the tests share ------------------------------------------------------------------------------------------

P_SCALE, P_MAX_PX = ITER_SCALE, 9.0
P_SHAPES = [((131, 37), (262, 74)), ((131, 37), (263, 75)), ((5, 3), (10, 6)), ((1, 1), (2, 2)), ((1, 1), (3, 3)), ((130, 9), (260, 18))]   # (wc, hc), (w, h)
P_KINDS = ["smooth", "noise", "salted"]


def threshold(scale=P_SCALE, max_px=P_MAX_PX):
    """(lim, above): the largest float32 whose rounded product with the scale is <= max_px, and the next one"""
    scale = F32(scale)
    lim = F32(max_px / float(scale))
    while F32(scale * lim) > F32(max_px):
        lim = np.nextafter(lim, F32(0))
    while F32(scale * np.nextafter(lim, F32(np.inf))) <= F32(max_px):
        lim = np.nextafter(lim, F32(np.inf))
    return lim, np.nextafter(lim, F32(np.inf))


@functools.lru_cache(maxsize=None)
def coarse_case(kind, wc, hc):
    """a coarse field float32 [hc, wc, 2] in OFX_ITER_SCALE units: 'smooth' (a few pixels, slowly varying), 'noise' (uniform, up to
    +-20 px: some beyond max_px = 9), 'salted' (the noise with one vector in five hit by NaN, +-Inf, +-1e30, the two values either
    side of the max_px threshold, -0.0, and vectors of hundreds and of 1e8 pixels, which send the warp's taps to every border)"""
    rng = np.random.default_rng(17 * wc + hc + 5 * P_KINDS.index(kind))
    ys, xs = np.mgrid[0:hc, 0:wc].astype(np.float64)
    if kind == "smooth":
        f = np.stack([3.0 * np.sin(xs / 9.0 + ys / 5.0) + 1.5, 2.0 * np.cos(xs / 7.0 - ys / 11.0) - 0.7], axis=2) / float(ITER_SCALE)
        f = f.astype(F32)
    else:
        f = (rng.uniform(-20.0, 20.0, (hc, wc, 2)) / float(ITER_SCALE)).astype(F32)
    if kind == "salted":
        lim, above = threshold()
        vals = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, lim, -lim, above, -above, -0.0, 0.0, 600.0, -600.0, 1.5e8, -1.5e8], F32)
        hit = rng.random((hc, wc, 2)) < 0.1
        f[hit] = vals[rng.integers(0, len(vals), int(hit.sum()))]
        flat = f.reshape(-1)
        flat[: min(len(vals), flat.size)] = vals[: min(len(vals), flat.size)]     # every value at least once, where the field is large enough
    f.setflags(write=False)
    return f
