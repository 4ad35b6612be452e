"""Referee of the flow median (ofx_flow_median, ofx_session_run_flow_dense_median, the engine's median= arguments): the block
"flow median" of include/ofx.h restated in plain NumPy, and the pair's dense flow with median composed from dense_ref.prolong and
the oracle's calls, as dense_ref.dense_pair is.  Not a test module and not a conftest: tests import it.

tests/test_median_ref.py pins median() on hand-made fields and measures the quality on the oracle alone."""
import functools

import numpy as np

import dense_ref as D

F32 = np.float32
ITER_SCALE = D.ITER_SCALE


def median(field, r):
    """float32 [h, w, 2]: sanitise (a vector with a component that is not finite reads as (+0, +0)), gather the (2r + 1)^2 window
    with the border replicated, order each component's values and take the middle one, then + 0 (a -0 result leaves as +0)"""
    assert r in (1, 2)
    f = np.array(field, F32)                                   # (a copy)
    assert f.ndim == 3 and f.shape[2] == 2
    h, w = f.shape[:2]
    f[~np.isfinite(f).all(axis=2)] = F32(0)
    ys = np.clip(np.arange(h)[:, None] + np.arange(-r, r + 1)[None, :], 0, h - 1)      # [h, 2r + 1]
    xs = np.clip(np.arange(w)[:, None] + np.arange(-r, r + 1)[None, :], 0, w - 1)      # [w, 2r + 1]
    win = f[ys[:, None, :, None], xs[None, :, None, :]]                                 # [h, w, 2r + 1, 2r + 1, 2]
    win = win.reshape(h, w, (2 * r + 1) ** 2, 2)
    mid = np.sort(win, axis=2)[:, :, (2 * r + 1) ** 2 // 2, :]
    return (mid + F32(0)).astype(F32)


def dense_pair_median(orc, prev1, next1, levels, window, iters, min_det=0.0, max_px=None, r=2):
    """The flow pyramid of "a pair's dense flow with median": dense_ref.dense_pair with one median after the top level and after
    every accumulating iteration below it; the next warped image is made from the FILTERED flow."""
    iters = max(int(iters), 1)
    max_px = float(window) if max_px is None else float(max_px)
    pp, npyr = D._pyr1(orc, prev1, levels), D._pyr1(orc, next1, levels)
    flow = [None] * levels
    flow[levels - 1] = median(orc.lk_iter_level(pp[-1], npyr[-1], window, iters, min_det)[0], r)
    for k in range(levels - 2, -1, -1):
        h, w = pp[k].shape
        f = D.prolong(flow[k + 1], w, h, ITER_SCALE, max_px)
        warped = orc.warp_bilinear_u8(npyr[k], f)
        for i in range(iters):
            with np.errstate(invalid="ignore", over="ignore"):
                f = (f + orc.lk_iter_level(pp[k], warped, window, 1, min_det)[0]).astype(F32)
            f = median(f, r)
            if i + 1 < iters:
                warped = orc.warp_bilinear_u8(npyr[k], f)
        flow[k] = f
    return flow


def dense_displacement_median(orc, prev1, next1, levels, window, iters, min_det=0.0, max_px=None, r=2, level=0):
    """the level's displacement in pixels: OFX_ITER_SCALE * flow_k (r = 0: dense_ref.dense_pair, no median)"""
    pyr = D.dense_pair(orc, prev1, next1, levels, window, iters, min_det, max_px) if r == 0 else \
        dense_pair_median(orc, prev1, next1, levels, window, iters, min_det, max_px, r)
    return D.IR.displacement(pyr[level], None, ITER_SCALE)


def seam_score(disp, truth):
    """dense_ref.score inside the band it excludes: the 40 columns around the seam at w / 2, inside the 20 px border"""
    disp, truth = np.asarray(disp, F32), np.asarray(truth, F32)
    h, w, _ = truth.shape
    keep = np.zeros((h, w), bool)
    keep[D.BORDER: h - D.BORDER, w // 2 - D.SEAM: w // 2 + D.SEAM] = True
    with np.errstate(invalid="ignore"):
        hit = (np.abs(disp - truth) <= F32(1.0)).all(axis=2)
    return float(hit[keep].sum()) / float(keep.sum())


# ---- the fields the tests share ---------------------------------------------------------------------------------------------------

M_SHAPES = [(1, 1), (2, 3), (4, 1), (5, 4), (63, 7), (65, 9), (262, 74), (263, 75)]      # (w, h)
M_KINDS = ["smooth", "noise", "salted", "ties"]
DENORM = (1e-45, -3e-39)


@functools.lru_cache(maxsize=None)
def field_case(kind, w, h):
    """a field float32 [h, w, 2]: dense_ref.coarse_case's 'smooth' / 'noise' / 'salted'; 'ties': every value drawn from five
    levels, +0, -0, two denormals and 1.5, so that the window's middle value has many equals; 'patched' (for the fused warp): the
    salted field with 9x9 patches of +-1e30 and of (Inf, 2), whose insides survive a 5x5 median as vectors that are not warped"""
    if kind == "patched":
        f = np.array(D.coarse_case("salted", w, h))
        if w >= 40 and h >= 40:
            f[3:12, 5:14] = F32(1e30)                         # (x + scale * u beyond 1e9: not warped)
            f[20:29, 30:39, 0], f[20:29, 30:39, 1] = F32(np.inf), F32(2.0)      # sanitised: zeros inside the patch
            f[h - 12: h - 3, w - 14: w - 5] = F32(-1e30)
        f.setflags(write=False)
        return f
    if kind != "ties":
        return D.coarse_case(kind, w, h)
    rng = np.random.default_rng(29 * w + h)
    vals = np.array([0.0, -0.0, DENORM[0], DENORM[1], 1.5], F32)
    f = vals[rng.integers(0, len(vals), (h, w, 2))]
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def want(kind, w, h, r):
    f = median(field_case(kind, w, h), r)
    f.setflags(write=False)
    return f
