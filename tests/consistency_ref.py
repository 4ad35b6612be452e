"""Referee of the forward-backward check (ofx_flow_consistency, ofx_flow_consistency_batch, engine.video_consistency): the
definition in include/ofx.h ("forward-backward consistency") restated in plain NumPy, every float32 operation spelled out and
rounded once, plus the seeded inputs the CPU and the GPU tests share.  Not a test module and not a conftest: tests import it.

tests/test_consistency_ref.py pins the tap geometry and the blend against motion_ref.warp, which is itself pinned against the
oracle (tests/test_motion_ref.py)."""
import functools

import numpy as np

F32 = np.float32
ITER_SCALE = F32(8.0 / 15.0)
FLT_MAX = F32(np.finfo(np.float32).max)
INF = F32(np.inf)
CONSISTENT, INCONSISTENT, LEAVES, UNDEFINED = 0, 1, 2, 3

SIZES = [(67, 33), (130, 9), (257, 40), (4, 1), (1, 5)]   # (w, h)
LARGE = SIZES[:3]
KINDS = ["inverse", "integers", "borders", "nonfinite", "edge"]
ALPHA, BETA_PX2 = 0.01, 0.5


def beta_of(beta_px2, scale):
    """beta in squared field units: beta_px2 / scale^2 in float64, rounded once to float32 (engine._beta)"""
    s = np.float64(F32(scale))
    return F32(np.float64(beta_px2) / (s * s))


def consistency(fwd, bwd, scale, alpha, beta, parts=False):
    """(mask uint8 [h, w], err float32 [h, w], stats int64 [4]) of the definition; with parts, also a dict of px, py and r_u."""
    fwd, bwd = np.asarray(fwd, F32), np.asarray(bwd, F32)
    scale, alpha, beta = F32(scale), F32(alpha), F32(beta)
    h, w, _ = fwd.shape
    assert bwd.shape == fwd.shape == (h, w, 2)
    u, v = fwd[..., 0], fwd[..., 1]
    xs, ys = np.arange(w, dtype=F32)[None, :], np.arange(h, dtype=F32)[:, None]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        px = (xs + (scale * u).astype(F32)).astype(F32)                       # 1. the product rounded, then the sum
        py = (ys + (scale * v).astype(F32)).astype(F32)
        ok = (np.abs(px) <= F32(1e9)) & (np.abs(py) <= F32(1e9))              # 2. (a NaN fails)
        gone = (px < F32(0)) | (px > F32(w - 1)) | (py < F32(0)) | (py > F32(h - 1))   # 3.
        live = ok & ~gone
        sx, sy = np.where(live, px, F32(0)).astype(F32), np.where(live, py, F32(0)).astype(F32)
        x0, y0 = sx.astype(np.int64), sy.astype(np.int64)                     # 4. truncation; sx, sy >= 0
        fx, fy = (sx - x0.astype(F32)).astype(F32), (sy - y0.astype(F32)).astype(F32)
        x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)

        def blend(plane):                                                     # 5.
            b00, b01, b10, b11 = plane[y0, x0], plane[y0, x1], plane[y1, x0], plane[y1, x1]
            a = (b00 + (fx * (b01 - b00).astype(F32)).astype(F32)).astype(F32)
            c = (b10 + (fx * (b11 - b10).astype(F32)).astype(F32)).astype(F32)
            return (a + (fy * (c - a).astype(F32)).astype(F32)).astype(F32)

        ru, rv = blend(bwd[..., 0]), blend(bwd[..., 1])
        du, dv = (u + ru).astype(F32), (v + rv).astype(F32)                   # 6.
        e = ((du * du).astype(F32) + (dv * dv).astype(F32)).astype(F32)
        m = (((u * u).astype(F32) + (v * v).astype(F32)).astype(F32) + ((ru * ru).astype(F32) + (rv * rv).astype(F32)).astype(F32)).astype(F32)
        thr = ((alpha * m).astype(F32) + beta).astype(F32)
        finite = np.abs(e) <= FLT_MAX                                         # 7.
        within = e <= thr
    mask = np.where(~ok, UNDEFINED, np.where(gone, LEAVES, np.where(~finite, UNDEFINED, np.where(within, CONSISTENT, INCONSISTENT)))).astype(np.uint8)
    err = np.where(mask <= INCONSISTENT, e, INF).astype(F32)
    stats = np.array([w * h] + [int(np.count_nonzero(mask == c)) for c in (1, 2, 3)], np.int64)
    if parts:
        return mask, err, stats, {"px": px, "py": py, "ru": ru}
    return mask, err, stats


# ---- the inputs the tests share -------------------------------------------------------------------------------------------------

def _inverse(rng, w, h):
    """a translation t from [-2.5, 2.5]^2 px plus N(0, 0.35 px) noise, and -t plus the same kind of noise; in pixels"""
    t = rng.uniform(-2.5, 2.5, 2)
    return t + rng.normal(0.0, 0.35, (h, w, 2)), -t + rng.normal(0.0, 0.35, (h, w, 2))


@functools.lru_cache(maxsize=None)
def field_case(kind, w, h, seed=0):
    """(fwd float32 [h, w, 2], bwd float32 [h, w, 2], scale)"""
    rng = np.random.default_rng(100 * seed + 13 * w + h + 7 * KINDS.index(kind))
    xs, ys = np.arange(w)[None, :], np.arange(h)[:, None]
    if kind == "integers":                                   # scale 1, whole pixels: every fraction is 0
        fwd, bwd, scale = rng.integers(-3, 4, (h, w, 2)).astype(F32), rng.integers(-3, 4, (h, w, 2)).astype(F32), F32(1.0)
    elif kind == "edge":                                     # scale 1: the last column and the last row, exactly
        scale = F32(1.0)
        fwd = rng.choice([-0.5, 0.5], (h, w, 2)).astype(F32)
        pick = rng.integers(0, 3, (h, w))
        fwd[..., 0] = np.where(pick == 0, (w - 1 - xs).astype(F32), fwd[..., 0])
        fwd[..., 1] = np.where(pick == 1, (h - 1 - ys).astype(F32), fwd[..., 1])
        bwd = rng.choice([-0.5, 0.5], (h, w, 2)).astype(F32)
        bwd[:, 0, :] = np.nan                                # the memory neighbour of column w - 1 of the row above
    else:
        scale = ITER_SCALE
        f, b = _inverse(rng, w, h)
        if kind == "borders":                                # one vector in three pushed beyond one of the four borders
            far = max(w, h) + 7.3
            pick = rng.integers(0, 3, (h, w)) == 0
            side = rng.integers(0, 4, (h, w))
            f[..., 0] = np.where(pick & (side == 0), -far - xs, np.where(pick & (side == 1), (w - 1 - xs) + far, f[..., 0]))
            f[..., 1] = np.where(pick & (side == 2), -far - ys, np.where(pick & (side == 3), (h - 1 - ys) + far, f[..., 1]))
        fwd, bwd = (f / float(scale)).astype(F32), (b / float(scale)).astype(F32)
        if kind == "nonfinite":                              # in 4 % of the components of each field
            vals = np.array([np.nan, np.inf, -np.inf, 1e12, -1e12, 1e30, -1e30], F32)
            for fld in (fwd, bwd):
                hit = rng.random((h, w, 2)) < 0.04
                fld[hit] = vals[rng.integers(0, len(vals), int(hit.sum()))]
    fwd.setflags(write=False)
    bwd.setflags(write=False)
    return fwd, bwd, scale


def tolerances(scale):
    """the two (alpha, beta) pairs every comparison runs with"""
    return [(F32(ALPHA), beta_of(BETA_PX2, scale)), (F32(0.0), F32(0.0))]


@functools.lru_cache(maxsize=None)
def reference(kind, w, h, ti, seed=0):
    """(mask, err, stats) of field_case(kind, w, h, seed) with tolerances(scale)[ti]; computed once, not to be written to"""
    fwd, bwd, scale = field_case(kind, w, h, seed)
    alpha, beta = tolerances(scale)[ti]
    out = consistency(fwd, bwd, scale, alpha, beta)
    for a in out:
        a.setflags(write=False)
    return out
