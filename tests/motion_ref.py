"""Referee of motion compensation (ofx_motion_compensate, ofx_session_stream_motion): the definition in include/ofx.h
("motion compensation") restated in plain NumPy, every float32 operation spelled out and rounded once, plus the seeded inputs
the CPU and the GPU tests share.  Not a test module and not a conftest: tests import it.

tests/test_motion_ref.py pins shift() and warp() against the oracle (oracle.shift_back_pyramid on channel 0 with a zero
destination, oracle.warp_bilinear_u8) on exactly these inputs."""
import numpy as np

F32 = np.float32
ITER_SCALE = F32(8.0 / 15.0)

SIZES = [(67, 33), (130, 9), (257, 40), (4, 1), (1, 5)]   # (w, h)


def shift(next1, uv):
    """ofx_shift_1ch: next((int)(x + u), (int)(y + v)) when that lands inside the image (> -1 and < w, float compare; truncation
    toward zero), else next(x, y) if 3 * (y * w + x) < w * h, else 0."""
    next1 = np.asarray(next1, np.uint8)
    h, w = next1.shape
    u, v = (F32(0), F32(0)) if uv is None else (F32(uv[0]), F32(uv[1]))
    with np.errstate(invalid="ignore", over="ignore"):
        tx = (np.arange(w, dtype=F32) + u).astype(F32)               # one float32 add
        ty = (np.arange(h, dtype=F32) + v).astype(F32)
        xin = (tx > F32(-1.0)) & (tx < F32(w))                        # a NaN fails both
        yin = (ty > F32(-1.0)) & (ty < F32(h))
    nx = np.where(xin, tx, F32(0)).astype(np.int64)                   # truncation toward zero
    ny = np.where(yin, ty, F32(0)).astype(np.int64)
    inside = yin[:, None] & xin[None, :]
    pos = np.arange(h, dtype=np.int64)[:, None] * w + np.arange(w, dtype=np.int64)[None, :]
    own = np.where(3 * pos < w * h, next1, np.uint8(0))
    return np.where(inside, next1[ny[:, None], nx[None, :]], own).astype(np.uint8)


def warp(src1, flow, scale):
    """ofx_warp_levels / orc_warp_bilinear_u8: (mc, not_warped mask)."""
    src1, flow, scale = np.asarray(src1, np.uint8), np.asarray(flow, F32), F32(scale)
    h, w = src1.shape
    xs, ys = np.arange(w, dtype=F32)[None, :], np.arange(h, dtype=F32)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        sx = (xs + (scale * flow[..., 0]).astype(F32)).astype(F32)   # product rounded, then the sum
        sy = (ys + (scale * flow[..., 1]).astype(F32)).astype(F32)
        ok = (sx >= F32(-1e9)) & (sx <= F32(1e9)) & (sy >= F32(-1e9)) & (sy <= F32(1e9))
    sx = np.where(ok, sx, F32(0))
    sy = np.where(ok, sy, F32(0))
    sx = np.where(sx < F32(0), F32(0), np.where(sx > F32(w - 1), F32(w - 1), sx)).astype(F32)   # replicate border
    sy = np.where(sy < F32(0), F32(0), np.where(sy > F32(h - 1), F32(h - 1), sy)).astype(F32)
    x0, y0 = sx.astype(np.int64), sy.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    fx, fy = (sx - x0.astype(F32)).astype(F32), (sy - y0.astype(F32)).astype(F32)
    p00, p01 = src1[y0, x0].astype(F32), src1[y0, x1].astype(F32)
    p10, p11 = src1[y1, x0].astype(F32), src1[y1, x1].astype(F32)
    a = (p00 + (fx * (p01 - p00).astype(F32)).astype(F32)).astype(F32)
    b = (p10 + (fx * (p11 - p10).astype(F32)).astype(F32)).astype(F32)
    v = (a + (fy * (b - a).astype(F32)).astype(F32)).astype(F32)
    out = (v + F32(0.5)).astype(F32).astype(np.int64).astype(np.uint8)
    return np.where(ok, out, src1).astype(np.uint8), ~ok


def sums(prev1, next1, mc, not_warped):
    prev1 = np.asarray(prev1, np.int64)
    return np.array([prev1.size, np.abs(prev1 - np.asarray(next1, np.int64)).sum(), np.abs(prev1 - np.asarray(mc, np.int64)).sum(),
                     int(np.count_nonzero(not_warped))], np.int64)


def motion(prev1, next1, flow, uv, scale):
    """(mc uint8 [h, w], stats int64 [4]) of the definition."""
    mc, bad = warp(shift(next1, uv), flow, scale)
    return mc, sums(prev1, next1, mc, bad)


# ---- the inputs the tests share -------------------------------------------------------------------------------------------------

def uv_cases(w, h):
    """(0, 0); the map's collapse at 0; two general shifts; everything out (the one-third rule over the whole image); a NaN; 1e30"""
    return [None, (0.0, 0.0), (-0.5, -0.5), (3.7, -2.2), (-3.2, 5.9), (float(w + 5), 0.0), (float("nan"), 1.0), (1e30, 0.0)]


FLOW_KINDS = ["random", "integers", "borders", "nonfinite", "corner"]


def planes(w, h, seed):
    rng = np.random.default_rng(1000 * seed + 7 * w + h)
    return rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w), dtype=np.uint8)


def flow_case(kind, w, h, seed):
    """(flow float32 [h, w, 2], scale)"""
    rng = np.random.default_rng(100 * seed + 13 * w + h + 7 * FLOW_KINDS.index(kind))
    if kind == "integers":                                   # fractions 0: scale 1, whole pixels
        return rng.integers(-3, 4, (h, w, 2)).astype(F32), F32(1.0)
    scale = ITER_SCALE
    flow = (rng.uniform(-6.0, 6.0, (h, w, 2)) / float(scale)).astype(F32)   # taps within +-6 px
    if kind == "borders":                                    # taps pushed beyond all four borders
        far = F32(max(w, h) + 7.3) / scale
        pick = rng.integers(0, 5, (h, w))
        flow[..., 0] = np.where(pick == 1, -far, np.where(pick == 2, far, flow[..., 0]))
        flow[..., 1] = np.where(pick == 3, -far, np.where(pick == 4, far, flow[..., 1]))
    elif kind == "nonfinite":
        vals = np.array([np.nan, np.inf, -np.inf, 1e12, -1e12], F32)
        hit = rng.random((h, w, 2)) < 0.08
        flow = np.where(hit, vals[rng.integers(0, len(vals), (h, w, 2))], flow).astype(F32)
        for i, val in enumerate(vals):                       # and in whole rows
            if i < h:
                flow[(i * 3) % h, :, i % 2] = val
    elif kind == "corner":                                   # the last pixel points further out
        flow[h - 1, w - 1] = (F32(50.0), F32(50.0))
    return flow, scale


def stateless_cases():
    """(id, w, h, prev, next, flow, uv, scale) of every size x shift x flow kind"""
    for si, (w, h) in enumerate(SIZES):
        prev1, next1 = planes(w, h, si)
        for ui, uv in enumerate(uv_cases(w, h)):
            for kind in FLOW_KINDS:
                flow, scale = flow_case(kind, w, h, 10 * si + ui)
                yield f"{w}x{h}-uv{ui}-{kind}", w, h, prev1, next1, flow, uv, scale
