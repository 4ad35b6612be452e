"""Referee of the pixel displacement and of frame interpolation (ofx_flow_displacement, ofx_session_stream_displacement,
ofx_interpolate_frames, ofx_interpolate_frames_batch, engine.video_displacement, engine.video_interpolate): the two definitions in
include/ofx.h ("pixel displacement", "frame interpolation") restated in plain NumPy, every float32 operation spelled out and
rounded once, plus the seeded inputs the CPU and the GPU tests share.  Not a test module and not a conftest: tests import it.

tests/test_interp_ref.py pins displacement() against motion_ref (itself pinned against the oracle) and interpolate() against
translations, its own symmetry and the oracle's flows."""
import functools

import numpy as np

F32 = np.float32
ITER_SCALE = F32(8.0 / 15.0)
MAX_TIMES = 8

SIZES = [(67, 33), (130, 9), (257, 40), (4, 1), (1, 5)]   # (w, h)
LARGE = SIZES[:3]
KINDS = ["inverse", "integers", "borders", "nonfinite", "edge"]
TIME_SETS = [(F32(0.5),), (F32(0.25), F32(0.5), F32(0.75)), tuple(F32(k / 9) for k in range(1, 9))]
UV_CASES = [None, (0.0, 0.0), (-0.5, -0.5), (3.7, -2.2), (float("nan"), 1.0), (1e30, 0.0)]


# ---- "pixel displacement" -------------------------------------------------------------------------------------------------------

def displacement(flow, uv, scale):
    """D float32 [h, w, 2] = (floorf(uv[0]) + scale*u, floorf(uv[1]) + scale*v): the product rounded, then the sum; uv None: 0.0f"""
    flow, scale = np.asarray(flow, F32), F32(scale)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        fl = (F32(0), F32(0)) if uv is None else (np.floor(F32(uv[0])).astype(F32), np.floor(F32(uv[1])).astype(F32))
        out = np.empty_like(flow)
        for c in (0, 1):
            out[..., c] = (fl[c] + (scale * flow[..., c]).astype(F32)).astype(F32)
    return out


# ---- "frame interpolation" ------------------------------------------------------------------------------------------------------

def coefficients(t):
    """the host step: (t, c00, c01, c10) in float32"""
    t = F32(t)
    omt = F32(F32(1.0) - t)
    return t, F32(-F32(omt * t)), F32(t * t), F32(omt * omt)


def _side(plane, px, py, xs, ys):
    """steps 3 to 5 for one side: (usable, V float32 [h, w])"""
    h, w = plane.shape
    fin = (np.abs(px) <= F32(1e9)) & (np.abs(py) <= F32(1e9))                                 # 3. (a NaN fails)
    usable = fin & (px >= F32(0)) & (px <= F32(w - 1)) & (py >= F32(0)) & (py <= F32(h - 1))
    cx, cy = np.where(fin, px, F32(0)).astype(F32), np.where(fin, py, F32(0)).astype(F32)
    cx = np.where(cx < F32(0), F32(0), np.where(cx > F32(w - 1), F32(w - 1), cx)).astype(F32)   # 4. replicate border
    cy = np.where(cy < F32(0), F32(0), np.where(cy > F32(h - 1), F32(h - 1), cy)).astype(F32)
    sx, sy = np.where(fin, cx, xs).astype(F32), np.where(fin, cy, ys).astype(F32)
    x0, y0 = sx.astype(np.int64), sy.astype(np.int64)                                         # 5. truncation; sx, sy >= 0
    fx, fy = (sx - x0.astype(F32)).astype(F32), (sy - y0.astype(F32)).astype(F32)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    p00, p01 = plane[y0, x0].astype(F32), plane[y0, x1].astype(F32)
    p10, p11 = plane[y1, x0].astype(F32), plane[y1, x1].astype(F32)
    r0 = (p00 + (fx * (p01 - p00).astype(F32)).astype(F32)).astype(F32)
    r1 = (p10 + (fx * (p11 - p10).astype(F32)).astype(F32)).astype(F32)
    return usable, (r0 + (fy * (r1 - r0).astype(F32)).astype(F32)).astype(F32)


def interpolate(a, b, dab, dba, t):
    """(out uint8 [h, w], stats int64 [4], cls uint8 [h, w]) of the definition at one time t"""
    a, b = np.asarray(a, np.uint8), np.asarray(b, np.uint8)
    dab, dba = np.asarray(dab, F32), np.asarray(dba, F32)
    h, w = a.shape
    assert b.shape == (h, w) and dab.shape == dba.shape == (h, w, 2)
    t, c00, c01, c10 = coefficients(t)
    xs = np.broadcast_to(np.arange(w, dtype=F32)[None, :], (h, w))
    ys = np.broadcast_to(np.arange(h, dtype=F32)[:, None], (h, w))
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        def two(c0, c1, comp):                                                                # 1. both products rounded, then the sum
            return ((c0 * dab[..., comp]).astype(F32) + (c1 * dba[..., comp]).astype(F32)).astype(F32)

        tax, tay, tbx, tby = two(c00, c01, 0), two(c00, c01, 1), two(c10, c00, 0), two(c10, c00, 1)
        ua, A = _side(a, (xs + tax).astype(F32), (ys + tay).astype(F32), xs, ys)              # 2. one add each
        ub, B = _side(b, (xs + tbx).astype(F32), (ys + tby).astype(F32), xs, ys)
        cls = np.where(ua & ub, 0, np.where(ua, 1, np.where(ub, 2, 3))).astype(np.uint8)      # 6.
        mix = (A + (t * (B - A).astype(F32)).astype(F32)).astype(F32)
        v = np.where(cls == 1, A, np.where(cls == 2, B, mix)).astype(F32)
        out = (v + F32(0.5)).astype(F32).astype(np.int64).astype(np.uint8)
    stats = np.array([w * h] + [int(np.count_nonzero(cls == c)) for c in (1, 2, 3)], np.int64)   # 7.
    return out, stats, cls


def interpolate_times(a, b, dab, dba, times):
    """(frames uint8 [T, h, w], stats int64 [T, 4]) of the definition at every time"""
    res = [interpolate(a, b, dab, dba, t) for t in times]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


# ---- the inputs the tests share -------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def planes(w, h, seed=0):
    """(a, b) uint8 [h, w]: two independent planes of uniform noise with 5 % of the pixels at 255 and 5 % at 0"""
    rng = np.random.default_rng(1000 * seed + 7 * w + h)
    out = []
    for _ in range(2):
        p = rng.integers(0, 256, (h, w), dtype=np.uint8)
        p[rng.random((h, w)) < 0.05] = 255
        p[rng.random((h, w)) < 0.05] = 0
        p.setflags(write=False)
        out.append(p)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def field_case(kind, w, h, seed=0):
    """(dab float32 [h, w, 2], dba float32 [h, w, 2]), both in pixels"""
    rng = np.random.default_rng(100 * seed + 13 * w + h + 7 * KINDS.index(kind))
    xs, ys = np.arange(w)[None, :], np.arange(h)[:, None]
    if kind == "integers":                                   # whole pixels: with t = 0.5 every fraction is a quarter
        dab, dba = rng.integers(-3, 4, (h, w, 2)).astype(F32), rng.integers(-3, 4, (h, w, 2)).astype(F32)
    elif kind == "edge":
        # at t = 0.5 (c00 = -0.25, c01 = c10 = 0.25) a sampling position exactly on column w - 1 or on row h - 1, on side a
        # (through dab, dba = 0 there) or on side b (through dba, dab = 0 there); elsewhere quarter-pixel positions
        dab, dba = rng.choice([-2.0, 2.0], (h, w, 2)).astype(F32), rng.choice([-2.0, 2.0], (h, w, 2)).astype(F32)
        pick = rng.integers(0, 6, (h, w))
        tox, toy = (-4.0 * (w - 1 - xs) + 0 * ys).astype(F32), (-4.0 * (h - 1 - ys) + 0 * xs).astype(F32)
        for p, fld, other, comp, val in ((0, dab, dba, 0, tox), (1, dab, dba, 1, toy), (2, dba, dab, 0, tox), (3, dba, dab, 1, toy)):
            m = pick == p
            fld[m] = 0
            other[m] = 0
            fld[..., comp][m] = val[m]
    else:
        tr = rng.uniform(-2.5, 2.5, 2)
        f, b = tr + rng.normal(0.0, 0.35, (h, w, 2)), -tr + rng.normal(0.0, 0.35, (h, w, 2))
        if kind == "borders":
            # one pixel in three: a long vector along one axis in dab, in dba or in both, of a length between a few pixels and
            # several image sizes: at every time some positions of side a only, of side b only and of both lie beyond a border
            pick = rng.integers(0, 3, (h, w)) == 0
            which, axis = rng.integers(0, 3, (h, w)), rng.integers(0, 2, (h, w))
            far = np.exp(rng.uniform(np.log(2.0), np.log(12.0 * (max(w, h) + 7.3)), (h, w))) * rng.choice([-1.0, 1.0], (h, w))
            for fld, sel in ((f, (0, 2)), (b, (1, 2))):
                for comp in (0, 1):
                    m = pick & np.isin(which, sel) & (axis == comp)
                    fld[..., comp] = np.where(m, far if fld is f else -0.7 * far, fld[..., comp])
        dab, dba = f.astype(F32), b.astype(F32)
        if kind == "nonfinite":                              # in 4 % of the components of each field
            vals = np.array([np.nan, np.inf, -np.inf, 1e12, -1e12, 1e30, -1e30], F32)
            for fld in (dab, dba):
                hit = rng.random((h, w, 2)) < 0.04
                fld[hit] = vals[rng.integers(0, len(vals), int(hit.sum()))]
    dab.setflags(write=False)
    dba.setflags(write=False)
    return dab, dba


@functools.lru_cache(maxsize=None)
def reference(kind, w, h, ts, seed=0):
    """(frames [T, h, w], stats [T, 4]) of planes(w, h, seed), field_case(kind, w, h, seed) at TIME_SETS[ts]; computed once, not to
    be written to"""
    a, b = planes(w, h, seed)
    dab, dba = field_case(kind, w, h, seed)
    out = interpolate_times(a, b, dab, dba, TIME_SETS[ts])
    for x in out:
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def flow_case(kind, w, h):
    """a flow for displacement(): 'iter' in OFX_ITER_SCALE units (+-6 px), 'nonfinite' the same with NaN, +-Inf, +-1e12, +-1e30 in 8 %"""
    rng = np.random.default_rng(31 * w + h + (5 if kind == "nonfinite" else 0))
    flow = (rng.uniform(-6.0, 6.0, (h, w, 2)) / float(ITER_SCALE)).astype(F32)
    if kind == "nonfinite":
        vals = np.array([np.nan, np.inf, -np.inf, 1e12, -1e12, 1e30, -1e30], F32)
        hit = rng.random((h, w, 2)) < 0.08
        flow[hit] = vals[rng.integers(0, len(vals), int(hit.sum()))]
    flow.setflags(write=False)
    return flow


# ---- the quality experiment (CPU: the oracle's flows; GPU: engine.video_interpolate) ----------------------------------------------

Q_W, Q_H, Q_LEVELS, Q_WIN = 128, 96, 3, 9
Q_STEPS = [(0.6, -0.3), (1.0, 0.5)]      # motion per frame; the clip's pairs are four frames apart


@functools.lru_cache(maxsize=None)
def quality_clip(step):
    """nine frames of the moving texture: frames 0, 4, 8 are the clip, the others the truth at t = 1/4, 1/2, 3/4"""
    from cuda_optical_flow_2_amd import synth

    return tuple(synth.smooth_pair(Q_W, Q_H, step[0] * i, step[1] * i, seed=41)[1] for i in range(9))


def sad(x, y):
    return int(np.abs(np.asarray(x, np.int64) - np.asarray(y, np.int64)).sum())


def cross_fade(a, b, t):
    """what one has without any flow: (1 - t) a + t b, rounded"""
    return np.clip(np.floor((1.0 - float(t)) * a.astype(np.float64) + float(t) * b.astype(np.float64) + 0.5), 0, 255).astype(np.uint8)
