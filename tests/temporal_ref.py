"""NumPy referee of "temporal noise filter" (include/ofx.h; ofx_temporal_filter), restated from the definition: positions, the nine
patch values each at its own clamped position through VALUE of "affine frame warp", the patch test, the weighted mean and the
stats.  It shares no code with the engine; engine.temporal_weights is restated here too."""
import numpy as np

MAX_NEIGHBOURS = 4
MAX_DISP = np.float32(1048576.0)


def weights_for(sigma):
    """uint16 [256]: rint(256 exp(-t^2 / (2 (0.75 sigma)^2))), t = max(0, i - 1.5 sigma), in float64"""
    out = np.zeros(256, np.uint16)
    for i in range(256):
        t = max(0.0, i - 1.5 * float(sigma))
        out[i] = int(np.rint(256.0 * np.exp(-(t * t) / (2.0 * (0.75 * float(sigma)) ** 2))))
    return out


def positions(field, w, h):
    """(qx, qy int64 [h, w], defined, usable bool [h, w]) of POSITION; qx = qy = 0 where not defined"""
    f = np.asarray(field, np.float32).reshape(h, w, 2)
    u, v = f[..., 0], f[..., 1]
    with np.errstate(invalid="ignore"):
        defined = np.isfinite(u) & np.isfinite(v) & (np.abs(u) <= MAX_DISP) & (np.abs(v) <= MAX_DISP)
    su = (np.float32(32.0) * np.where(defined, u, np.float32(0.0))).astype(np.float32)
    sv = (np.float32(32.0) * np.where(defined, v, np.float32(0.0))).astype(np.float32)
    x = np.arange(w, dtype=np.int64)[None, :]
    y = np.arange(h, dtype=np.int64)[:, None]
    qx = np.where(defined, 32 * x + np.rint(su).astype(np.int64), 0)
    qy = np.where(defined, 32 * y + np.rint(sv).astype(np.int64), 0)
    usable = defined & (qx >= 0) & (qx <= 32 * (w - 1)) & (qy >= 0) & (qy <= 32 * (h - 1))
    return qx, qy, defined, usable


def value_at(plane, qx, qy):
    """VALUE of "affine frame warp" of plane [h, w, C] at positions in 0 .. 32 (size - 1): int64 [.., C]"""
    h, w = plane.shape[:2]
    p = plane.astype(np.int64)
    ix, fa, iy, fb = qx >> 5, qx & 31, qy >> 5, qy & 31
    ix1, iy1 = np.minimum(ix + 1, w - 1), np.minimum(iy + 1, h - 1)
    fa, fb = fa[..., None], fb[..., None]
    s = (32 - fa) * (32 - fb) * p[iy, ix] + fa * (32 - fb) * p[iy, ix1] + (32 - fa) * fb * p[iy1, ix] + fa * fb * p[iy1, ix1]
    return (s + 512) >> 10


def _planes3(a):
    a = np.asarray(a, np.uint8)
    return a if a.ndim == 3 else a[:, :, None]


def patch_test(centre, plane, field):
    """(m int64 [h, w]: the rounded mean absolute patch difference, clipped to 255; N0 int64 [h, w, C]: N_k(0, 0); usable; interior:
    where the 4 x 4 block of taps lies inside the plane) of one neighbour.  Positions that are not usable are evaluated at (0, 0)."""
    c, n = _planes3(centre), _planes3(plane)
    h, w, C = c.shape
    qx, qy, _, usable = positions(field, w, h)
    qx, qy = np.where(usable, qx, 0), np.where(usable, qy, 0)
    x = np.arange(w)[None, :]
    y = np.arange(h)[:, None]
    sad = np.zeros((h, w), np.int64)
    for j in (-1, 0, 1):
        for i in (-1, 0, 1):
            N = value_at(n, np.clip(qx + 32 * i, 0, 32 * (w - 1)), np.clip(qy + 32 * j, 0, 32 * (h - 1)))
            cc = c[np.clip(y + j, 0, h - 1), np.clip(x + i, 0, w - 1)].astype(np.int64)
            sad += np.abs(N - cc).sum(axis=2)
            if i == 0 and j == 0:
                N0 = N
    m = np.minimum(255, (sad + 4) // 9 if C == 1 else (sad + 13) // 27)
    ix, iy = qx >> 5, qy >> 5
    interior = (ix >= 1) & (ix + 2 <= w - 1) & (iy >= 1) & (iy + 2 <= h - 1)
    return m, N0, usable, interior


def temporal_filter(centre, planes, fields, weights, centre_weight=256):
    """(out uint8 like centre, stats int64 [8])"""
    weights = np.asarray(weights).astype(np.int64)
    assert weights.shape == (256,) and weights.min() >= 0 and weights.max() <= 256 and 1 <= centre_weight <= 256
    assert 1 <= len(planes) <= MAX_NEIGHBOURS and len(fields) == len(planes)
    c = _planes3(centre).astype(np.int64)
    h, w, C = c.shape
    num = centre_weight * c
    den = np.full((h, w), centre_weight, np.int64)
    stats = np.zeros(8, np.int64)
    stats[0] = w * h
    for k, (plane, field) in enumerate(zip(planes, fields)):
        m, N0, usable, _ = patch_test(centre, plane, field)
        wk = np.where(usable, weights[m], 0)
        num = num + wk[:, :, None] * N0
        den = den + wk
        stats[1 + k] = int((~usable).sum())
    out = (2 * num + den[:, :, None]) // (2 * den[:, :, None])
    assert out.min() >= 0 and out.max() <= 255
    stats[5] = int((den == centre_weight).sum())
    stats[6] = int(np.abs(out - c).sum())
    stats[7] = int((den - centre_weight).sum())
    return out.astype(np.uint8).reshape(np.asarray(centre).shape), stats


def denoise_rings(frames, fwd, bwd, weights, centre_weight=256):
    """[(out, stats)] per frame of engine._denoise_rings: frame f with frame f-1 through bwd[N-1-f], then frame f+1 through fwd[f]"""
    frames = np.asarray(frames)
    N = len(frames)
    res = []
    for f in range(N):
        near = ([(frames[f - 1], bwd[N - 1 - f])] if f >= 1 else []) + ([(frames[f + 1], fwd[f])] if f + 1 < N else [])
        res.append(temporal_filter(frames[f], [p for p, _ in near], [d for _, d in near], weights, centre_weight))
    return res
