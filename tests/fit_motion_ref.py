"""NumPy referee of "camera motion from point matches" (include/ofx.h; ofx_fit_motion): restated from the definition, one float64
operation per rounding, every integer expression in int64 or in Python ints (|u| <= 2^20: no product or sum reaches 2^63).
Plain on purpose."""
import numpy as np

TRANSLATION, SIMILARITY, AFFINE = 0, 1, 2
MODELS = {"translation": TRANSLATION, "similarity": SIMILARITY, "affine": AFFINE}
FIT_OK, FIT_FEW, FIT_DEGENERATE = 0, 1, 2
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
M32 = 0xFFFFFFFF
f64 = np.float64


def mix(seed, j, k, a):
    h = (seed ^ (j * 0x9E3779B1) ^ (k * 0x85EBCA77) ^ (a * 0xC2B2AE3D)) & M32
    h ^= h >> 16
    h = (h * 0x7FEB352D) & M32
    h ^= h >> 15
    h = (h * 0x846CA68B) & M32
    h ^= h >> 16
    return h


def sample_index(seed, j, k, a, n):
    return (mix(seed, j, k, a) * n) >> 32


def lattice(p, q, size, status=None, pair=0):
    """(u int64 [n, 2], v int64 [n, 2], usable bool [n]); u and v of an unusable match are 0"""
    w, h = size
    p = np.asarray(p, np.float32).reshape(-1, 2)
    q = np.asarray(q, np.float32).reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(p).all(axis=1) & np.isfinite(q).all(axis=1)
        for t in (p, q):
            ok &= (t[:, 0] >= 0) & (t[:, 0] <= np.float32(w - 1)) & (t[:, 1] >= 0) & (t[:, 1] <= np.float32(h - 1))
    if status is not None:
        s = np.asarray(status, np.int32).reshape(-1)
        ok &= (s == 0) | ((s >> 8) > pair)
    o = np.array([16 * (w - 1), 16 * (h - 1)], np.int64)
    u = np.zeros(p.shape, np.int64)
    v = np.zeros(p.shape, np.int64)
    u[ok] = np.rint(np.ldexp(p[ok], 5)).astype(np.int64) - o
    v[ok] = np.rint(np.ldexp(q[ok], 5)).astype(np.int64) - o
    return u, v, ok


def _translation(m, u0, v0):
    a, b, c, d = m
    tx = f64(v0[0]) - (a * f64(u0[0]) + b * f64(u0[1]))
    ty = f64(v0[1]) - (c * f64(u0[0]) + d * f64(u0[1]))
    return (a, b, tx, c, d, ty)


def hypothesis(model, seed, j, u, v, ok):
    """the six float64 of hypothesis j, or None when it is invalid"""
    n, K = len(ok), model + 1
    idx = []
    for k in range(K):
        for a in range(8):
            i = sample_index(seed, j, k, a, n)
            if ok[i] and i not in idx:
                idx.append(i)
                break
        else:
            return None
    u0, v0 = [int(t) for t in u[idx[0]]], [int(t) for t in v[idx[0]]]
    if model == TRANSLATION:
        return (f64(1.0), f64(0.0), f64(v0[0] - u0[0]), f64(0.0), f64(1.0), f64(v0[1] - u0[1]))
    if model == SIMILARITY:
        dpx, dpy = int(u[idx[1]][0]) - u0[0], int(u[idx[1]][1]) - u0[1]
        dqx, dqy = int(v[idx[1]][0]) - v0[0], int(v[idx[1]][1]) - v0[1]
        den = dpx * dpx + dpy * dpy
        if den == 0:
            return None
        a = f64(dpx * dqx + dpy * dqy) / f64(den)
        b = f64(dpx * dqy - dpy * dqx) / f64(den)
        return _translation((a, -b, b, a), u0, v0)
    d1x, d1y = int(u[idx[1]][0]) - u0[0], int(u[idx[1]][1]) - u0[1]
    d2x, d2y = int(u[idx[2]][0]) - u0[0], int(u[idx[2]][1]) - u0[1]
    e1x, e1y = int(v[idx[1]][0]) - v0[0], int(v[idx[1]][1]) - v0[1]
    e2x, e2y = int(v[idx[2]][0]) - v0[0], int(v[idx[2]][1]) - v0[1]
    det = d1x * d2y - d1y * d2x
    if det == 0:
        return None
    a = f64(e1x * d2y - e2x * d1y) / f64(det)
    b = f64(e2x * d1x - e1x * d2x) / f64(det)
    c = f64(e1y * d2y - e2y * d1y) / f64(det)
    d = f64(e2y * d1x - e1y * d2x) / f64(det)
    return _translation((a, b, c, d), u0, v0)


def inliers(m, u, v, ok, thr_q):
    a, b, tx, c, d, ty = m
    ux, uy, vx, vy = (t.astype(f64) for t in (u[:, 0], u[:, 1], v[:, 0], v[:, 1]))
    rx = (a * ux + b * uy) + (tx - vx)
    ry = (c * ux + d * uy) + (ty - vy)
    e2 = rx * rx + ry * ry
    return ok & (e2 <= f64(thr_q) * f64(thr_q))


def refit(model, m, u, v, inl):
    """(the refitted model, True) or (m, False) when the refit is skipped"""
    ux, uy, vx, vy = (col[inl] for col in (u[:, 0], u[:, 1], v[:, 0], v[:, 1]))     # int64; every sum below is under 2^60: exact
    dot = lambda s, t: f64(int((s * t).sum()))                                      # int64 -> float64 rounds to nearest even
    cnt = len(ux)
    n, Sx, Sy, Vx, Vy = f64(cnt), f64(int(ux.sum())), f64(int(uy.sum())), f64(int(vx.sum())), f64(int(vy.sum()))
    Sxx, Sxy, Syy = dot(ux, ux), dot(ux, uy), dot(uy, uy)
    Sxvx, Syvx, Sxvy, Syvy = dot(ux, vx), dot(uy, vx), dot(ux, vy), dot(uy, vy)
    if model == TRANSLATION:
        if cnt == 0:
            return m, False
        return (f64(1.0), f64(0.0), (Vx - Sx) / n, f64(0.0), f64(1.0), (Vy - Sy) / n), True
    Cxx, Cyy, Cxy = n * Sxx - Sx * Sx, n * Syy - Sy * Sy, n * Sxy - Sx * Sy
    Cxvx, Cyvx, Cxvy, Cyvy = n * Sxvx - Sx * Vx, n * Syvx - Sy * Vx, n * Sxvy - Sx * Vy, n * Syvy - Sy * Vy
    if model == SIMILARITY:
        den = Cxx + Cyy
        if not den > 0:
            return m, False
        a = (Cxvx + Cyvy) / den
        b = (Cxvy - Cyvx) / den
        a, b, c, d = a, -b, b, a
    else:
        D = Cxx * Cyy - Cxy * Cxy
        if not D > 0:
            return m, False
        a = (Cyy * Cxvx - Cxy * Cyvx) / D
        b = (Cxx * Cyvx - Cxy * Cxvx) / D
        c = (Cyy * Cxvy - Cxy * Cyvy) / D
        d = (Cxx * Cyvy - Cxy * Cxvy) / D
    return (a, b, (Vx - (a * Sx + b * Sy)) / n, c, d, (Vy - (c * Sx + d * Sy)) / n), True


def to_pixels(m, size):
    a, b, tx, c, d, ty = m
    ox, oy = f64(16 * (size[0] - 1)), f64(16 * (size[1] - 1))
    return np.array([a, b, ((tx + ox) - (a * ox + b * oy)) / f64(32.0), c, d, ((ty + oy) - (c * ox + d * oy)) / f64(32.0)], f64)


def fit_motion(p, q, size, status=None, pair=0, model=SIMILARITY, hypotheses=256, thr_q=32, refits=2, seed=0):
    """(model float64 [6] in pixels, info int32 [8], inlier uint8 [n]) of one item"""
    model = MODELS.get(model, model)
    u, v, ok = lattice(p, q, size, status, pair)
    n, K = len(ok), model + 1
    info = np.zeros(8, np.int32)
    info[1], info[3] = int(ok.sum()), -1
    mask = np.zeros(n, np.uint8)
    ident = np.array(IDENTITY, f64)
    if info[1] < K:
        info[0] = FIT_FEW
        return ident, info, mask
    best, best_count, valid = None, -1, 0
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(hypotheses):
            m = hypothesis(model, seed, j, u, v, ok)
            if m is None:
                continue
            valid += 1
            count = int(inliers(m, u, v, ok, thr_q).sum())
            if count > best_count:
                best, best_count, info[3] = m, count, j
        info[2] = valid
        if best is None:
            info[0] = FIT_DEGENERATE
            return ident, info, mask
        info[4] = best_count
        m = best
        for _ in range(refits):
            m, done = refit(model, m, u, v, inliers(m, u, v, ok, thr_q))
            info[6] += int(done)
        inl = inliers(m, u, v, ok, thr_q)
        info[5] = int(inl.sum())
        return to_pixels(m, size), info, inl.astype(np.uint8)


def compose(m2, m1):
    """m2 after m1: products, then sums left to right"""
    a2, b2, tx2, c2, d2, ty2 = (f64(t) for t in m2)
    a1, b1, tx1, c1, d1, ty1 = (f64(t) for t in m1)
    with np.errstate(all="ignore"):
        return np.array([a2 * a1 + b2 * c1, a2 * b1 + b2 * d1, (a2 * tx1 + b2 * ty1) + tx2,
                         c2 * a1 + d2 * c1, c2 * b1 + d2 * d1, (c2 * tx1 + d2 * ty1) + ty2], f64)


def invert(m):
    """the inverse map, or None when det = a d - b c is 0 or not finite"""
    a, b, tx, c, d, ty = (f64(t) for t in m)
    with np.errstate(all="ignore"):
        det = a * d - b * c
        if det == 0 or not np.isfinite(det):
            return None
        ia, ib, ic, id_ = d / det, -b / det, -c / det, a / det
        return np.array([ia, ib, -(ia * tx + ib * ty), ic, id_, -(ic * tx + id_ * ty)], f64)
