"""Referee of "planar homography from point matches" (include/ofx.h; ofx_fit_homography) and of the host helpers on float64 [9]
models: restated from the definition -- Python ints for the sums, float(int) for their conversion (to nearest even, in one
rounding), NumPy float64 scalars, one operation per rounding, for the rest.  Plain on purpose."""
import numpy as np

from fit_motion_ref import FIT_DEGENERATE, FIT_FEW, FIT_OK, lattice, sample_index

HOMOGRAPHY = 3
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
f64 = np.float64
ONE, ZERO = f64(1.0), f64(0.0)


def scale_exponent(size):
    big, e = max(16 * (size[0] - 1), 16 * (size[1] - 1), 1), 0
    while (1 << e) < big:
        e += 1
    return e


def solve(M):
    """SOLVE of an 8 x 9 list of lists of float64 (changed in place): [h0 .. h7], or None when INVALID"""
    with np.errstate(all="ignore"):
        for c in range(8):
            p = c
            for r in range(c + 1, 8):
                if abs(M[r][c]) > abs(M[p][c]):
                    p = r
            if M[p][c] == 0 or not np.isfinite(M[p][c]):
                return None
            M[p], M[c] = M[c], M[p]
            for r in range(c + 1, 8):
                f = M[r][c] / M[c][c]
                for k in range(c + 1, 9):
                    M[r][k] = M[r][k] - f * M[c][k]
        h = [None] * 8
        for c in range(7, -1, -1):
            s = M[c][8]
            for k in range(c + 1, 8):
                s = s - M[c][k] * h[k]
            h[c] = s / M[c][c]
        return h if all(np.isfinite(v) for v in h) else None


def normalised(t, e):
    return f64(np.ldexp(f64(int(t)), -e))


def sample(seed, j, ok):
    """SAMPLER with K = 4: the four match indices of hypothesis j, or None when a sample finds no match in eight attempts"""
    n, idx = len(ok), []
    for k in range(4):
        for a in range(8):
            i = sample_index(seed, j, k, a, n)
            if ok[i] and i not in idx:
                idx.append(i)
                break
        else:
            return None
    return idx


def system(pts):
    """the 8 x 9 system of four normalised samples (x, y, X, Y)"""
    M = []
    for x, y, X, Y in pts:
        M.append([x, y, ONE, ZERO, ZERO, ZERO, -(x * X), -(y * X), X])
        M.append([ZERO, ZERO, ZERO, x, y, ONE, -(x * Y), -(y * Y), Y])
    return M


def hypothesis(seed, j, u, v, ok, e):
    """[h0 .. h7] of hypothesis j, or None when it is invalid"""
    idx = sample(seed, j, ok)
    if idx is None:
        return None
    pts = [tuple(normalised(t, e) for t in (u[i][0], u[i][1], v[i][0], v[i][1])) for i in idx]
    h = solve(system(pts))
    if h is None:
        return None
    for x, y, _, _ in pts:
        if not (h[6] * x + h[7] * y) + ONE > 0:
            return None
    return h


def inliers(h, u, v, ok, thr_q, e):
    with np.errstate(all="ignore"):
        x, y, X, Y = (np.ldexp(t.astype(f64), -e) for t in (u[:, 0], u[:, 1], v[:, 0], v[:, 1]))
        W = (h[6] * x + h[7] * y) + ONE
        rx = ((h[0] * x + h[1] * y) + h[2]) - X * W
        ry = ((h[3] * x + h[4] * y) + h[5]) - Y * W
        tw = f64(np.ldexp(f64(thr_q), -e)) * W
        return ok & (W > 0) & (rx * rx + ry * ry <= tw * tw)


def sums(u, v, inl):
    """the 23 exact sums over the inliers, Python ints, by name"""
    s = dict.fromkeys("m Sx Sy SX SY Sxx Sxy Syy SxX SyX SxY SyY SxxX SxyX SyyX SxxY SxyY SyyY SxR SyR SxxR SxyR SyyR".split(), 0)
    for i in np.flatnonzero(inl):
        x, y, X, Y = int(u[i][0]), int(u[i][1]), int(v[i][0]), int(v[i][1])
        R = X * X + Y * Y
        for name, t in (("m", 1), ("Sx", x), ("Sy", y), ("SX", X), ("SY", Y), ("Sxx", x * x), ("Sxy", x * y), ("Syy", y * y), ("SxX", x * X),
                        ("SyX", y * X), ("SxY", x * Y), ("SyY", y * Y), ("SxxX", x * x * X), ("SxyX", x * y * X), ("SyyX", y * y * X),
                        ("SxxY", x * x * Y), ("SxyY", x * y * Y), ("SyyY", y * y * Y), ("SxR", x * R), ("SyR", y * R), ("SxxR", x * x * R),
                        ("SxyR", x * y * R), ("SyyR", y * y * R)):
            s[name] += t
    return s


DEGREE = dict(m=0, Sx=1, Sy=1, SX=1, SY=1, Sxx=2, Sxy=2, Syy=2, SxX=2, SyX=2, SxY=2, SyY=2, SxxX=3, SxyX=3, SyyX=3, SxxY=3, SxyY=3, SyyY=3,
              SxR=3, SyR=3, SxxR=4, SxyR=4, SyyR=4)


def refit(h, u, v, inl, e):
    """(the refitted [h0 .. h7], True) or (h, False) when the refit is skipped"""
    s = sums(u, v, inl)
    if s["m"] < 4:
        return h, False
    S = {k: f64(np.ldexp(f64(float(t)), -DEGREE[k] * e)) for k, t in s.items()}       # float(int): to nearest even, once
    g = lambda k: S[k]
    M = [[g("Sxx"), g("Sxy"), g("Sx"), ZERO, ZERO, ZERO, -g("SxxX"), -g("SxyX"), g("SxX")],
         [g("Sxy"), g("Syy"), g("Sy"), ZERO, ZERO, ZERO, -g("SxyX"), -g("SyyX"), g("SyX")],
         [g("Sx"), g("Sy"), g("m"), ZERO, ZERO, ZERO, -g("SxX"), -g("SyX"), g("SX")],
         [ZERO, ZERO, ZERO, g("Sxx"), g("Sxy"), g("Sx"), -g("SxxY"), -g("SxyY"), g("SxY")],
         [ZERO, ZERO, ZERO, g("Sxy"), g("Syy"), g("Sy"), -g("SxyY"), -g("SyyY"), g("SyY")],
         [ZERO, ZERO, ZERO, g("Sx"), g("Sy"), g("m"), -g("SxY"), -g("SyY"), g("SY")],
         [-g("SxxX"), -g("SxyX"), -g("SxX"), -g("SxxY"), -g("SxyY"), -g("SxY"), g("SxxR"), g("SxyR"), -g("SxR")],
         [-g("SxyX"), -g("SyyX"), -g("SyX"), -g("SxyY"), -g("SyyY"), -g("SyY"), g("SxyR"), g("SyyR"), -g("SyR")]]
    new = solve(M)
    return (h, False) if new is None else (new, True)


def to_pixels(h, size, e):
    """float64 [9] in pixels, or None when its entry 8 would be 0 or not finite"""
    h = list(h) + [ONE]
    s, cx, cy = f64(np.ldexp(1.0, 5 - e)), f64(np.ldexp(f64(16 * (size[0] - 1)), -e)), f64(np.ldexp(f64(16 * (size[1] - 1)), -e))
    with np.errstate(all="ignore"):
        A = [[h[3 * i] * s, h[3 * i + 1] * s, h[3 * i + 2] - (h[3 * i] * cx + h[3 * i + 1] * cy)] for i in range(3)]
        B = [[A[0][j] + cx * A[2][j] for j in range(3)], [A[1][j] + cy * A[2][j] for j in range(3)], [s * A[2][j] for j in range(3)]]
        d = B[2][2]
        if d == 0 or not np.isfinite(d):
            return None
        return np.array([B[i][j] / d for i in range(3) for j in range(3)], f64)


def fit_homography(p, q, size, status=None, pair=0, hypotheses=256, thr_q=32, refits=2, seed=0):
    """(model float64 [9] in pixels, info int32 [8], inlier uint8 [n]) of one item"""
    u, v, ok = lattice(p, q, size, status, pair)
    n, e = len(ok), scale_exponent(size)
    info = np.zeros(8, np.int32)
    info[1], info[3] = int(ok.sum()), -1
    mask = np.zeros(n, np.uint8)
    ident = np.array(IDENTITY, f64)
    if info[1] < 4:
        info[0] = FIT_FEW
        return ident, info, mask
    best, best_count, best_j, valid = None, -1, -1, 0
    for j in range(hypotheses):
        h = hypothesis(seed, j, u, v, ok, e)
        if h is None:
            continue
        valid += 1
        count = int(inliers(h, u, v, ok, thr_q, e).sum())
        if count > best_count:
            best, best_count, best_j = h, count, j
    info[2] = valid
    if best is None:
        info[0] = FIT_DEGENERATE
        return ident, info, mask
    h, done = best, 0
    for _ in range(refits):
        h, did = refit(h, u, v, inliers(h, u, v, ok, thr_q, e), e)
        done += int(did)
    model = to_pixels(h, size, e)
    if model is None:
        info[0] = FIT_DEGENERATE
        return ident, info, mask
    inl = inliers(h, u, v, ok, thr_q, e)
    info[3], info[4], info[5], info[6] = best_j, best_count, int(inl.sum()), done
    return model, info, inl.astype(np.uint8)


# ---- the host helpers ----------------------------------------------------------------------------------------------------------------

def compose(m2, m1):
    """m2 after m1, the 3 x 3 product: products, then sums left to right; not renormalised"""
    a, b = [f64(t) for t in np.asarray(m2, f64).reshape(9)], [f64(t) for t in np.asarray(m1, f64).reshape(9)]
    with np.errstate(all="ignore"):
        return np.array([(a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j] for i in range(3) for j in range(3)], f64)


def invert(m):
    """the adjugate divided by the determinant, or None when the determinant is 0 or not finite"""
    m = [f64(t) for t in np.asarray(m, f64).reshape(9)]
    with np.errstate(all="ignore"):
        c0, c1, c2 = m[4] * m[8] - m[5] * m[7], m[5] * m[6] - m[3] * m[8], m[3] * m[7] - m[4] * m[6]
        det = (m[0] * c0 + m[1] * c1) + m[2] * c2
        if det == 0 or not np.isfinite(det):
            return None
        adj = [c0, m[2] * m[7] - m[1] * m[8], m[1] * m[5] - m[2] * m[4], c1, m[0] * m[8] - m[2] * m[6], m[2] * m[3] - m[0] * m[5],
               c2, m[1] * m[6] - m[0] * m[7], m[0] * m[4] - m[1] * m[3]]
        return np.array([t / det for t in adj], f64)


def normalize(m):
    """m / m[8], or None when m[8] is 0 or not finite"""
    m = np.asarray(m, f64).reshape(9)
    if m[8] == 0 or not np.isfinite(m[8]):
        return None
    with np.errstate(all="ignore"):
        return np.array([t / m[8] for t in m], f64)


def from_affine(m6):
    a, b, tx, c, d, ty = (f64(t) for t in np.asarray(m6, f64).reshape(6))
    return np.array([a, b, tx, c, d, ty, 0.0, 0.0, 1.0], f64)


def smooth_path(models, radius):
    """row f: the mean of the normalised rows max(f - radius, 0) .. min(f + radius, N - 1), summed in index order, divided once"""
    m = np.stack([normalize(r) for r in np.asarray(models, f64).reshape(-1, 9)])
    N, out = m.shape[0], np.empty((m.shape[0], 9), f64)
    for f in range(N):
        g0, g1 = max(f - radius, 0), min(f + radius, N - 1)
        for e in range(9):
            s = f64(0.0)
            for g in range(g0, g1 + 1):
                s = s + m[g, e]
            out[f, e] = s / f64(g1 - g0 + 1)
    return out


def apply(m, pts):
    """the images of points float [n, 2] under a [9] model (plain float64; for building test data, not part of the definition)"""
    m, pts = np.asarray(m, f64).reshape(3, 3), np.asarray(pts, f64).reshape(-1, 2)
    t = np.concatenate([pts, np.ones((len(pts), 1))], axis=1) @ m.T
    return t[:, :2] / t[:, 2:3]
