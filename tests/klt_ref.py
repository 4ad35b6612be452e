"""The definition "sparse Lucas-Kanade tracking" of include/ofx.h in NumPy: int64 up to the 2x2 solve, float64 after it (NumPy
rounds every operation once and fuses nothing), vectorised over the points.  No GPU, no library: tests/test_klt_ref.py checks this
file against the definition in words, tests/test_gpu_klt.py checks the kernel against this file by the bits."""
from collections import namedtuple

import numpy as np

START, SINGULAR, OUT, RESIDUAL, FB = 1, 2, 3, 4, 5
Params = namedtuple("Params", "window max_iters eps_q min_lambda max_sad", defaults=(10, 1, 0.0, 0))


def sample(P, qx, qy):
    """SAMPLE: S(P, qx, qy) for int64 lattice positions of any shape; P a u8 plane [h, w]"""
    h, w = P.shape
    qx, qy = np.asarray(qx, np.int64), np.asarray(qy, np.int64)
    ix, a, iy, b = qx >> 5, qx & 31, qy >> 5, qy & 31
    x0, x1 = np.clip(ix, 0, w - 1), np.clip(ix + 1, 0, w - 1)
    y0, y1 = np.clip(iy, 0, h - 1), np.clip(iy + 1, 0, h - 1)
    Q = P.astype(np.int64)
    s = (32 - a) * (32 - b) * Q[y0, x0] + a * (32 - b) * Q[y0, x1] + (32 - a) * b * Q[y1, x0] + a * b * Q[y1, x1]
    return (s + 16) >> 5


def lam_of(gxx, gyy, gxy):
    """step 2 of TEXTURE STRENGTH on float64 arrays"""
    tr, d = gxx + gyy, gxx - gyy
    q = d * d
    p2 = gxy * gxy
    p4 = 4.0 * p2
    r = q + p4
    return 0.5 * (tr - np.sqrt(r))


def lattice(x, k):
    """lrintf(ldexpf(x, 5 - k)) of float32 values"""
    return np.rint(np.ldexp(np.asarray(x, np.float32), 5 - k)).astype(np.int64)


def track_pair(A, B, points, status, pair, prm):
    """One pair.  A, B: lists of u8 planes, level 0 first.  points float32 [n, 2], status int32 [n].  Returns (points, status, sad
    int32 [n], stats int64 [7]); the inputs are left as they are."""
    prm = Params(*prm)
    levels, (h, w) = len(A), A[0].shape
    R = prm.window >> 1
    n = len(points)
    points, status = np.array(points, np.float32), np.array(status, np.int32)
    sad = np.full(n, -1, np.int32)
    stats = np.zeros(7, np.int64)
    off = np.arange(-R, R + 1, dtype=np.int64) * 32
    oi, oj = off[None, None, :], off[None, :, None]                 # [1, 1, W] across, [1, W, 1] down
    x, y = points[:, 0], points[:, 1]
    with np.errstate(invalid="ignore"):
        ok = (x >= 0) & (x <= np.float32(w - 1)) & (y >= 0) & (y <= np.float32(h - 1))
    live = status == 0
    reason = np.zeros(n, np.int64)
    reason[live & ~ok] = START
    idx = np.flatnonzero(live & ok)                                 # the points still on their way
    d = np.zeros((len(idx), 2), np.int64)
    c = np.zeros((len(idx), 2), np.int64)
    I = None
    for k in range(levels - 1, -1, -1):
        if k != levels - 1:
            d *= 2
        Ak, Bk = A[k], B[k]
        assert Ak.shape == (h >> k, w >> k) == Bk.shape
        c = np.stack([lattice(x[idx], k), lattice(y[idx], k)], axis=1)
        px, py = c[:, 0, None, None] + oi, c[:, 1, None, None] + oj  # [m, W, W]
        I = sample(Ak, px, py)
        gx = sample(Ak, px + 32, py) - sample(Ak, px - 32, py)
        gy = sample(Ak, px, py + 32) - sample(Ak, px, py - 32)
        Gxx, Gyy, Gxy = ((gx * gx).sum((1, 2)), (gy * gy).sum((1, 2)), (gx * gy).sum((1, 2)))
        fxx, fyy, fxy = Gxx.astype(np.float64), Gyy.astype(np.float64), Gxy.astype(np.float64)
        D = fxx * fyy - fxy * fxy
        lam = lam_of(fxx, fyy, fxy)
        sing = ~(D > 0) | ~(lam > np.float64(np.float32(prm.min_lambda)))
        run = np.flatnonzero(~sing)                                 # rows of idx that iterate at this level
        for _ in range(prm.max_iters):
            if len(run) == 0:
                break
            q = c[run] + d[run]
            e = sample(Bk, q[:, 0, None, None] + oi, q[:, 1, None, None] + oj) - I[run]
            bx, by = (gx[run] * e).sum((1, 2)).astype(np.float64), (gy[run] * e).sum((1, 2)).astype(np.float64)
            sx = -64.0 * ((fyy[run] * bx - fxy[run] * by) / D[run])
            sy = -64.0 * ((fxx[run] * by - fxy[run] * bx) / D[run])
            tx = np.clip(np.rint(sx), -2048, 2048).astype(np.int64)
            ty = np.clip(np.rint(sy), -2048, 2048).astype(np.int64)
            d[run, 0] += tx
            d[run, 1] += ty
            stats[5] += len(run)
            run = run[~((np.abs(tx) <= prm.eps_q) & (np.abs(ty) <= prm.eps_q))]
        if k == 0:
            reason[idx[sing]] = SINGULAR
            keep = ~sing
            idx, d, c, I = idx[keep], d[keep], c[keep], I[keep]
    q = c + d
    out = (q[:, 0] < 0) | (q[:, 0] > 32 * (w - 1)) | (q[:, 1] < 0) | (q[:, 1] > 32 * (h - 1))
    reason[idx[out]] = OUT
    idx, q, I = idx[~out], q[~out], I[~out]
    s = np.abs(sample(B[0], q[:, 0, None, None] + oi, q[:, 1, None, None] + oj) - I).sum((1, 2))
    bad = (s > prm.max_sad) if prm.max_sad > 0 else np.zeros(len(idx), bool)
    reason[idx[bad]] = RESIDUAL
    idx, q, s = idx[~bad], q[~bad], s[~bad]
    points[idx] = q.astype(np.float32) / np.float32(32)
    sad[idx] = s
    lost = reason != 0
    status[lost] = (pair << 8) | reason[lost]
    stats[0] = int((status == 0).sum())
    for r in (START, SINGULAR, OUT, RESIDUAL):
        stats[r] = int((reason == r).sum())
    stats[6] = int(s.sum())
    return points, status, sad, stats


def track_chain(pyramids, points, status, pair0, prm):
    """CHAIN over len(pyramids) - 1 pairs.  Returns (points, status, history float32 [pairs, n, 2], sad int32 [pairs, n], stats int64
    [pairs, 7])."""
    hist, sads, stats = [], [], []
    points, status = np.array(points, np.float32), np.array(status, np.int32)
    for b in range(len(pyramids) - 1):
        points, status, s, st = track_pair(pyramids[b], pyramids[b + 1], points, status, pair0 + b, prm)
        hist.append(points.copy()), sads.append(s), stats.append(st)
    return points, status, np.stack(hist), np.stack(sads), np.stack(stats)


def forward_backward(A, B, points, status, sad, start, fb_max, pair, prm):
    """engine.track_points' fb_max: the tracked points go back B -> A; where the round trip is lost or misses the start by more
    than fb_max px in either coordinate (on the lattice: more than floor(32 fb_max) units), the point is lost with reason FB: it
    keeps its start, and its sad is -1."""
    back, bstat, _, _ = track_pair(B, A, points, status, pair, prm)
    lim = int(np.floor(32.0 * fb_max))
    live = status == 0                                              # (the others may hold anything, a NaN among it)
    q0, q1 = (np.rint(np.where(live[:, None], v, 0) * np.float32(32)).astype(np.int64) for v in (np.asarray(start, np.float32), back))
    miss = live & ((bstat != 0) | (np.abs(q1 - q0) > lim).any(axis=1))
    points, status, sad = points.copy(), status.copy(), sad.copy()
    points[miss] = np.asarray(start, np.float32)[miss]
    status[miss] = (pair << 8) | FB
    sad[miss] = -1
    return points, status, sad


# ---- planes ---------------------------------------------------------------------------------------------------------------------
def pyramid(img, levels):
    """a pyramid for the referee's own tests and the kernel's, of any size: level k + 1 (x, y) = the (1 2 1) x (1 2 1) / 16 mean
    around (2x, 2y) of level k, rounded, the border replicated.  (The tracker does not care how its planes were made; the engine's
    calls use ofx_pyramid_1ch.)"""
    out = [np.ascontiguousarray(img, np.uint8)]
    for _ in range(1, levels):
        h, w = out[-1].shape[0] // 2, out[-1].shape[1] // 2
        assert h >= 1 and w >= 1
        p = np.pad(out[-1].astype(np.int32), 1, mode="edge")
        s = p[:, :-2] + 2 * p[:, 1:-1] + p[:, 2:]
        s = s[:-2] + 2 * s[1:-1] + s[2:]
        out.append(((s[0:2 * h:2, 0:2 * w:2] + 8) >> 4).astype(np.uint8))
    return out


_COS = None


def cosine_texture(w, h, sx=0.0, sy=0.0, seed=17, terms=40, fmax=0.6):
    """a sum of `terms` cosines with spatial frequencies within +-fmax rad/px, rounded to u8, seen from (sx, sy): the content at
    (x, y) of the unshifted image is at (x + sx, y + sy) here"""
    rng = np.random.RandomState(seed)
    fx, fy = rng.uniform(-fmax, fmax, terms), rng.uniform(-fmax, fmax, terms)
    ph, amp = rng.uniform(0, 2 * np.pi, terms), rng.uniform(0.5, 1.0, terms)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    xx, yy = xx - sx, yy - sy
    img = sum(a * np.cos(u * xx + v * yy + p) for a, u, v, p in zip(amp, fx, fy, ph))
    img = 127.5 + img * (40.0 / np.sqrt(0.5 * (amp * amp).sum()))   # (40 grey levels per standard deviation, whatever the shift)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def interior_points(w, h, nx, ny, margin):
    xs, ys = np.linspace(margin, w - 1 - margin, nx), np.linspace(margin, h - 1 - margin, ny)
    return np.stack(np.meshgrid(np.rint(xs), np.rint(ys)), axis=-1).reshape(-1, 2).astype(np.float32)
