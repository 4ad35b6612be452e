"""The definition "sparse Lucas-Kanade tracking" of include/ofx.h in NumPy: int64 up to the 2x2 solve, float64 after it (NumPy
rounds every operation once and fuses nothing), vectorised over the points.  No GPU, no library: tests/test_klt_ref.py checks this
file against the definition in words, tests/test_gpu_klt.py checks the kernel against this file by the bits.  The inputs that the
two share are at the end."""
import functools
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


# ---- the inputs that tests/test_klt_ref.py (the conditions on them, by the referee alone) and tests/test_gpu_klt.py (the kernel
# ---- against the referee) share, made once ------------------------------------------------------------------------------------------
NAN, INF = np.float32("nan"), np.float32("inf")
ALL_WINDOWS = tuple(range(3, 24, 2))                              # one instance of klt_kernel<R> each
HARD_SHAPE = (67, 45, 4)                                          # (w, h, levels): where every window runs


def _shift(img, sx, sy):
    """the content of img at (x, y) at (x + sx, y + sy), the border replicated"""
    h, w = img.shape
    yy, xx = np.clip(np.arange(h) - sy, 0, h - 1), np.clip(np.arange(w) - sx, 0, w - 1)
    return np.ascontiguousarray(img[yy][:, xx])


def _frozen(planes):
    for p in planes:
        p.setflags(write=False)
    return tuple(planes)


@functools.lru_cache(maxsize=None)
def hard_pyramids(w, h, levels):
    """the hard frame of tests/iter_hard.py (flat blocks, stripes, noise; below 33 x 17 plain noise) against a copy shifted by
    (2, -1), noise of +-2 grey levels added to it"""
    import iter_hard

    rng = np.random.RandomState(w * 131 + h)
    a = iter_hard.hard_frames(w, h, 1, block=(max(h // 4, 1), max(w // 4, 1)), band=max(w // 8, 1))[0] if w >= 33 else rng.randint(0, 256, (h, w)).astype(np.uint8)
    b = np.clip(_shift(a, 2, -1).astype(np.int32) + rng.randint(-2, 3, (h, w)), 0, 255).astype(np.uint8)
    return _frozen(pyramid(a, levels)), _frozen(pyramid(b, levels))


@functools.lru_cache(maxsize=None)
def smooth_pyramid(w, h, levels, sx, sy):
    return _frozen(pyramid(cosine_texture(w, h, sx, sy), levels))


def specials(w, h):
    """positions that a tracker gets wrong first: the four corners, edge points, points whose window hangs over a border, ties of
    the lattice, NaN, infinities, negative positions and positions past the last pixel"""
    X, Y = np.float32(w - 1), np.float32(h - 1)
    return [(0, 0), (X, 0), (0, Y), (X, Y), (X / 2, 0), (0, Y / 2), (X, Y / 2), (X / 2, Y), (1.546875, 1.515625), (X - 1.546875, Y - 0.515625),
            (NAN, 1), (1, NAN), (INF, 0), (0, -INF), (-0.03125, 0), (0, -1e-30), (X + 0.03125, 0), (0, Y + 1), (-1e30, 1e30), (X - 0.5, Y - 0.25),
            (0.015625, 0.046875), (2.5, 3.5), (X - 2, Y / 3), (X - 1, Y / 2), (X / 3, 1), (0.5, 0.5), (1e-40, 0), (-0.0, -0.0)]


def points_for(w, h, n, seed=0):
    """(points float32 [n, 2], status int32 [n]): specials(w, h), three points frozen on entry, and random ones on and off the
    lattice.  n == 1: a random point."""
    rng = np.random.RandomState(seed + 7 * n)
    special = specials(w, h)
    pts = np.zeros((n, 2), np.float32)
    q = np.stack([rng.randint(0, 32 * (w - 1) + 1, n), rng.randint(0, 32 * (h - 1) + 1, n)], axis=1).astype(np.float32) / np.float32(32)
    r = (rng.rand(n, 2) * [w - 1, h - 1]).astype(np.float32)
    pts[:] = np.where((np.arange(n) & 1)[:, None] == 0, q, r)
    status = np.zeros(n, np.int32)
    if n > 1:
        k = min(len(special), n - 1)
        with np.errstate(invalid="ignore"):
            pts[1:1 + k] = np.float32(special[:k])
        for i, st in ((n - 1, (3 << 8) | OUT), (n // 2, 1), (n // 3, -5)):
            status[i] = st
    return pts, status


def lam_for(win):
    """a min_lambda between the flat / striped / weak windows and the textured ones of the test frames"""
    return float(np.float32(2.0e5 * win * win))


def combos(windows):
    """(window, max_iters, eps_q, min_lambda, max_sad, n_points): every window with every n_points; the other parameters take
    both of their values at every window"""
    out = []
    for win in windows:
        for j, n in enumerate((1, 63, 65, 257)):
            out.append(Params(win, (1, 32, 32, 4)[j], (0, 1, 0, 1)[j], (0.0, lam_for(win), 0.0, lam_for(win))[j], (0, 0, 60 * win * win, 200 * win * win)[j]) + (n,))
    return out


_WANT = {}


def want_chain(key, pyramids, pts, status, pair0, prm):
    """the referee's chain, computed once per key and shared"""
    if key not in _WANT:
        _WANT[key] = track_chain(pyramids, pts, status, pair0, prm)
        for a in _WANT[key]:
            a.setflags(write=False)
    return _WANT[key]


def reasons_of(want, status):
    """[tracked, START, SINGULAR, OUT, RESIDUAL, FB] counts of a chain's final status, of the points alive on entry"""
    return np.bincount(want[1][status == 0] & 255, minlength=6)[:6]


def hard_case(c):
    """one of combos()'s cases on the hard frame at HARD_SHAPE: (pyramids, points, status, pair0, Params, the referee's chain)"""
    w, h, levels = HARD_SHAPE
    pa, pb = hard_pyramids(w, h, levels)
    prm, n = Params(*c[:5]), c[5]
    pts, status = points_for(w, h, n, seed=w)
    return [pa, pb], pts, status, 3, prm, want_chain(("hard", w, h, levels, tuple(c)), [pa, pb], pts, status, 3, prm)


# more points than the launch has waves: csrc/klt.hip launches at most 8192 blocks of four waves
TURN_FIRST = 4 * 8192                                             # the first point that a wave takes on its second visit
TURN_N = TURN_FIRST + 261
TURN_WINDOWS = (3, 5)
TURN_PAIR0 = 300


@functools.lru_cache(maxsize=None)
def turn_case(window):
    """(pyramids, points, status, pair0, Params, the referee's chain): TURN_N points on three frames of the texture drifting by
    (0.7, -0.4) px per frame.  points_for's points, and its specials and frozen points once more from TURN_FIRST + 3 on; five more
    of the last 261 points come with a status."""
    w, h, levels = HARD_SHAPE
    pyr = [smooth_pyramid(w, h, levels, 0.7 * i, -0.4 * i) for i in range(3)]
    pts, status = points_for(w, h, TURN_N, seed=11)
    sp = specials(w, h)
    with np.errstate(invalid="ignore"):
        pts[TURN_FIRST + 3:TURN_FIRST + 3 + len(sp)] = np.float32(sp)
    for i, st in ((TURN_FIRST, (2 << 8) | SINGULAR), (TURN_FIRST + 64, 1), (TURN_FIRST + 129, -5), (TURN_FIRST + 255, (299 << 8) | RESIDUAL), (TURN_N - 2, 7)):
        status[i] = st
    pts.setflags(write=False), status.setflags(write=False)
    prm = Params(window, 4, 1, 0.0, 60 * window * window)
    return pyr, pts, status, TURN_PAIR0, prm, want_chain(("turn", window), pyr, pts, status, TURN_PAIR0, prm)


# 6, 7 and 8 levels: OFX_TRACK_MAX_LEVELS is 8; the coarsest levels are 6 x 2, 4 x 2, 2 x 1 and 1 x 1 pixels
DEEP_SHAPES = [(200, 70, 6), (262, 137, 7), (259, 131, 8), (131, 129, 8)]
DEEP_SHIFTS = ((0.4, -0.3), (-2.75, 1.5), (9.0, 5.0))
DEEP_WINDOWS = (7, 15)


def deep_cases(w, h, levels):
    """[(name, pyramids, points, status, pair0, Params, padded pitches, the referee's chain)]: every shift x window x min_lambda off
    and on"""
    out = []
    for i, (sx, sy) in enumerate(DEEP_SHIFTS):
        pyr = [smooth_pyramid(w, h, levels, 0.0, 0.0), smooth_pyramid(w, h, levels, sx, sy)]
        for win in DEEP_WINDOWS:
            pts, status = points_for(w, h, 129, seed=int(sx * 4))
            for lam in (0.0, lam_for(win)):
                prm = Params(win, 10, 1, lam, 0)
                key = ("deep", w, h, levels, sx, sy, win, lam)
                out.append((f"{w}x{h}x{levels} shift ({sx}, {sy}) window {win} min_lambda {lam}", pyr, pts, status, 2, prm, (i + (lam > 0)) & 1,
                            want_chain(key, pyr, pts, status, 2, prm)))
    return out


# the widest plane the call accepts
WIDE_W, WIDE_H = 1 << 19, 3
WIDE_WINDOWS = (5, 9)


@functools.lru_cache(maxsize=None)
def wide_pyramids():
    """one level of 2^19 x 3: noise smoothed along the rows by a 5-tap box, its contrast stretched to 0 .. 255, against itself rolled by
    one column: the content of A at (x, y) is at (x + 1, y) in B"""
    rng = np.random.RandomState(19)
    n = rng.randint(0, 256, (WIDE_H, WIDE_W + 4)).astype(np.int64)
    c = np.concatenate([np.zeros((WIDE_H, 1), np.int64), n.cumsum(1)], axis=1)
    s = (c[:, 5:] - c[:, :-5]).astype(np.float64) / 5.0                         # [3, 2^19]
    a = np.clip(np.rint((s - s.min()) * (255.0 / (s.max() - s.min()))), 0, 255).astype(np.uint8)
    assert a.shape == (WIDE_H, WIDE_W)
    return _frozen([a]), _frozen([np.roll(a, 1, axis=1)])


@functools.lru_cache(maxsize=None)
def wide_case(window):
    """257 points within 300 columns of the right edge, half of them on the lattice; among them the last pixel, the last lattice
    point before the last column and a point half a pixel from it"""
    w, h = WIDE_W, WIDE_H
    rng = np.random.RandomState(5)
    q = np.stack([32 * (w - 1) - rng.randint(0, 32 * 300, 257), rng.randint(0, 32 * (h - 1) + 1, 257)], axis=1).astype(np.float32) / np.float32(32)
    r = np.stack([w - 1 - 300 * rng.rand(257), (h - 1) * rng.rand(257)], axis=1).astype(np.float32)
    pts = np.where((np.arange(257) & 1)[:, None] == 0, q, r).astype(np.float32)
    pts[:3] = np.float32([(w - 1, h - 1), (w - 1 - 1 / 32, 0), (w - 1.5, 1)])
    status = np.zeros(257, np.int32)
    pts.setflags(write=False), status.setflags(write=False)
    pa, pb = wide_pyramids()
    prm = Params(window, 10, 1, 0.0, 0)
    return [pa, pb], pts, status, 1, prm, want_chain(("wide", window), [pa, pb], pts, status, 1, prm)


# saturated contrast: a checkerboard of 0 / 255 in 2-px squares, |gx| = 8160 at every window pixel of a pixel-centred window
SAT_WINDOWS = (3, 13, 23)
SAT_LEVELS = (1, 3)
SAT_KINDS = ("shifted", "inverse")


@functools.lru_cache(maxsize=None)
def sat_pyramids(levels, kind):
    import texture_ref as T

    w, h = HARD_SHAPE[:2]
    a = T.checkerboard(w, h)
    if kind == "inverse":
        b = (255 - a).astype(np.uint8)
    else:
        b = np.clip(_shift(a, 1, 0).astype(np.int32) + np.random.RandomState(23).randint(-2, 3, (h, w)), 0, 255).astype(np.uint8)
    return _frozen(pyramid(a, levels)), _frozen(pyramid(b, levels))


def sat_case(levels, window, kind):
    w, h = HARD_SHAPE[:2]
    pa, pb = sat_pyramids(levels, kind)
    pts, status = points_for(w, h, 257, seed=window)
    prm = Params(window, 10, 1, 0.0, 0)
    return [pa, pb], pts, status, 1, prm, want_chain(("sat", levels, window, kind), [pa, pb], pts, status, 1, prm)
