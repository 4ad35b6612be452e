"""Inputs shared by the homography tests (CPU and GPU): matches of a known mild homography with noise, outliers and unusable
entries, and the corner error of an estimate."""
import numpy as np

import homography_ref as R

NAN, INF = float("nan"), float("inf")


def true_model(size):
    """a mild perspective in pixels about the image origin: a pan/tilt of a few degrees' worth, scaled to the frame"""
    w, h = size
    s = max(w, h)
    return np.array([1.02, -0.015, 0.012 * w, 0.02, 0.99, -0.008 * h, 0.04 / s, -0.03 / s, 1.0])


def corner_error(m, truth, size):
    w, h = size
    corners = np.array([[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]], np.float64)
    return float(np.abs(R.apply(m, corners) - R.apply(truth, corners)).max())


def noisy_matches(n, size, seed, outliers, noise=0.05):
    """n matches inside the frame: q = truth(p) + N(0, noise) px, a fraction `outliers` of them replaced by uniform positions"""
    w, h = size
    rng = np.random.RandomState(seed)
    truth = true_model(size)
    p = np.stack([rng.uniform(0, w - 1, n), rng.uniform(0, h - 1, n)], axis=1)
    q = R.apply(truth, p) + rng.normal(0, noise, (n, 2))
    out = rng.uniform(0, 1, n) < outliers
    q[out] = np.stack([rng.uniform(0, w - 1, out.sum()), rng.uniform(0, h - 1, out.sum())], axis=1)
    keep = (q[:, 0] >= 0) & (q[:, 0] <= w - 1) & (q[:, 1] >= 0) & (q[:, 1] <= h - 1)
    q[~keep] = p[~keep]                                  # (a match that would leave the frame becomes one more outlier)
    return p.astype(np.float32), q.astype(np.float32)


def matches(n, size, seed, status=False):
    """n matches of true_model(size): noise on and off the lattice, outliers, NaN, infinities, points outside the frame,
    duplicates; with `status`, an int32 array in ofx_track_points' encoding around pair 5"""
    w, h = size
    rng = np.random.RandomState(seed + 13 * n)
    p = np.stack([rng.uniform(0, w - 1, n), rng.uniform(0, h - 1, n)], axis=1)
    q = np.clip(R.apply(true_model(size), p) + rng.normal(0, 0.03, (n, 2)), 0, [w - 1, h - 1])
    kind = rng.randint(0, 20, n)
    out = kind == 6
    q[out] = np.stack([rng.uniform(0, w - 1, out.sum()), rng.uniform(0, h - 1, out.sum())], axis=1)
    p, q = p.astype(np.float32), q.astype(np.float32)
    if n > 8:
        p[kind == 7, 0] = NAN
        q[kind == 8, 1] = INF
        p[kind == 9, 1] = -INF
        q[kind == 10, 0] = np.float32(w - 1) + np.float32(0.25)
        p[kind == 11] = np.float32(-0.03125)
        dup = np.flatnonzero(kind == 12)
        if len(dup):
            p[dup], q[dup] = p[dup[0]], q[dup[0]]                # coincident matches: singular samples
    st = None
    if status:
        st = np.zeros(n, np.int32)
        lost = rng.randint(0, 6, n)
        st[lost == 1] = (4 << 8) | 2
        st[lost == 2] = (5 << 8) | 3
        st[lost == 3] = (6 << 8) | 1
        st[lost == 4] = (400 << 8) | 4
    return p, q, st


DYADIC_MODEL = (0.25, 0.0, 0.0, 0.0, 0.25, 0.0, -1.0, 0.0)          # normalised: X = x / (4 (1 - x)), Y = y / (4 (1 - x))


def dyadic_four():
    """four exact matches of the normalised DYADIC_MODEL in a 257 x 257 frame (e = 12, pixel = 128 (normalised + 1)), no three of
    them on a line: 1 - x is a power of two at each, so every coordinate is on the lattice"""
    xy = np.array([[0.0, 0.0], [0.0, 1.0], [0.5, 1.0], [0.75, -1.0]])
    XY = 0.25 * xy / (1.0 - xy[:, :1])
    return (128.0 * (xy + 1.0)).astype(np.float32), (128.0 * (XY + 1.0)).astype(np.float32), (257, 257)


def wide_sum_matches():
    """2048 matches near the four corners of a 65536 x 65536 frame: every degree-4 term is near +-2^80, and the mixed terms change
    sign from corner to corner"""
    n, size = 2048, (1 << 16, 1 << 16)
    rng = np.random.RandomState(8)
    corner = rng.randint(0, 4, n)
    p = np.stack([(corner & 1) * 65535.0, (corner >> 1) * 65535.0], axis=1) + rng.randint(0, 65, (n, 2)) * (1 - 2 * np.stack([corner & 1, corner >> 1], axis=1))
    p = np.clip(p, 0, 65535)
    q = np.clip(32767.5 + (p - 32767.5) * (1 - 2.0 ** -14) + rng.randint(-3, 4, (n, 2)) / 32.0, 0, 65535)
    return p.astype(np.float32), q.astype(np.float32), size
