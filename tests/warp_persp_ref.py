"""NumPy referee of "perspective frame warp" (include/ofx.h; ofx_warp_perspective): restated from the definition, one float64
operation per rounding; from the lattice position on it is warp_affine_ref's arithmetic."""
import numpy as np

from warp_affine_ref import BORDER_CONSTANT, BORDER_REPLICATE, BORDERS  # noqa: F401

IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
LIMITS = (16.0, 16.0, 2.0 ** 20, 16.0, 16.0, 2.0 ** 20, 1.0, 1.0, 16.0)
f64 = np.float64


def accepted(m):
    """whether the call takes the model"""
    m = np.asarray(m, f64).reshape(9)
    return bool(np.isfinite(m).all() and (np.abs(m) <= np.array(LIMITS)).all())


def positions(m, w, h):
    """(qx, qy, defined): int64 [h, w] source positions in 1/32 px (0 where undefined) and bool [h, w]"""
    assert accepted(m)
    m = [f64(v) for v in np.asarray(m, f64).reshape(9)]
    x, y = np.arange(w, dtype=f64)[None, :], np.arange(h, dtype=f64)[:, None]
    with np.errstate(all="ignore"):
        X = (m[0] * x + m[1] * y) + m[2]
        Y = (m[3] * x + m[4] * y) + m[5]
        W = (m[6] * x + m[7] * y) + m[8]
        r = f64(1.0) / W
        fx, fy = np.ldexp(X * r, 5), np.ldexp(Y * r, 5)
        defined = (W > 0) & np.isfinite(fx) & np.isfinite(fy) & (np.abs(fx) <= 2.0 ** 40) & (np.abs(fy) <= 2.0 ** 40)
    qx = np.rint(np.where(defined, fx, 0.0)).astype(np.int64)        # (ties to even)
    qy = np.rint(np.where(defined, fy, 0.0)).astype(np.int64)
    return qx, qy, defined


def warp_perspective(src, m, out_size=None, border=BORDER_REPLICATE, fill=0):
    """(the warped frame, the number of output pixels undefined or out of range); src uint8 [sh, sw] or [sh, sw, 3], out_size (w, h)"""
    border = BORDERS.get(border, border)
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim in (2, 3)
    sh, sw = src.shape[:2]
    w, h = (sw, sh) if out_size is None else out_size
    qx, qy, defined = positions(m, w, h)
    xmax, ymax = 32 * (sw - 1), 32 * (sh - 1)
    inside = defined & (qx >= 0) & (qx <= xmax) & (qy >= 0) & (qy <= ymax)
    qx, qy = np.clip(qx, 0, xmax), np.clip(qy, 0, ymax)
    ix, a, iy, b = qx >> 5, qx & 31, qy >> 5, qy & 31
    ix1, iy1 = np.minimum(ix + 1, sw - 1), np.minimum(iy + 1, sh - 1)
    P = src.astype(np.int64).reshape(sh, sw, -1)
    k = lambda t: t[:, :, None]
    s = k((32 - a) * (32 - b)) * P[iy, ix] + k(a * (32 - b)) * P[iy, ix1] + k((32 - a) * b) * P[iy1, ix] + k(a * b) * P[iy1, ix1]
    out = (s + 512) >> 10
    if border == BORDER_CONSTANT:
        out[~inside] = fill
    out[~defined] = fill
    return out.astype(np.uint8).reshape((h, w) + src.shape[2:]), int((~inside).sum())
