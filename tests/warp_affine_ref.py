"""NumPy referee of "affine frame warp" (include/ofx.h; ofx_warp_affine): restated from the definition in int64."""
import numpy as np

BORDER_CONSTANT, BORDER_REPLICATE = 0, 1
BORDERS = {"constant": BORDER_CONSTANT, "replicate": BORDER_REPLICATE}
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def quantise(m):
    """the six int coefficients, or None for a model the call refuses"""
    m = np.asarray(m, np.float64).reshape(6)
    lim = np.array([16, 16, 1 << 20, 16, 16, 1 << 20], np.float64)
    if not np.isfinite(m).all() or (np.abs(m) > lim).any():
        return None
    return [int(np.rint(np.ldexp(v, 21))) for v in m]          # (ties to even; the scaling is exact)


def positions(m, w, h):
    """(qx, qy) int64 [h, w]: the source position of every output pixel in 1/32 px"""
    A, B, Tx, C, D, Ty = quantise(m)
    x, y = np.arange(w, dtype=np.int64)[None, :], np.arange(h, dtype=np.int64)[:, None]
    return (A * x + B * y + Tx + (1 << 15)) >> 16, (C * x + D * y + Ty + (1 << 15)) >> 16


def warp_affine(src, m, out_size=None, border=BORDER_REPLICATE, fill=0):
    """(the warped frame, the number of output pixels out of range); src uint8 [sh, sw] or [sh, sw, 3], out_size (w, h)"""
    border = BORDERS.get(border, border)
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim in (2, 3)
    sh, sw = src.shape[:2]
    w, h = (sw, sh) if out_size is None else out_size
    qx, qy = positions(m, w, h)
    xmax, ymax = 32 * (sw - 1), 32 * (sh - 1)
    inside = (qx >= 0) & (qx <= xmax) & (qy >= 0) & (qy <= ymax)
    qx, qy = np.clip(qx, 0, xmax), np.clip(qy, 0, ymax)
    ix, a, iy, b = qx >> 5, qx & 31, qy >> 5, qy & 31
    ix1, iy1 = np.minimum(ix + 1, sw - 1), np.minimum(iy + 1, sh - 1)
    P = src.astype(np.int64).reshape(sh, sw, -1)
    k = lambda t: t[:, :, None]
    s = k((32 - a) * (32 - b)) * P[iy, ix] + k(a * (32 - b)) * P[iy, ix1] + k((32 - a) * b) * P[iy1, ix] + k(a * b) * P[iy1, ix1]
    out = (s + 512) >> 10
    if border == BORDER_CONSTANT:
        out[~inside] = fill
    return out.astype(np.uint8).reshape((h, w) + src.shape[2:]), int((~inside).sum())
