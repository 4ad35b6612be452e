"""The referee of texture strength and feature selection (include/ofx.h, "texture strength and feature selection") in NumPy, and
the inputs its tests share.  No GPU.

The sums are the oracle's: Oracle.level_planes(p3, p3, window, lk_float) gives Ix, Iy (integers of magnitude <= 1020 in float
planes) and the window sums.  The oracle forms each sum exactly in double and then rounds it ONCE to float32 (orc_srm_1ch_f32_exact),
so above 2^24 its planes are not the definition's exact integers any more.  exact_sums() therefore adds the oracle's Ix, Iy up
again in int64 over the same clipped windows and asserts that the oracle's planes are these integers rounded once to float32 and
that every sum is below 2^31 -- which is what tests/test_gpu_parity.py asserts of ofx_lk_level_sums' exact planes."""
import numpy as np

from cuda_optical_flow_2_amd import synth

import iter_hard

WINDOWS = (3, 9, 23)
ALL_WINDOWS = tuple(range(3, 24, 2))                      # one instance of csrc/texture.hip's strength_kernel<R> each
LK_FLOAT = 1
STRIP = 64                                                # kStrip of csrc/texture.hip: the output rows of a block
INSTANCE_INPUTS = ("noise", "checker", "hard")


def tile_out(win):
    """the output columns of a block of csrc/texture.hip: kTile - 2R"""
    return 256 - 2 * (win >> 1)


def instance_shapes(win):
    """(w, h), the fewest that still tell an instance's constants: one column past a tile seam and one row past a strip (the ring of
    2R + 1 rows wraps 65 / (2R + 1) times), two tiles and two strips of odd size, a field smaller than the window, one pixel"""
    return [(tile_out(win) + 1, STRIP + 1), (263, 75), (5, 4), (1, 1)]


# ---- the definition -----------------------------------------------------------------------------------------------------------
def _box(a, r):
    """the sum of the int64 plane a over the (2r + 1)^2 window clipped at the image"""
    h, w = a.shape
    ii = np.zeros((h + 1, w + 1), np.int64)
    ii[1:, 1:] = a.cumsum(0).cumsum(1)
    y0, y1 = np.clip(np.arange(h) - r, 0, h), np.clip(np.arange(h) + r + 1, 0, h)
    x0, x1 = np.clip(np.arange(w) - r, 0, w), np.clip(np.arange(w) + r + 1, 0, w)
    return ii[y1][:, x1] - ii[y0][:, x1] - ii[y1][:, x0] + ii[y0][:, x0]


def exact_sums(orc, p, window):
    """(Sxx, Syy, Sxy) of step 1 as int64 planes"""
    p = np.ascontiguousarray(p, np.uint8)
    p3 = synth.to_3ch(p)
    ix, iy, _, s = orc.level_planes(p3, p3, window, LK_FLOAT, exact_sums=True)
    assert (ix == np.rint(ix)).all() and (iy == np.rint(iy)).all() and np.abs(ix).max() <= 1020 and np.abs(iy).max() <= 1020
    ix, iy = ix.astype(np.int64), iy.astype(np.int64)
    r = window >> 1
    out = [_box(ix * ix, r), _box(iy * iy, r), _box(ix * iy, r)]
    for k, e in enumerate(out):
        assert (s[k] == np.rint(s[k])).all() and np.abs(s[k]).max() < 2.0 ** 31, f"plane {k}: the oracle's sums are no integers below 2^31"
        assert np.abs(e).max() < 2 ** 31
        assert np.array_equal(e.astype(np.float32), s[k].astype(np.float32)), f"plane {k}: the oracle's sum is not the exact one rounded once"
    return out


def strength_of_sums(sxx, syy, sxy):
    """steps 2 and 3: float64, one rounding per operation (NumPy fuses nothing), then one rounding to float32"""
    sxx, syy, sxy = (np.asarray(a, np.int64) for a in (sxx, syy, sxy))
    tr = (sxx + syy).astype(np.float64)
    d = (sxx - syy).astype(np.float64)
    b = sxy.astype(np.float64)
    q = d * d
    p2 = b * b
    p4 = 4.0 * p2
    r = q + p4
    s = np.sqrt(r)
    m = tr - s
    lam = 0.5 * m
    out = np.where(lam > 0, lam, 0.0).astype(np.float32)
    assert not np.isnan(out).any() and not np.signbit(out).any()
    return out


def strength(orc, p, window):
    return strength_of_sums(*exact_sums(orc, p, window))


def grid(w, h, c):
    return (w + c - 1) // c, (h + c - 1) // c      # ncx, ncy


def default_border(window):
    return window // 2 + 1


def candidates(R, border, min_strength):
    """(inside the border, candidate) as bool planes"""
    R = np.asarray(R, np.float32)
    h, w = R.shape
    yy, xx = np.mgrid[0:h, 0:w]
    inside = (xx >= border) & (xx < w - border) & (yy >= border) & (yy < h - border)
    pad = np.full((h + 2, w + 2), -np.inf, np.float32)      # a neighbour outside the image is no neighbour
    pad[1:-1, 1:-1] = R
    cand = inside & (R > np.float32(min_strength))
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy == 0 and dx == 0:
                continue
            n = pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
            cand &= (R > n) if (dy < 0 or (dy == 0 and dx < 0)) else (R >= n)
    return inside, cand


def select(R, cell, border, min_strength):
    """(cells int32 [ncy, ncx, 2], cell_strength float32 [ncy, ncx], stats int64 [4])"""
    R = np.asarray(R, np.float32)
    h, w = R.shape
    ncx, ncy = grid(w, h, cell)
    inside, cand = candidates(R, border, min_strength)
    cells = np.full((ncy, ncx, 2), -1, np.int32)
    cs = np.zeros((ncy, ncx), np.float32)
    ys, xs = np.nonzero(cand)
    order = np.lexsort((ys * w + xs, -R[ys, xs].astype(np.float64)))     # the largest R first, then the smallest index
    for i in order[::-1]:                                                # (the best of a cell is written last)
        cells[ys[i] // cell, xs[i] // cell] = (xs[i], ys[i])
        cs[ys[i] // cell, xs[i] // cell] = R[ys[i], xs[i]]
    stats = np.array([ncx * ncy, int((cells[..., 0] >= 0).sum()), int(cand.sum()), int((inside & ~(R > np.float32(min_strength))).sum())], np.int64)
    return cells, cs, stats


def compact(cells, max_points=None):
    """(points float32 [n, 2], occupied) of the compaction"""
    c = np.asarray(cells, np.int32).reshape(-1, 2)
    pts = c[c[:, 0] >= 0].astype(np.float32)
    return (pts if max_points is None else pts[:max_points]), len(pts)


def good_features(orc, p, window, cell=16, border=None, min_strength=0.0, max_points=None):
    """what engine.good_features returns"""
    R = strength(orc, p, window)
    cells, cs, _ = select(R, cell, default_border(window) if border is None else border, min_strength)
    pts, _ = compact(cells, max_points)
    return pts, cs.reshape(-1)[cells.reshape(-1, 2)[:, 0] >= 0][:len(pts)]


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def checkerboard(w, h, square=2):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((((xx // square) + (yy // square)) & 1) * 255).astype(np.uint8)


def hard_frame(w=264, h=80):
    return iter_hard.hard_frames(w, h, 2, seed=5)[0]


INPUTS = ("smooth", "noise", "hard", "checker", "const")


def make_input(kind, w, h):
    if kind == "smooth":
        return synth.smooth_pair(w, h)[0]
    if kind == "noise":
        return synth.random_pair(w, h, seed=3 * w + h)[0]
    if kind == "hard":
        return hard_frame(w, h)
    if kind == "checker":
        return checkerboard(w, h)
    if kind == "const":
        return np.full((h, w), 77, np.uint8)
    if kind == "tiled":         # an 8 x 8 patch of noise repeated: away from the edge every strength occurs again 8 pixels on
        return np.tile(synth.random_pair(8, 8, seed=11)[0], ((h + 7) // 8, (w + 7) // 8))[:h, :w].copy()
    raise ValueError(kind)
