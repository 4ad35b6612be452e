"""CPU: the NumPy referee of ofx_warp_affine (tests/warp_affine_ref.py) alone -- the identity and whole-pixel shifts are exact,
both border modes, the outside counts from geometry, the quantisation, and the rounding of the value at a hand-made 2 x 2 plane."""
import numpy as np
import pytest

import warp_affine_ref as W


def image(w, h, channels=1, seed=0):
    rng = np.random.RandomState(seed + w + 1000 * h)
    return rng.randint(0, 256, (h, w) if channels == 1 else (h, w, 3)).astype(np.uint8)


@pytest.mark.parametrize("channels", [1, 3])
def test_the_identity_copies_the_source(channels):
    src = image(37, 21, channels)
    for border in ("replicate", "constant"):
        out, outside = W.warp_affine(src, W.IDENTITY, border=border, fill=99)
        assert np.array_equal(out, src) and outside == 0


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("dx,dy", [(3, 0), (0, -2), (-5, 4), (36, 0), (40, 30)])
def test_a_whole_pixel_shift_is_a_shifted_copy(channels, dx, dy):
    w, h = 37, 21
    src = image(w, h, channels, 1)
    m = (1.0, 0.0, float(dx), 0.0, 1.0, float(dy))           # output (x, y) shows the source at (x + dx, y + dy)
    ys, xs = np.arange(h)[:, None] + dy, np.arange(w)[None, :] + dx
    inside = (xs >= 0) & (xs < w) & (ys >= 0) & (ys < h)
    want_outside = w * h - max(w - abs(dx), 0) * max(h - abs(dy), 0)
    rep, n_rep = W.warp_affine(src, m, border="replicate")
    con, n_con = W.warp_affine(src, m, border="constant", fill=7)
    assert n_rep == n_con == want_outside == int((~inside).sum())
    assert np.array_equal(rep, src[np.clip(ys, 0, h - 1), np.clip(xs, 0, w - 1)])
    assert np.array_equal(con[inside], src[np.clip(ys, 0, h - 1), np.clip(xs, 0, w - 1)][inside])
    assert (con[~inside] == 7).all()


def test_the_value_at_a_hand_made_plane():
    src = np.array([[10, 20], [30, 41]], np.uint8)
    at = lambda tx, ty, **kw: int(W.warp_affine(src, (1.0, 0.0, tx, 0.0, 1.0, ty), (1, 1), **kw)[0][0, 0])
    assert at(0.0, 0.0) == 10 and at(1.0, 0.0) == 20 and at(0.0, 1.0) == 30 and at(1.0, 1.0) == 41
    # (16, 16) / 32: s = 256 (10 + 20 + 30 + 41) = 25856; (25856 + 512) >> 10 = 25  (25.25 rounds down)
    assert at(0.5, 0.5) == 25
    # (16, 0) / 32: s = 512 (10 + 20) = 15360 -> exactly 15; (0, 16) / 32: s = 512 (10 + 30) -> 20
    assert at(0.5, 0.0) == 15 and at(0.0, 0.5) == 20
    # (31, 31) / 32: s = 1 * 10 + 31 * 20 + 31 * 30 + 961 * 41 = 40961; (40961 + 512) >> 10 = 40  (40.0009..)
    assert at(31 / 32, 31 / 32) == 40
    # (1, 0) / 32: s = 31 * 32 * 10 + 1 * 32 * 20 = 10560; (10560 + 512) >> 10 = 10  (10.3125); (16, 31) / 32 between 30 and 41 mostly:
    # s = 16 * 1 * 10 + 16 * 1 * 20 + 16 * 31 * 30 + 16 * 31 * 41 = 480 + 35216 = 35696; + 512 >> 10 = 35  (35.36)
    assert at(1 / 32, 0.0) == 10 and at(0.5, 31 / 32) == 35
    # a half rounds up: planes (0, 1; 0, 1) at (16, 0) / 32: s = 512 -> (512 + 512) >> 10 = 1
    half = np.array([[0, 1], [0, 1]], np.uint8)
    assert int(W.warp_affine(half, (1.0, 0.0, 0.5, 0.0, 1.0, 0.0), (1, 1))[0][0, 0]) == 1
    # the position rounds to the lattice to nearest, a half up: 1/64 px -> (2^15 + 2^15) >> 16 = 1, just below it -> 0
    assert W.positions((1.0, 0.0, 1 / 64, 0.0, 1.0, 0.0), 1, 1)[0][0, 0] == 1
    assert W.positions((1.0, 0.0, 1 / 64 - 2.0 ** -21, 0.0, 1.0, 0.0), 1, 1)[0][0, 0] == 0
    assert W.positions((1.0, 0.0, -1 / 64, 0.0, 1.0, 0.0), 1, 1)[0][0, 0] == 0
    assert W.positions((1.0, 0.0, -1 / 64 - 2.0 ** -21, 0.0, 1.0, 0.0), 1, 1)[0][0, 0] == -1
    # out of range by one lattice step: replicate clamps to the last pixel, constant fills
    assert at(1.0 + 1 / 32, 0.0) == 20 and at(1.0 + 1 / 32, 0.0, border="constant", fill=200) == 200
    assert at(-1 / 32, 0.0, border="constant", fill=200) == 200 and at(0.0, 1.0, border="constant", fill=200) == 30


def test_the_quantisation_and_its_limits():
    assert W.quantise(W.IDENTITY) == [1 << 21, 0, 0, 0, 1 << 21, 0]
    assert W.quantise((16.0, -16.0, 1048576.0, 0.0, 2.0 ** -22, -1048576.0)) == [1 << 25, -(1 << 25), 1 << 41, 0, 0, -(1 << 41)]
    assert W.quantise((0, 0, 1.5 * 2.0 ** -21, 0, 0, 2.5 * 2.0 ** -21))[2::3] == [2, 2], "ties go to even"
    for bad in ((16.000001, 0, 0, 0, 1, 0), (1, 0, 1048576.5, 0, 1, 0), (1, 0, 0, float("nan"), 1, 0), (1, float("inf"), 0, 0, 1, 0), (1, 0, 0, 0, 1, -2.0 ** 21)):
        assert W.quantise(bad) is None


@pytest.mark.parametrize("channels", [1, 3])
def test_a_rotation_counts_the_pixels_whose_source_is_out_of_range(channels):
    w, h, sw, sh = 45, 31, 33, 40
    src = image(sw, sh, channels, 2)
    c, s = 1.1 * np.cos(0.3), 1.1 * np.sin(0.3)
    m = (c, -s, 2.25, s, c, -6.5)
    qx, qy = W.positions(m, w, h)
    inside = (qx >= 0) & (qx <= 32 * (sw - 1)) & (qy >= 0) & (qy <= 32 * (sh - 1))
    assert 0 < inside.sum() < w * h
    # the positions are the real ones to half a lattice step plus the quantisation of the model (2^-22 per coefficient)
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    assert np.abs(qx / 32 - (c * x - s * y + 2.25)).max() <= 1 / 64 + 1e-4
    rep, n_rep = W.warp_affine(src, m, (w, h), "replicate")
    con, n_con = W.warp_affine(src, m, (w, h), "constant", 255)
    assert rep.shape == con.shape == ((h, w) if channels == 1 else (h, w, 3))
    assert n_rep == n_con == int((~inside).sum())
    assert np.array_equal(rep[inside], con[inside]) and (con[~inside] == 255).all()
    # a convex combination of four taps: within their range
    P = src.reshape(sh, sw, -1).astype(int)
    ix, iy = np.clip(qx, 0, 32 * (sw - 1)) >> 5, np.clip(qy, 0, 32 * (sh - 1)) >> 5
    taps = np.stack([P[iy, ix], P[iy, np.minimum(ix + 1, sw - 1)], P[np.minimum(iy + 1, sh - 1), ix], P[np.minimum(iy + 1, sh - 1), np.minimum(ix + 1, sw - 1)]])
    r = rep.reshape(h, w, -1).astype(int)
    assert (r >= taps.min(axis=0)).all() and (r <= taps.max(axis=0)).all()


def test_a_map_that_leaves_the_source_entirely():
    src = image(9, 7, 1, 3)
    rep, n = W.warp_affine(src, (1.0, 0.0, 500.0, 0.0, 1.0, -500.0), (5, 4), "replicate")
    assert n == 20 and (rep == src[0, 8]).all()
    con, n = W.warp_affine(src, (-16.0, 16.0, -1048576.0, 16.0, -16.0, 1048576.0), (5, 4), "constant", 3)
    assert n == 20 and (con == 3).all()
