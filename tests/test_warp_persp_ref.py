"""CPU: the NumPy referee of ofx_warp_perspective (tests/warp_persp_ref.py) alone -- the identity and whole-pixel shifts are exact,
affine models on the 1/32 lattice give warp_affine_ref's bytes, and a horizon that crosses the output, a pixel with W exactly 0
included, gives `fill` and counts under either border mode."""
import numpy as np
import pytest

import warp_affine_ref as A
import warp_persp_ref as W


def image(w, h, channels=1, seed=0):
    rng = np.random.RandomState(seed + w + 1000 * h)
    return rng.randint(0, 256, (h, w) if channels == 1 else (h, w, 3)).astype(np.uint8)


def lattice_models(sw, sh):
    """affine models whose six entries are multiples of 1/32"""
    return [(1.0, 0.0, 3 / 32, 0.0, 1.0, 17 / 32), (1.0, 0.0, -33 / 32, 0.0, 1.0, -31 / 32), (29 / 32, 11 / 32, -1.75, -7 / 32, 34 / 32, 0.625),
            (-1.0, 0.5, sw - 1.0, 0.25, -1.0, sh - 1.0), (16.0, -16.0, 1048576.0, -16.0, 16.0, -1048576.0), (0.0, 0.0, 2.5, 0.0, 0.0, 1.03125)]


@pytest.mark.parametrize("channels", [1, 3])
def test_the_identity_copies_the_source(channels):
    src = image(37, 21, channels)
    for border in ("replicate", "constant"):
        out, outside = W.warp_perspective(src, W.IDENTITY, border=border, fill=99)
        assert np.array_equal(out, src) and outside == 0
    # any positive scale of the identity is the identity: X r = x exactly when m0 = m8 is a power of two
    out, outside = W.warp_perspective(src, tuple(4.0 * v for v in W.IDENTITY))
    assert np.array_equal(out, src) and outside == 0


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("dx,dy", [(3, 0), (0, -2), (-5, 4), (40, 30)])
def test_a_whole_pixel_shift_is_a_shifted_copy(channels, dx, dy):
    w, h = 37, 21
    src = image(w, h, channels, 1)
    m = (1.0, 0.0, float(dx), 0.0, 1.0, float(dy), 0.0, 0.0, 1.0)
    ys, xs = np.arange(h)[:, None] + dy, np.arange(w)[None, :] + dx
    inside = (xs >= 0) & (xs < w) & (ys >= 0) & (ys < h)
    rep, n_rep = W.warp_perspective(src, m, border="replicate")
    con, n_con = W.warp_perspective(src, m, border="constant", fill=7)
    assert n_rep == n_con == int((~inside).sum())
    assert np.array_equal(rep, src[np.clip(ys, 0, h - 1), np.clip(xs, 0, w - 1)])
    assert np.array_equal(con[inside], src[np.clip(ys, 0, h - 1), np.clip(xs, 0, w - 1)][inside]) and (con[~inside] == 7).all()


@pytest.mark.parametrize("channels", [1, 3])
def test_affine_models_on_the_lattice_give_the_affine_warps_bytes(channels):
    sw, sh = 45, 31
    src = image(sw, sh, channels, 2)
    for m6 in lattice_models(sw, sh):
        for border in ("replicate", "constant"):
            want, want_n = A.warp_affine(src, m6, (40, 33), border, 5)
            got, got_n = W.warp_perspective(src, tuple(m6) + (0.0, 0.0, 1.0), (40, 33), border, 5)
            assert np.array_equal(got, want) and got_n == want_n, (m6, border)


def test_the_limits_of_the_model():
    assert W.accepted(W.IDENTITY) and W.accepted(W.LIMITS) and W.accepted(tuple(-v for v in W.LIMITS))
    for k in range(9):
        for v in (np.nan, np.inf, -np.inf, W.LIMITS[k] * (1 + 2.0 ** -50), -W.LIMITS[k] * (1 + 2.0 ** -50)):
            m = list(W.IDENTITY)
            m[k] = v
            assert not W.accepted(m)


@pytest.mark.parametrize("channels", [1, 3])
def test_a_horizon_inside_the_frame(channels):
    """W = 1 - y / 8 on 16 rows: rows 0 .. 7 are in front of the horizon, row 8 is on it (W exactly 0), rows 9 .. 15 behind it"""
    w, h = 12, 16
    src = image(w, h, channels, 3)
    m = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, -0.125, 1.0)
    qx, qy, defined = W.positions(m, w, h)
    assert defined[:8].all() and not defined[8:].any()
    for border in ("replicate", "constant"):
        out, outside = W.warp_perspective(src, m, border=border, fill=200)
        assert (out[8:] == 200).all(), "an undefined pixel gets fill under either border mode"
        assert np.array_equal(out[0], src[0]), "W = 1 on row 0: the identity there"
        # row 4: W = 1/2, the source position is (2 x, 8): inside for x <= 5
        inside = 2 * np.arange(w) <= w - 1
        assert np.array_equal(out[4][inside], src[8, 2 * np.arange(w)[inside]])
        assert outside == int((~defined).sum()) + int((defined & ((qx > 32 * (w - 1)) | (qy > 32 * (h - 1)))).sum())
        if border == "constant":
            assert (out[4][~inside] == 200).all()
        else:
            assert (out[4][~inside] == src[8, w - 1]).all()
    # W < 0 everywhere, and a position beyond 2^40 / 32 px from a tiny W
    out, outside = W.warp_perspective(src, (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, -1.0), border="replicate", fill=9)
    assert (out == 9).all() and outside == w * h
    out, outside = W.warp_perspective(src, (1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 2.0 ** -40), (3, 1), "replicate", 9)
    assert (out == 9).all() and outside == 3
    # exactly 2^40 is still a position: X r 32 = 2^40 at x = 0 with m2 = 2^-5 ... and out of range, so replicate clamps it
    qx, qy, defined = W.positions((0.0, 0.0, 2.0 ** -5, 0.0, 0.0, 0.0, 0.0, 0.0, 2.0 ** -40), 1, 1)
    assert defined.all() and int(qx[0, 0]) == 1 << 40


def test_the_position_rounds_to_the_lattice_ties_to_even():
    at = lambda tx: int(W.positions((1.0, 0.0, tx, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0), 1, 1)[0][0, 0])
    assert at(1 / 64) == 0 and at(3 / 64) == 2 and at(-1 / 64) == 0 and at(-3 / 64) == -2 and at(1 / 64 + 2.0 ** -30) == 1
    # a division that rounds: W = 3, X = 1 -> fx = 32 * fl(fl(1/3)) = 10.67 -> 11
    assert int(W.positions((0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 3.0), 1, 1)[0][0, 0]) == 11
