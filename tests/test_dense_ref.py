"""CPU, the oracle only: the restatement of "coarse-to-fine propagation" (tests/dense_ref.py) on hand-made fields, and what the
dense flow buys -- the share of pixels within 1 px of the true motion on scenes that move by more than the window can see, and the
in-between frames of a moving texture -- against the reference's way (one global shift per level plus a local estimate).  The bars
are the issue's; every figure is printed before it is asserted."""
import functools

import numpy as np
import pytest

import dense_ref as D
import interp_ref as IR

F32 = np.float32
NAN, INF = F32("nan"), F32("inf")


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _field(hc, wc, fn):
    ys, xs = np.mgrid[0:hc, 0:wc]
    return np.stack([fn(xs, ys), fn(ys, xs)], axis=2).astype(F32)


# ---- prolong on hand-made fields --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("odd_w", [0, 1])
@pytest.mark.parametrize("odd_h", [0, 1])
def test_a_constant_field_comes_back_doubled(odd_w, odd_h):
    c = np.empty((3, 5, 2), F32)
    c[...] = (1.25, -3.5)
    f = D.prolong(c, 10 + odd_w, 6 + odd_h, 1.0, 0.0)
    assert f.shape == (6 + odd_h, 10 + odd_w, 2) and f.dtype == F32
    assert np.array_equal(_bits(f), _bits(np.broadcast_to(np.array([2.5, -7.0], F32), f.shape)))


def test_a_ramp_is_exact_at_even_positions_and_midway_at_odd_ones():
    c = _field(4, 6, lambda a, b: 3.0 * a + 0.25 * b)
    f = D.prolong(c, 13, 9, 1.0, 0.0)
    assert np.array_equal(f[0::2, 0::2][:4, :6], 2 * c)
    assert np.array_equal(f[0:8:2, 1:11:2], c[:, :-1] + c[:, 1:])           # midway, doubled
    assert np.array_equal(f[1:7:2, 0:12:2], c[:-1] + c[1:])
    assert np.array_equal(f[1:7:2, 1:11:2], (c[:-1, :-1] + c[:-1, 1:] + c[1:, :-1] + c[1:, 1:]) / 2)
    # beyond the last coarse sample the field is held: column 11 (x0 = x1 = 5), column 12 and row 8 of the odd sizes, row 7
    assert np.array_equal(f[0:8:2, 11], 2 * c[:, 5]) and np.array_equal(f[0:8:2, 12], 2 * c[:, 5])
    assert np.array_equal(f[7, 0:12:2], 2 * c[3]) and np.array_equal(f[8, 0:12:2], 2 * c[3])


def test_one_coarse_pixel():
    c = np.array([[[1.5, -2.0]]], F32)
    for w, h in ((2, 2), (3, 3), (2, 3), (3, 2)):
        f = D.prolong(c, w, h, 1.0, 0.0)
        assert f.shape == (h, w, 2) and np.array_equal(f, np.broadcast_to(np.array([3.0, -4.0], F32), (h, w, 2)))
    with pytest.raises(AssertionError):
        D.prolong(c, 4, 2)


def test_sanitise():
    scale, max_px = D.ITER_SCALE, 9.0
    # the largest float whose rounded product with the scale is still <= max_px, and the next one
    lim = F32(max_px / float(scale))
    while F32(scale * lim) > F32(max_px):
        lim = np.nextafter(lim, F32(0))
    while F32(scale * np.nextafter(lim, INF)) <= F32(max_px):
        lim = np.nextafter(lim, INF)
    above = np.nextafter(lim, INF)
    assert F32(scale * lim) <= F32(max_px) < F32(scale * above)
    c = np.zeros((2, 8, 2), F32)
    c[0, :, 0] = [NAN, INF, -INF, 1e30, above, -above, lim, -lim]
    c[0, :, 1] = 1.0
    c[1, :, 1] = [NAN, INF, -INF, -1e30, above, -above, lim, -lim]
    c[1, :, 0] = -1.0
    s = D.sanitise(c, scale, max_px)
    assert np.array_equal(_bits(s[:, :6]), np.zeros((2, 6, 2), np.uint32)), "a bad component takes the whole vector to (+0, +0)"
    assert np.array_equal(_bits(s[:, 6:]), _bits(c[:, 6:])), "a vector just below the threshold survives"
    s0 = D.sanitise(c, scale, 0.0)                       # max_px = 0: only the finiteness test
    assert np.array_equal(_bits(s0[:, :3]), np.zeros((2, 3, 2), np.uint32)) and np.array_equal(_bits(s0[:, 3:]), _bits(c[:, 3:]))
    f = D.prolong(c, 16, 4, scale, max_px)
    assert np.isfinite(f).all() and np.array_equal(f[0, 12], 2 * c[0, 6]) and np.array_equal(f[0, 14], 2 * c[0, 7])
    assert not f[:, :10].any(), "nothing of a sanitised vector reaches its neighbours"


def test_minus_zero_survives_at_even_positions():
    c = np.full((2, 3, 2), -0.0, F32)
    f = D.prolong(c, 7, 5, 1.0, 9.0)
    assert np.signbit(f[0:4:2, 0:6:2]).all()
    assert not np.signbit(f[0, 1]).any(), "-0 + 0.5 * (-0 - -0) is +0: the odd positions do the arithmetic"
    assert np.array_equal(_bits(D.prolong(np.zeros((2, 3, 2), F32), 7, 5, 1.0, 9.0)), np.zeros((5, 7, 2), np.uint32))


# ---- the quality bars, on the oracle ----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _scores(name, seed):
    from oracle import Oracle

    orc = Oracle()
    prev, nxt, truth = D.scene(name, seed)
    dense = D.dense_displacement(orc, prev, nxt, D.S_LEVELS, D.S_WIN, D.S_ITERS, D.S_MIN_DET)
    exist = D.existing_displacement(orc, prev, nxt, D.S_LEVELS, D.S_WIN, D.S_ITERS, D.S_MIN_DET)
    out = D.score(dense, truth), D.score(exist, truth)
    print(f"scene {name} seed {seed}: dense {out[0]:.3f}, existing {out[1]:.3f}")
    return out


@pytest.mark.parametrize("seed", D.S_SEEDS)
@pytest.mark.parametrize("name", ["split", "split2"])
def test_two_motions_in_one_scene(name, seed):
    dense, exist = _scores(name, seed)
    assert dense >= 0.85, (name, seed, dense)
    if name == "split":
        assert exist <= 0.45, (name, seed, exist)


@pytest.mark.parametrize("seed", D.S_SEEDS)
def test_a_pan_beyond_the_window(seed):
    dense, exist = _scores("pan", seed)
    assert dense >= 0.75, (seed, dense)
    assert exist <= 0.30, (seed, exist)


@pytest.mark.parametrize("seed", D.S_SEEDS)
def test_a_small_motion_stays_right(seed):
    dense, _ = _scores("small", seed)
    assert dense >= 0.98, (seed, dense)


@functools.lru_cache(maxsize=None)
def _ratios(step, levels):
    from oracle import Oracle

    orc = Oracle()
    frames = IR.quality_clip(step)
    dense = D.interp_ratios(frames, lambda i, j: D.dense_displacement(orc, frames[i], frames[j], levels, IR.Q_WIN, 3, D.S_MIN_DET))
    exist = D.interp_ratios(frames, lambda i, j: D.existing_displacement(orc, frames[i], frames[j], levels, IR.Q_WIN, 3, D.S_MIN_DET))
    print(f"step {step}, {levels} levels: SAD(interp) / SAD(cross-fade) dense {min(dense):.2f} .. {max(dense):.2f}, "
          f"existing {min(exist):.2f} .. {max(exist):.2f}")
    return dense, exist


@pytest.mark.parametrize("step", [(1.0, 0.5), (2.0, 1.0)], ids=str)
def test_in_between_frames_of_a_moving_texture(step):
    dense, exist = _ratios(step, 3)
    assert max(dense) < 0.25, (step, dense)
    assert max(dense) < max(exist), (step, dense, exist)


def test_in_between_frames_of_a_fast_texture_figures():
    """(3.0, -1.5) per frame at 4 levels: the third row of the table in DESIGN.md; the issue sets no bar for it"""
    dense, exist = _ratios((3.0, -1.5), 4)
    assert all(np.isfinite(dense)) and all(np.isfinite(exist))
