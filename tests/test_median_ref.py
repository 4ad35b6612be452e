"""CPU: the referee of the flow median (tests/median_ref.py) on hand-made fields, and what the median buys on the oracle alone --
the quality experiment of DESIGN.md section 4.15: dense_ref's scenes and score, 192x128, 4 levels, 9x9, 3 iterations, min_det 1.0,
with no median, 3x3 and 5x5, and the in-between frames of interp_ref.quality_clip.  Every figure is printed before it is asserted."""
import functools

import numpy as np
import pytest

import dense_ref as D
import interp_ref as IR
import median_ref as M

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _smooth(w, h):
    ys, xs = np.mgrid[0:h, 0:w].astype(F32)
    return np.stack([F32(0.25) * xs + F32(0.125) * ys, F32(-0.5) * ys + F32(3.0)], axis=2).astype(F32)


# ---- hand-made fields -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r", [1, 2])
def test_a_constant_field_comes_back(r):
    f = np.empty((7, 9, 2), F32)
    f[..., 0], f[..., 1] = F32(1.25), F32(-7.5)
    assert np.array_equal(_bits(M.median(f, r)), _bits(f))


@pytest.mark.parametrize("r", [1, 2])
def test_one_wild_vector_in_a_smooth_field_disappears(r):
    f = _smooth(12, 10)
    clean = M.median(f, r)
    g = f.copy()
    g[5, 6] = (F32(1e6), F32(-1e6))
    got = M.median(g, r)
    assert np.abs(got - f).max() <= 0.75, "every result is a value of the smooth neighbourhood"
    assert np.isin(_bits(got[..., 0]), _bits(f[..., 0])).all() and np.isin(_bits(got[..., 1]), _bits(f[..., 1])).all(), "a selection: no new value"
    # in the interior a linear ramp is its own median: the wild vector is gone and its neighbours moved by at most one place in the order
    assert np.array_equal(_bits(clean[r:-r, r:-r]), _bits(f[r:-r, r:-r]))
    assert np.abs(got[5, 6] - f[5, 6]).max() <= 0.25


@pytest.mark.parametrize("r", [1, 2])
def test_a_vertical_step_edge_stays_where_it_is(r):
    f = np.zeros((9, 12, 2), F32)
    f[:, :6] = (F32(7.0), F32(3.0))
    f[:, 6:] = (F32(-6.0), F32(-2.0))
    assert np.array_equal(_bits(M.median(f, r)), _bits(f))


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("comp", [0, 1])
def test_a_component_that_is_not_finite_zeroes_the_whole_vector(bad, comp):
    # a 3x3 window of four vectors (2, 2) and five with one bad component and 9 in the other: were only the bad component zeroed,
    # the other component's values would be 2 2 2 2 [9] 9 9 9 9 -- with the whole vector zeroed they are 0 0 0 0 [0] 2 2 2 2 in both
    f = np.full((3, 3, 2), 2.0, F32)
    for (y, x) in ((0, 0), (0, 2), (2, 0), (2, 2), (1, 1)):
        f[y, x, comp], f[y, x, 1 - comp] = bad, 9.0
    got = M.median(f, 1)[1, 1]
    assert np.array_equal(_bits(got), _bits(np.zeros(2, F32))), got
    assert np.isfinite(M.median(f, 2)).all()


def test_a_minus_zero_result_is_stored_as_plus_zero():
    f = np.full((5, 5, 2), -0.0, F32)
    for r in (1, 2):
        assert np.array_equal(_bits(M.median(f, r)), np.zeros((5, 5, 2), np.uint32))
    g = np.full((3, 3, 2), -0.0, F32)
    g[0, :, :] = F32(1.0)                                     # three ones, six -0: the middle is a zero
    assert np.array_equal(_bits(M.median(g, 1)[1, 1]), np.zeros(2, np.uint32))


def test_denormals_survive():
    d = np.array(M.DENORM, F32)
    assert (d != 0).all() and (np.abs(d) < np.finfo(F32).tiny).all()
    f = np.empty((6, 6, 2), F32)
    f[..., 0], f[..., 1] = d[0], d[1]
    for r in (1, 2):
        assert np.array_equal(_bits(M.median(f, r)), _bits(f))


@pytest.mark.parametrize("shape", [(1, 1), (2, 3), (4, 1)], ids=str)
@pytest.mark.parametrize("r", [1, 2])
def test_fields_smaller_than_the_window(shape, r):
    w, h = shape
    rng = np.random.default_rng(w + 10 * h + r)
    f = rng.uniform(-5, 5, (h, w, 2)).astype(F32)
    got = M.median(f, r)
    assert got.shape == f.shape
    for y in range(h):
        for x in range(w):
            for c in (0, 1):
                vals = sorted(float(f[min(max(y + j, 0), h - 1), min(max(x + i, 0), w - 1), c]) for j in range(-r, r + 1) for i in range(-r, r + 1))
                assert got[y, x, c] == F32(vals[len(vals) // 2]), (x, y, c)
    if shape == (1, 1):
        assert np.array_equal(_bits(got), _bits(f))


@pytest.mark.parametrize("kind", M.M_KINDS)
def test_the_shared_fields_against_a_per_pixel_loop(kind):
    """median() on the fields the GPU tests use, against the definition spelled out pixel by pixel (on a small shape)"""
    w, h = 5, 4
    f = M.field_case(kind, w, h)
    s = np.array(f, F32)
    s[~np.isfinite(s).all(axis=2)] = 0
    for r in (1, 2):
        got = M.median(f, r)
        for y in range(h):
            for x in range(w):
                for c in (0, 1):
                    vals = sorted(float(s[min(max(y + j, 0), h - 1), min(max(x + i, 0), w - 1), c]) for j in range(-r, r + 1) for i in range(-r, r + 1))
                    m = F32(vals[len(vals) // 2])
                    assert got[y, x, c] == m and not (m == 0 and np.signbit(got[y, x, c])), (kind, r, x, y, c)


# ---- the quality bars, on the oracle ----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _orc():
    from oracle import Oracle

    return Oracle()


@functools.lru_cache(maxsize=None)
def _scores(name, seed, r):
    """(score, seam-band score) of the scene's level-0 displacement; r = 0: no median"""
    prev, nxt, truth = D.scene(name, seed)
    disp = M.dense_displacement_median(_orc(), prev, nxt, D.S_LEVELS, D.S_WIN, D.S_ITERS, D.S_MIN_DET, None, r)
    out = D.score(disp, truth), M.seam_score(disp, truth)
    print(f"scene {name} seed {seed} median {r}: score {out[0]:.3f}, seam band {out[1]:.3f}")
    return out


@pytest.mark.parametrize("seed", D.S_SEEDS)
@pytest.mark.parametrize("name,bar", [("pan", 0.95), ("split", 0.97), ("split2", 0.97), ("small", 0.99)])
def test_the_5x5_median_meets_its_bars(name, bar, seed):
    assert _scores(name, seed, 2)[0] >= bar, (name, seed)


@pytest.mark.parametrize("seed", D.S_SEEDS)
def test_the_3x3_median_on_the_pan(seed):
    assert _scores("pan", seed, 1)[0] >= 0.93, seed


@pytest.mark.parametrize("seed", D.S_SEEDS)
@pytest.mark.parametrize("name", list(D.SCENES))
@pytest.mark.parametrize("r", [1, 2])
def test_a_median_never_scores_below_no_median(name, seed, r):
    assert _scores(name, seed, r)[0] >= _scores(name, seed, 0)[0], (name, seed, r)


@pytest.mark.parametrize("seed", D.S_SEEDS)
@pytest.mark.parametrize("name", ["split", "split2"])
def test_the_seam_band_gains_too(name, seed):
    assert _scores(name, seed, 2)[1] > _scores(name, seed, 0)[1], (name, seed)


@functools.lru_cache(maxsize=None)
def _ratios(step, levels, r):
    frames = IR.quality_clip(step)
    out = D.interp_ratios(frames, lambda i, j: M.dense_displacement_median(_orc(), frames[i], frames[j], levels, IR.Q_WIN, 3, D.S_MIN_DET, None, r))
    print(f"step {step}, {levels} levels, median {r}: SAD(interp) / SAD(cross-fade) {min(out):.3f} .. {max(out):.3f}")
    return out


@pytest.mark.parametrize("step,levels", [((1.0, 0.5), 3), ((2.0, 1.0), 3), ((3.0, -1.5), 4)], ids=str)
def test_in_between_frames_gain(step, levels):
    with_median, without = _ratios(step, levels, 2), _ratios(step, levels, 0)
    assert max(with_median) < max(without), (step, with_median, without)
