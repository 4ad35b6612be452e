"""CPU: the referee of the forward-backward check (tests/consistency_ref.py) -- its shared inputs reach every class, its tap
geometry and blend are those of the oracle-pinned warp (motion_ref.warp), and it counts what can be counted by hand."""
import numpy as np
import pytest

import consistency_ref as R
import motion_ref as M

F32 = np.float32


def _share(mask, c):
    return np.count_nonzero(mask == c) / mask.size


@pytest.mark.parametrize("size", R.LARGE, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_shared_inputs_cover_every_class(size):
    """So that the GPU comparison cannot pass on a near-empty class.  (A seed that misses these is changed, not the bounds.)"""
    w, h = size
    mask = R.reference("inverse", w, h, 0)[0]
    assert _share(mask, 0) >= 0.50 and _share(mask, 1) >= 0.10, (_share(mask, 0), _share(mask, 1))
    assert _share(R.reference("borders", w, h, 0)[0], 2) >= 0.30
    assert _share(R.reference("nonfinite", w, h, 0)[0], 3) >= 0.10
    fwd, bwd, scale = R.field_case("edge", w, h)
    mask, _, _, parts = R.consistency(fwd, bwd, scale, *R.tolerances(scale)[0], parts=True)
    assert np.count_nonzero((parts["px"] == F32(w - 1)) & (mask <= 1)) >= 1, "no pixel targets column w - 1 exactly and gets through"
    assert np.count_nonzero((parts["py"] == F32(h - 1)) & (mask <= 1)) >= 1, "no pixel targets row h - 1 exactly and gets through"
    # the trap itself: such a pixel sits next to the NaN of column 0 of the next row in memory, and its error is finite
    assert np.isnan(bwd[:, 0]).all()


@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("scale", [R.ITER_SCALE, F32(1.0)])
def test_tap_geometry_is_the_pinned_warps(size, scale):
    """bwd's u component holds the integers of a u8 plane: at every pixel of class <= 1 the blend, rounded as the warp rounds,
    is the warp's byte."""
    w, h = size
    rng = np.random.default_rng(5 * w + h)
    plane = rng.integers(0, 256, (h, w), dtype=np.uint8)
    fwd = (rng.uniform(-6.0, 6.0, (h, w, 2)) / float(scale)).astype(F32)
    fwd[::2, ::3] = 0                                       # (the degenerate sizes: something has to stay inside)
    bwd = np.stack([plane.astype(F32), np.zeros((h, w), F32)], axis=-1)
    mask, _, _, parts = R.consistency(fwd, bwd, scale, 0.01, 0.5, parts=True)
    inside = mask <= 1
    assert inside.any()
    got = (parts["ru"] + F32(0.5)).astype(F32)[inside].astype(np.int64)
    want, not_warped = M.warp(plane, fwd, scale)
    assert not not_warped[inside].any()
    assert np.array_equal(got, want[inside].astype(np.int64))


@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("ab", [(2, 1), (-3, 0), (0, -2), (-1, -4), (0, 0), (300, 0)])
def test_integer_translation_and_its_swap(size, ab):
    w, h = size
    a, b = ab
    fwd = np.broadcast_to(np.array([a, b], F32), (h, w, 2))
    bwd = np.broadcast_to(np.array([-a, -b], F32), (h, w, 2))
    left = w * h - max(w - abs(a), 0) * max(h - abs(b), 0)
    for alpha, beta in ((0.01, 0.5), (0.0, 0.0)):
        mask, err, stats = R.consistency(fwd, bwd, 1.0, alpha, beta)
        assert stats.tolist() == [w * h, 0, left, 0]
        assert (err[mask == 0] == 0).all()
        # the other direction: the same call with the fields swapped gives the mirrored mask
        mask_b, _, stats_b = R.consistency(bwd, fwd, 1.0, alpha, beta)
        assert stats_b.tolist() == [w * h, 0, left, 0]
        assert np.array_equal(mask_b, mask[::-1, ::-1])


def test_err_is_never_nan_and_infinite_exactly_on_classes_2_and_3():
    n = 0
    for w, h in R.SIZES:
        for kind in R.KINDS:
            for ti in (0, 1):
                mask, err, stats = R.reference(kind, w, h, ti)
                assert not np.isnan(err).any()
                assert np.array_equal(err.view(np.uint32) == 0x7F800000, mask >= 2), (kind, w, h)
                assert np.isfinite(err[mask <= 1]).all()
                assert stats[0] == w * h and stats[1:].sum() + np.count_nonzero(mask == 0) == w * h
                n += 1
    assert n == 50
