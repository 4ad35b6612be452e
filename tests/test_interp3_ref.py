"""CPU: pins the referee of colour frame interpolation (tests/interp3_ref.py) -- equal channels, permuted channels, stats that do
not look at the planes -- and runs the quality experiment of tests/test_interp_ref.py in colour on the oracle's flows: every channel
of every in-between frame is closer to the true frame than a cross-fade.  No GPU."""
import functools

import numpy as np
import pytest

import interp3_ref as R3
import interp_ref as R

F32 = np.float32


@pytest.mark.parametrize("kind", R.KINDS)
def test_equal_channels_give_equal_channels_each_the_grey_result(kind):
    w, h = 67, 33
    a, b = R.planes(w, h)
    dab, dba = R.field_case(kind, w, h)
    a3, b3 = np.repeat(a[:, :, None], 3, 2), np.repeat(b[:, :, None], 3, 2)
    for t in R.TIME_SETS[1]:
        out, stats, cls = R3.interpolate3(a3, b3, dab, dba, t)
        want = R.interpolate(a, b, dab, dba, t)
        assert out.shape == (h, w, 3) and out.dtype == np.uint8
        for c in range(3):
            assert np.array_equal(out[..., c], want[0])
        assert np.array_equal(stats, want[1]) and np.array_equal(cls, want[2])


@pytest.mark.parametrize("perm", [(2, 1, 0), (1, 2, 0), (0, 2, 1)], ids=str)
def test_permuting_the_input_channels_permutes_the_output(perm):
    w, h = 130, 9
    a, b = R3.planes3(w, h)
    dab, dba = R.field_case("borders", w, h)
    out, stats, _ = R3.interpolate3(a, b, dab, dba, 0.25)
    out_p, stats_p, _ = R3.interpolate3(a[..., perm], b[..., perm], dab, dba, 0.25)
    assert np.array_equal(out_p, out[..., perm]) and np.array_equal(stats_p, stats)
    assert not np.array_equal(out[..., 0], out[..., 1])      # (the channels do differ)


@pytest.mark.parametrize("kind", ["borders", "nonfinite"])
def test_the_stats_do_not_depend_on_the_planes(kind):
    w, h = 67, 33
    dab, dba = R.field_case(kind, w, h)
    for ts in range(len(R.TIME_SETS)):
        st = R3.reference3(kind, w, h, ts)[1]
        other = R3.interpolate3_times(*R3.planes3(w, h, 5), dab, dba, R.TIME_SETS[ts])[1]
        assert np.array_equal(st, other) and np.array_equal(st, R.reference(kind, w, h, ts)[1])
        assert (st[:, 0] == w * h).all()                      # pixels, not bytes


def test_the_shared_inputs():
    a, b = R3.planes3(67, 33)
    assert a.shape == (33, 67, 3) and a.dtype == np.uint8 and not np.array_equal(a, b)
    assert not np.array_equal(a[..., 0], a[..., 1]) and not np.array_equal(a[..., 1], a[..., 2])
    img = np.array([[[1, 2, 4], [255, 255, 254], [0, 0, 2]]], np.uint8)
    assert R3.grey(img).tolist() == [[2, 254, 0]] and R3.grey(img).dtype == np.uint8
    clip = R3.colour_quality_clip(R.Q_STEPS[0])
    assert len(clip) == 9 and clip[0].shape == (R.Q_H, R.Q_W, 3)
    assert np.array_equal(clip[4][..., 0], R.quality_clip(R.Q_STEPS[0])[4])      # channel 0 is the grey experiment's texture


# ---- quality on the oracle ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _oracle_displacements(step, iters):
    """test_interp_ref._oracle_displacements' recipe on the grey average of the colour clip: the level-0 pixel displacement of the
    clip's pairs, both directions, from the oracle's iterated LK"""
    from oracle import Oracle

    orc = Oracle()
    frames = [R3.grey(f) for f in R3.colour_quality_clip(step)]
    L = R.Q_LEVELS

    def disp(prev1, next1):
        pp = orc.gauss_pyramid(np.repeat(prev1[:, :, None], 3, 2), L)
        npyr = orc.gauss_pyramid(np.repeat(next1[:, :, None], 3, 2), L)
        first = [np.zeros((R.Q_H >> k, R.Q_W >> k, 2), F32) for k in range(L)]
        out = [None] * L
        for k in range(L - 1, -1, -1):
            nxt3 = npyr[k] if k == L - 1 else orc.shift_back_pyramid(npyr[k], k, L, first)
            out[k], first[k] = orc.lk_iter_level(pp[k][:, :, 0], nxt3[:, :, 0], R.Q_WIN, iters)
        u = v = F32(0)                                                   # the shift of level 0 (shift_back_pyramid's accumulation)
        for k in range(L - 1, 0, -1):
            u, v = F32(u + F32(F32(1 << k) * first[k][0, 0, 0])), F32(v + F32(F32(1 << k) * first[k][0, 0, 1]))
        return R.displacement(out[0], (u, v), R.ITER_SCALE)

    return {(i, j): disp(frames[i], frames[j]) for i, j in ((0, 4), (4, 0), (4, 8), (8, 4))}


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("step", R.Q_STEPS, ids=str)
def test_interpolating_every_channel_beats_a_cross_fade(step, iters):
    """Measured here on the reference alone, SAD(interp) / SAD(cross-fade) over two pairs x three times x three channels:
    step (0.6, -0.3): iters 1 0.26 .. 0.46, iters 3 0.29 .. 0.49; step (1.0, 0.5): iters 1 0.21 .. 0.80, iters 3 0.18 .. 0.51."""
    frames = R3.colour_quality_clip(step)
    D = _oracle_displacements(step, iters)
    ratios = []
    for i, j in ((0, 4), (4, 8)):
        for k in (1, 2, 3):
            t = F32(k / 4)
            got = R3.interpolate3(frames[i], frames[j], D[i, j], D[j, i], t)[0]
            for c in range(3):
                truth = frames[i + k][..., c]
                s_int = R.sad(got[..., c], truth)
                s_fade = R.sad(R.cross_fade(frames[i][..., c], frames[j][..., c], t), truth)
                ratios.append(s_int / s_fade)
    print(f"step {step} iters {iters}: SAD(interp) / SAD(cross-fade) per channel = {min(ratios):.2f} .. {max(ratios):.2f}")
    assert len(ratios) == 18 and max(ratios) < 1.0, ratios
