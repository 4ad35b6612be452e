"""CPU: pins the referee of the pixel displacement and of frame interpolation (tests/interp_ref.py) -- against translations, whose
in-between frame is known exactly, against its own symmetry, against motion_ref (the displacement IS what shift-then-warp
applies), and on the oracle's flows: an in-between frame built from the displacement is closer to the true frame than a
cross-fade.  No GPU."""
import functools

import numpy as np
import pytest

import interp_ref as R
import motion_ref as M

F32 = np.float32


# ---- translations ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [(4, 2), (-6, 2), (2, -8), (0, 4), (-2, 0), (0, 0)], ids=str)
def test_a_translation_gives_the_half_way_frame_exactly(d):
    """b = a rolled by d (even components), Dab = d, Dba = -d, t = 0.5: Ta = -d/2 and Tb = +d/2 exactly.  Wherever a side is usable
    it reads a rolled by d/2 at a whole pixel, so classes 0, 1 and 2 all give that image exactly; side a is usable on
    (w - |dx/2|)(h - |dy/2|) pixels, so is side b, both on (w - |dx|)(h - |dy|), neither on the two corners of |dx/2| x |dy/2|."""
    w, h = 67, 33
    a = R.planes(w, h)[0]
    dx, dy = d
    b = np.roll(a, (dy, dx), axis=(0, 1))
    dab = np.broadcast_to(np.array([dx, dy], F32), (h, w, 2))
    out, stats, cls = R.interpolate(a, b, dab, -dab, 0.5)
    want = np.roll(a, (dy // 2, dx // 2), axis=(0, 1))
    assert np.array_equal(out[cls != 3], want[cls != 3])
    hx, hy = abs(dx) // 2, abs(dy) // 2
    xs, ys = np.arange(w)[None, :], np.arange(h)[:, None]
    ua = (xs - dx // 2 >= 0) & (xs - dx // 2 <= w - 1) & (ys - dy // 2 >= 0) & (ys - dy // 2 <= h - 1)
    ub = (xs + dx // 2 >= 0) & (xs + dx // 2 <= w - 1) & (ys + dy // 2 >= 0) & (ys + dy // 2 <= h - 1)
    assert np.array_equal(cls, np.where(ua & ub, 0, np.where(ua, 1, np.where(ub, 2, 3))))
    both, one = (w - 2 * hx) * (h - 2 * hy), (w - hx) * (h - hy)
    assert stats.tolist() == [w * h, one - both, one - both, 2 * hx * hy]
    assert (cls[2 * hy:h - 2 * hy, 2 * hx:w - 2 * hx] == 0).all()      # the interior


def test_a_fractional_translation_is_exact_for_the_positions():
    """t = 0.25, d = (8, -4), Dab = d, Dba = -d: c00 = -3/16, c01 = 1/16, c10 = 9/16, so Ta = -(3/16) d - (1/16) d = -d/4 and
    Tb = (9/16) d + (3/16) d = 3d/4, both whole pixels: every usable side reads a moved by d/4"""
    w, h = 67, 33
    a = R.planes(w, h)[0]
    d = np.array([8, -4], F32)
    b = np.roll(a, (-4, 8), axis=(0, 1))
    dab = np.broadcast_to(d, (h, w, 2))
    out, stats, cls = R.interpolate(a, b, dab, -dab, 0.25)
    want = np.roll(a, (-1, 2), axis=(0, 1))                             # a moved by d / 4
    assert np.array_equal(out[cls != 3], want[cls != 3]) and stats[0] == w * h


# ---- symmetry -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", R.LARGE, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", R.KINDS)
def test_swapping_the_frames_at_half_time(kind, size):
    w, h = size
    a, b = R.planes(w, h)
    dab, dba = R.field_case(kind, w, h)
    o1, s1, c1 = R.interpolate(a, b, dab, dba, 0.5)
    o2, s2, c2 = R.interpolate(b, a, dba, dab, 0.5)
    assert np.array_equal(c2, np.array([0, 2, 1, 3], np.uint8)[c1])
    assert s2.tolist() == [s1[0], s1[2], s1[1], s1[3]]
    assert np.abs(o1.astype(int) - o2.astype(int)).max() <= 1


# ---- the shared inputs do what they are for -------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", R.LARGE, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_shared_fields_reach_every_class_and_the_last_column_and_row(size):
    w, h = size
    for ts in range(len(R.TIME_SETS)):
        st = R.reference("borders", w, h, ts)[1]
        assert (st[:, 1:] > 0).all(), (ts, st.tolist())                 # classes 1, 2 and 3 at every time
        assert (st[:, 0] == w * h).all() and (st[:, 1:].sum(axis=1) < w * h).all()
        assert (R.reference("nonfinite", w, h, ts)[1][:, 3] > 0).all()
    dab, dba = R.field_case("edge", w, h)
    xs, ys = np.arange(w, dtype=F32)[None, :], np.arange(h, dtype=F32)[:, None]
    pax, pay = xs - F32(0.25) * dab[..., 0] + F32(0.25) * dba[..., 0], ys - F32(0.25) * dab[..., 1] + F32(0.25) * dba[..., 1]
    pbx, pby = xs + F32(0.25) * dab[..., 0] - F32(0.25) * dba[..., 0], ys + F32(0.25) * dab[..., 1] - F32(0.25) * dba[..., 1]
    for p, last in ((pax, w - 1), (pbx, w - 1), (pay, h - 1), (pby, h - 1)):
        assert np.count_nonzero(p == last) > h       # exactly on it


def test_the_host_step():
    for t in (0.5, 0.25, F32(1 / 9), F32(8 / 9)):
        tt, c00, c01, c10 = R.coefficients(t)
        assert all(isinstance(v, np.float32) for v in (tt, c00, c01, c10))
        omt = F32(F32(1) - F32(t))
        assert c00 == -F32(omt * F32(t)) and c01 == F32(F32(t) * F32(t)) and c10 == F32(omt * omt)
    assert R.coefficients(0.5)[1:] == (F32(-0.25), F32(0.25), F32(0.25))


# ---- the displacement is what shift-then-warp applies ---------------------------------------------------------------------------

@pytest.mark.parametrize("uv", [(0.0, 0.0), (3.0, -2.0), (3.7, -2.2), (-0.5, -0.5), (-4.25, 1.5), None], ids=str)
@pytest.mark.parametrize("size", R.LARGE, ids=lambda s: f"{s[0]}x{s[1]}")
def test_displacement_against_motion_ref(size, uv):
    """Whole-pixel flows at scale 1: motion_ref.warp(motion_ref.shift(next, uv), flow, 1) reads next at (y + D.y, x + D.x) wherever
    that index, and the shift's own (x + flow.x, y + flow.y, where the warp reads the shifted plane), is inside the image."""
    w, h = size
    nxt = R.planes(w, h)[1]
    flow = np.random.default_rng(w + h).integers(-3, 4, (h, w, 2)).astype(F32)
    D = R.displacement(flow, uv, 1.0)
    fl = (0.0, 0.0) if uv is None else (np.floor(uv[0]), np.floor(uv[1]))
    assert np.array_equal(D[..., 0], fl[0] + flow[..., 0]) and np.array_equal(D[..., 1], fl[1] + flow[..., 1])
    mc, bad = M.warp(M.shift(nxt, uv), flow, 1.0)
    assert not bad.any()
    xs, ys = np.arange(w)[None, :], np.arange(h)[:, None]
    wx, wy = xs + flow[..., 0].astype(int), ys + flow[..., 1].astype(int)        # where the warp reads the shifted plane
    sx, sy = xs + D[..., 0].astype(int), ys + D[..., 1].astype(int)              # where that pixel of the shifted plane came from
    ok = (wx >= 0) & (wx < w) & (wy >= 0) & (wy < h) & (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
    assert ok.sum() > 0.4 * w * h
    assert np.array_equal(mc[ok], nxt[sy[ok], sx[ok]])


def test_displacement_passes_everything_through():
    flow = R.flow_case("nonfinite", 67, 33)
    for uv in R.UV_CASES:
        D = R.displacement(flow, uv, R.ITER_SCALE)
        assert D.dtype == F32 and D.shape == flow.shape
        if uv is not None and np.isnan(uv[0]):
            assert np.isnan(D[..., 0]).all() and not np.isnan(D[..., 1][np.isfinite(flow[..., 1])]).any()
    D = R.displacement(flow, None, R.ITER_SCALE)
    assert np.array_equal(np.isnan(D), np.isnan(flow))
    z = R.displacement(np.full((1, 1, 2), -0.0, F32), None, 1.0)      # the add of 0.0f is performed: -0 becomes +0
    assert not np.signbit(z).any()


# ---- quality on the oracle ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _oracle_displacements(step, iters):
    """level-0 pixel displacement of (a -> b) for the clip's pairs, both directions, from the oracle's iterated LK (as
    Oracle.flow_pair_iter runs it: the level-0 flow and the shift accumulated from the coarser levels' first-iteration flows)"""
    from oracle import Oracle

    orc = Oracle()
    frames = R.quality_clip(step)
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
def test_interpolating_with_the_displacement_beats_a_cross_fade(step, iters):
    frames = R.quality_clip(step)
    D = _oracle_displacements(step, iters)
    ratios = []
    for i, j in ((0, 4), (4, 8)):
        med = np.median(D[i, j].reshape(-1, 2), axis=0)
        print(f"step {step} iters {iters} pair ({i}, {j}): median displacement {med.tolist()} (true {[4 * step[0], 4 * step[1]]})")
        for k in (1, 2, 3):
            t = F32(k / 4)
            got = R.interpolate(frames[i], frames[j], D[i, j], D[j, i], t)[0]
            s_int, s_fade = R.sad(got, frames[i + k]), R.sad(R.cross_fade(frames[i], frames[j], t), frames[i + k])
            ratios.append(s_int / s_fade)
            assert s_int < s_fade, (step, iters, i, j, k, s_int, s_fade)
    print(f"step {step} iters {iters}: SAD(interp) / SAD(cross-fade) = {min(ratios):.2f} .. {max(ratios):.2f}")
