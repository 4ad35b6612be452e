"""CPU: tests/motion_ref.py, the NumPy restatement of "motion compensation" (include/ofx.h), is pinned against the oracle on the
very inputs the GPU test runs -- its shift against oracle.shift_back_pyramid (channel 0, zero destination), its warp against
oracle.warp_bilinear_u8, both exactly -- and gives the known answers of two cases worked by hand."""
import numpy as np

import motion_ref as R

F32 = np.float32


def _oracle_shift(oracle, next1, uv):
    u, v = (F32(0), F32(0)) if uv is None else (F32(uv[0]), F32(uv[1]))
    with np.errstate(over="ignore", invalid="ignore"):
        half = np.array([u / F32(2), v / F32(2)], F32)    # the oracle forms u = 0 + 2 * flow_1[0]: exact
    src3 = np.repeat(np.asarray(next1, np.uint8)[..., None], 3, axis=2)
    return oracle.shift_back_pyramid(src3, 0, 2, [None, half])[..., 0]


def test_shift_and_warp_equal_the_oracle_on_the_shared_inputs(oracle):
    n = 0
    for name, w, h, prev1, next1, flow, uv, scale in R.stateless_cases():
        sh = R.shift(next1, uv)
        assert np.array_equal(sh, _oracle_shift(oracle, next1, uv)), f"{name}: shift"
        mc, bad = R.warp(sh, flow, scale)
        assert np.array_equal(mc, oracle.warp_bilinear_u8(sh, flow, scale)), f"{name}: warp"
        # not warped <=> the oracle's own test on the coordinates
        with np.errstate(invalid="ignore", over="ignore"):
            sx = (np.arange(w, dtype=F32)[None, :] + (F32(scale) * flow[..., 0]).astype(F32)).astype(F32)
            sy = (np.arange(h, dtype=F32)[:, None] + (F32(scale) * flow[..., 1]).astype(F32)).astype(F32)
            want_bad = ~((np.abs(sx) <= F32(1e9)) & (np.abs(sy) <= F32(1e9)))
        assert np.array_equal(bad, want_bad), f"{name}: not-warped mask"
        n += 1
    assert n == len(R.SIZES) * 8 * len(R.FLOW_KINDS)


def test_the_shared_inputs_reach_the_edge_cases():
    seen_out, seen_collapse, seen_bad, seen_third = False, False, False, False
    for name, w, h, prev1, next1, flow, uv, scale in R.stateless_cases():
        sh = R.shift(next1, uv)
        if uv is not None and uv[0] == w + 5:
            pos = np.arange(h)[:, None] * w + np.arange(w)[None, :]
            assert np.array_equal(sh, np.where(3 * pos < w * h, next1, 0)), f"{name}: everything out -> the one-third rule"
            seen_third = True
            seen_out = seen_out or (sh == 0).any()
        if uv == (-0.5, -0.5) and w > 1 and h > 1:
            assert np.array_equal(sh[0, :2], next1[0, [0, 0]]) and np.array_equal(sh[:2, 0], next1[[0, 0], 0]), f"{name}: the collapse at 0"
            seen_collapse = True
        seen_bad = seen_bad or R.warp(sh, flow, scale)[1].any()
    assert seen_out and seen_collapse and seen_bad and seen_third


def test_known_answers():
    for (w, h) in R.SIZES + [(64, 48)]:
        prev1, next1 = R.planes(w, h, 99)
        zero = np.zeros((h, w, 2), F32)
        for uv in (None, (0.0, 0.0)):
            mc, st = R.motion(prev1, next1, zero, uv, R.ITER_SCALE)
            assert np.array_equal(mc, next1)
            assert st[0] == w * h and st[2] == st[1] and st[3] == 0
            assert st[1] == np.abs(prev1.astype(np.int64) - next1.astype(np.int64)).sum()
        flow = np.empty((h, w, 2), F32)
        flow[..., 0], flow[..., 1] = 2.0, 1.0
        mc, st = R.motion(prev1, next1, flow, None, 1.0)
        ys, xs = np.minimum(np.arange(h) + 1, h - 1), np.minimum(np.arange(w) + 2, w - 1)
        assert np.array_equal(mc, next1[ys[:, None], xs[None, :]])
        assert st[3] == 0 and st[2] == np.abs(prev1.astype(np.int64) - mc.astype(np.int64)).sum()
    # a pair that IS a translation: the compensated image matches prev where the source is inside the image
    w, h = 40, 30
    _, base = R.planes(w + 2, h + 1, 5)
    prev1, next1 = base[:h, :w].copy(), np.zeros((h, w), np.uint8)
    next1[1:, 2:] = prev1[:-1, :-2]                       # next(y + 1, x + 2) = prev(y, x)
    flow = np.empty((h, w, 2), F32)
    flow[..., 0], flow[..., 1] = 2.0, 1.0
    mc, st = R.motion(prev1, next1, flow, None, 1.0)
    assert np.array_equal(mc[:-1, :-2], prev1[:-1, :-2]) and st[2] < st[1]
    # a flow that is not finite anywhere: nothing is warped, mc is the shifted image
    flow[...] = np.nan
    mc, st = R.motion(prev1, next1, flow, (3.7, -2.2), R.ITER_SCALE)
    assert np.array_equal(mc, R.shift(next1, (3.7, -2.2))) and st[3] == w * h
