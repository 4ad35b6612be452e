"""CPU: the referee of the sampled output stage (tests/sampled_ref.py) on hand-computed miniatures, and the seeded generator of
synthetic flow pyramids the GPU tests use -- asserted here, under the referee alone, to reach every branch of the contract."""
import numpy as np
import pytest

import sampled_ref as R

F32 = np.float32
NAN, INF = np.nan, np.inf


def field(h, w, fill=(0.0, 0.0)):
    C = np.zeros((h, w, 2), F32)
    C[...] = fill
    return C


def test_compose_is_the_oracles(oracle):
    for case in [(64, 48, 4, 0), (64, 48, 4, 1), (1000, 568, 4, 0), (40, 24, 1, 0)]:
        W, H, L, lv = case
        pyr = R.synth_pyramid(W, H, L, lv, 5, 3.0)
        filled = [p if p is not None else np.zeros((H >> k, W >> k, 2), F32) for k, p in enumerate(pyr)]
        got, want = R.compose(pyr, L, lv), oracle.compose_flow(filled, L, lv)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        assert np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32)), case


def test_compose_by_hand():
    # two levels, level 0 is 4 x 2: C = (float)((double)(float)(2 * coarse) + fine)
    coarse = np.array([[[1.5, -2.0], [0.25, 8.0]]], F32)                       # 1 x 2
    fine = np.arange(16, dtype=F32).reshape(2, 4, 2) / 8
    C = R.compose([fine, coarse], 2, 0)
    assert C.shape == (2, 4, 2)
    assert C[0, 0].tolist() == [3.0 + 0.0, -4.0 + 0.125]
    assert C[1, 3].tolist() == [0.5 + 14 / 8, 16.0 + 15 / 8]
    # the rounding order: 2^24 + 1 is not a float; the coarse term is rounded to float BEFORE the fine one is added
    big = R.compose([np.array([[[1.0, 0.0]]], F32), np.array([[[2.0 ** 23 + 0.5, 0.0]]], F32)], 2, 0)
    assert big[0, 0, 0] == F32(2.0 ** 24)


def test_arrows_by_hand():
    # 8 x 6 level, arrow_res 4 -> offset 2, grid 3 x 4
    C = field(6, 8)
    C[0, 0] = (5.0, 0.25)        # u clamps to +2
    C[0, 2] = (-7.5, -3.0)       # u clamps to -2: x1 = 0; v clamps to -2: y1 = (int)(-2 + 0) < 0 -> not drawn
    C[2, 0] = (-0.75, 1.0)       # x1 = (int)(-0.75) = 0: truncation toward zero, drawn
    C[2, 2] = (1.5, -2.5)        # v + i = -2 + 2 = 0
    C[0, 4] = (-1.0, 0.0)        # x1 = 3
    C[0, 6] = (0.0, -0.5)        # v + i = -0.5 -> 0, drawn
    C[4, 0] = (-1.0, 0.0)        # x1 = -1 -> not drawn
    C[4, 2] = (NAN, 0.0)
    C[4, 4] = (INF, -INF)        # clamps: (2, -2)
    C[4, 6] = (0.0, NAN)
    C[1, 1] = (99.0, 99.0)       # off the grid: never read
    A = R.arrows(C, 4)
    assert A.shape == (3, 4, 4) and A.dtype == np.int32
    assert A[0].tolist() == [[0, 0, 2, 0], [2, 0, -1, -1], [4, 0, 3, 0], [6, 0, 6, 0]]
    assert A[1].tolist() == [[0, 2, 0, 3], [2, 2, 3, 0], [4, 2, 4, 2], [6, 2, 6, 2]]
    assert A[2].tolist() == [[0, 4, -1, -1], [2, 4, -1, -1], [4, 4, 6, 2], [6, 4, -1, -1]]
    cu, cv = R.clamp_masks(C, 4)
    assert cu.sum() == 3 and cv.sum() == 3


def test_arrows_skipped_for_y_alone_and_a_partial_last_row_and_column():
    # 7 x 5 level, arrow_res 2 -> offset 3: rows 0, 3 and columns 0, 3, 6 (h % offset = 2, w % offset = 1)
    C = field(5, 7)
    C[0, 3] = (1.0, -1.0)        # y1 = -1 alone -> not drawn
    C[3, 6] = (0.5, 1.75)        # the partial column and row: (6, 3) -> (6, 4)
    A = R.arrows(C, 2)
    assert A.shape == (2, 3, 4)
    assert A[0].tolist() == [[0, 0, 0, 0], [3, 0, -1, -1], [6, 0, 6, 0]]
    assert A[1].tolist() == [[0, 3, 0, 3], [3, 3, 3, 3], [6, 3, 6, 4]]
    with pytest.raises(AssertionError):
        R.arrows(C, 8)           # offset 0: the reference would loop forever


def test_tracks_by_hand():
    C1 = field(4, 6, (1.0, 0.5))
    C1[1, 2] = (NAN, 0.0)
    C1[3, 5] = (0.5, 0.75)
    C1[0, 0] = (-0.5, 0.0)
    C1[2, 0] = (0.0, -2.5)
    C1[1, 4] = (INF, 0.0)
    pts = np.array([[1.25, 1.5],    # moves to (2.25, 2.0)
                    [2.5, 1.875],   # NaN flow: lost at pair 1, position kept
                    [5.5, 3.5],     # moves out to the right and below: (6.0, 4.25), lost at pair 2
                    [0.0, 0.25],    # moves out to the left: (-0.5, 0.25)
                    [0.5, 2.0],     # moves out above: (0.5, -0.5)
                    [4.0, 1.0],     # Inf flow: lost, position kept
                    [6.0, 1.0],     # starts outside (x == w)
                    [NAN, 1.0],     # starts as no number
                    [3.0, 3.0]], F32)    # frozen before: status 7 stays, position stays
    st = np.zeros(9, np.int32)
    st[8] = 7
    p1, s1 = R.advect(C1, pts, st, 1)
    assert p1[:7].tolist() == [[2.25, 2.0], [2.5, 1.875], [6.0, 4.25], [-0.5, 0.25], [0.5, -0.5], [4.0, 1.0], [6.0, 1.0]]
    assert np.isnan(p1[7, 0]) and p1[8].tolist() == [3.0, 3.0]
    assert s1.tolist() == [0, 1, 0, 0, 0, 1, 1, 1, 7]
    C2 = field(4, 6, (0.0, 1.0))
    p2, s2 = R.advect(C2, p1, s1, 2)
    assert s2.tolist() == [0, 1, 2, 2, 2, 1, 1, 1, 7]
    assert p2[0].tolist() == [2.25, 3.0]
    assert np.array_equal(p2[1:7], p1[1:7]) and p2[8].tolist() == [3.0, 3.0]          # lost and frozen points stay
    p3, s3 = R.advect(C2, p2, s2, 3)
    assert p3[0].tolist() == [2.25, 4.0] and s3[0] == 0                                # left below, noticed at the next pair
    _, s4 = R.advect(C2, p3, s3, 4)
    assert s4.tolist() == [4, 1, 2, 2, 2, 1, 1, 1, 7]
    # track(): the same, with the history and its ring
    pe, se, hist = R.track([C1, C2, C2, C2], pts, st)
    assert np.array_equal(se, s4) and len(hist) == 4
    assert np.array_equal(hist[0].view(np.uint32), p1.view(np.uint32)) and np.array_equal(hist[2].view(np.uint32), p3.view(np.uint32))
    _, _, ring = R.track([C1, C2, C2, C2], pts, st, n_slots=3)
    assert np.array_equal(ring[0].view(np.uint32), hist[3].view(np.uint32)) and np.array_equal(ring[1].view(np.uint32), p2.view(np.uint32))


@pytest.mark.parametrize("arrow_res", R.ARROW_RES, ids=str)
@pytest.mark.parametrize("case", R.STATELESS_CASES, ids=lambda c: "x".join(map(str, c)))
def test_generated_arrow_cases_reach_every_branch(case, arrow_res):
    W, H, L, lv = case
    pyr, res, w, h = R.arrow_case(case, arrow_res)
    assert all(pyr[k].shape == (H >> k, W >> k, 2) for k in range(lv, L))
    C = R.compose(pyr, L, lv)
    A = R.arrows(C, res)
    cu, cv = R.clamp_masks(C, res)
    n = A.shape[0] * A.shape[1]
    undrawn = int((A[..., 2] < 0).sum())
    print(f"{case} arrow_res {res}: {n} arrows, clamped u {cu.mean():.3f} v {cv.mean():.3f}, undrawn {undrawn / n:.3f}")
    assert 0.10 <= cu.mean() <= 0.90 and 0.10 <= cv.mean() <= 0.90
    assert undrawn >= 0.01 * n
    assert np.array_equal(A[..., 2] < 0, A[..., 3] < 0)
    g = C[::w // res, ::w // res]
    assert np.isnan(g).any() and np.isposinf(g).any() and np.isneginf(g).any()


@pytest.mark.parametrize("n_points", [1000, 1 << 21])
@pytest.mark.parametrize("case", R.STATELESS_CASES, ids=lambda c: "x".join(map(str, c)))
def test_generated_track_cases_reach_every_branch(case, n_points):
    W, H, L, lv = case
    pyrs, pts, w, h = R.track_case(case, n_points)
    fields = [R.compose(p, L, lv) for p in pyrs]
    _, st, hist = R.track(fields, pts)
    lost, alive = (st != 0).mean(), (st == 0).mean()
    print(f"{case} n {n_points}: lost {lost:.3f}, alive {alive:.3f}, by pair {np.bincount(st, minlength=R.TRACK_PAIRS + 1).tolist()}")
    assert lost >= 0.05 and alive >= 0.50
    assert set(np.unique(st)) == set(range(R.TRACK_PAIRS + 1))       # some lost at every pair
    moved = ~np.all(hist[-1].view(np.uint32) == pts.view(np.uint32), axis=1)
    assert moved[st == 0].all() or moved[st == 0].mean() > 0.99
