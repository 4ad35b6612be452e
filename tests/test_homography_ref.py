"""CPU: the referee of ofx_fit_homography (tests/homography_ref.py) alone -- the sampler with K = 4 by hand, four exact matches of a
dyadic homography, FEW and DEGENERATE, the W <= 0 rules, ties and skipped refits, seeds and H, and its accuracy under outliers."""
import numpy as np
import pytest

import homography_cases as Cs
import homography_ref as R
from fit_motion_ref import FIT_DEGENERATE, FIT_FEW, FIT_OK, lattice, sample_index

f64 = np.float64
SIZE = (192, 128)


def test_the_sampler_with_four_samples_by_hand():
    n, seed = 37, 5
    ok = np.ones(n, bool)
    ok[::3] = False
    seen_retry = seen_repeat = False
    for j in range(200):
        idx, fail = [], False
        for k in range(4):
            tries = [sample_index(seed, j, k, a, n) for a in range(8)]
            take = [i for i in tries if ok[i] and i not in idx]
            seen_retry |= bool(take) and take[0] != tries[0]
            seen_repeat |= any(i in idx for i in tries[:tries.index(take[0])]) if take else False
            if not take:
                fail = True
                break
            idx.append(take[0])
        assert R.sample(seed, j, ok) == (None if fail else idx)
        assert fail or len(set(idx)) == 4
    assert seen_retry and seen_repeat, "the cases the rule is about occur"
    assert all(0 <= sample_index(seed, j, 3, 7, n) < n for j in range(200))
    # fewer than four usable matches can never fill a sample; an only match fails at the second sample
    few = np.zeros(n, bool)
    few[[1, 2, 3]] = True
    assert all(R.sample(seed, j, few) is None for j in range(50))


def test_the_scale_exponent():
    assert [R.scale_exponent(s) for s in ((1, 1), (2, 1), (2, 2), (3, 2), (257, 257), (258, 2), (640, 480), (1 << 16, 1))] == [0, 4, 4, 5, 12, 13, 14, 20]
    for size in ((97, 61), (640, 480), (1 << 16, 1 << 16)):
        e = R.scale_exponent(size)
        big = max(16 * (size[0] - 1), 16 * (size[1] - 1))
        assert (1 << e) >= big and (e == 0 or (1 << (e - 1)) < big)


def test_four_exact_matches_of_a_dyadic_homography_are_recovered():
    p, q, size = Cs.dyadic_four()
    u, v, ok = lattice(p, q, size)
    e = R.scale_exponent(size)
    assert e == 12 and ok.all()
    h = R.solve(R.system([tuple(R.normalised(t, e) for t in (u[i][0], u[i][1], v[i][0], v[i][1])) for i in range(4)]))
    assert np.abs(np.array(h) - Cs.DYADIC_MODEL).max() <= 1e-13
    for refits in (0, 1):
        m, info, mask = R.fit_homography(p, q, size, hypotheses=8, thr_q=1, refits=refits, seed=0)
        assert info[:2].tolist() == [FIT_OK, 4] and 1 <= info[2] <= 8 and info[3] >= 0 and info[4] == info[5] == 4 and info[6] == refits and mask.tolist() == [1] * 4
        assert np.abs(m - R.to_pixels(Cs.DYADIC_MODEL, size, e)).max() <= 1e-9 and m[8] == 1.0
        assert np.abs(R.apply(m, p) - q).max() <= 1e-9


def test_few_three_usable_matches():
    p, q = Cs.noisy_matches(40, SIZE, 1, 0.0)
    p[3:, 0] = np.nan
    m, info, mask = R.fit_homography(p, q, SIZE, hypotheses=16)
    assert int(lattice(p, q, SIZE)[2].sum()) == 3
    assert m.tolist() == list(R.IDENTITY) and info.tolist() == [FIT_FEW, 3, 0, -1, 0, 0, 0, 0] and not mask.any()


def row_matches(size, n=30):
    """every match on the row y = (h - 1) / 2 of an odd-height frame: uy = vy = 0"""
    w, h = size
    assert h % 2 == 1
    x = np.linspace(1, w - 2, n)
    p = np.stack([x, np.full(n, (h - 1) / 2)], axis=1).astype(np.float32)
    q = p.copy()
    q[:, 0] += 0.5
    return p, q


def test_degenerate_every_match_on_the_middle_row():
    size = (97, 61)
    p, q = row_matches(size)
    u, v, ok = lattice(p, q, size)
    assert ok.all() and not u[:, 1].any() and not v[:, 1].any()
    # column 1 of every system is zero, so the pivot of column 1 is exactly 0
    idx = R.sample(0, 0, ok)
    M = R.system([tuple(R.normalised(t, 11) for t in (u[i][0], u[i][1], v[i][0], v[i][1])) for i in idx])
    assert all(row[1] == 0 for row in M) and R.solve(M) is None
    m, info, mask = R.fit_homography(p, q, size, hypotheses=32)
    assert m.tolist() == list(R.IDENTITY) and info.tolist() == [FIT_DEGENERATE, 30, 0, -1, 0, 0, 0, 0] and not mask.any()


def bow_tie():
    """a square sent to a twisted quadrilateral: the homography through the four matches has W < 0 at some of them"""
    p = np.float32([[40, 30], [120, 30], [120, 90], [40, 90]])
    q = np.float32([[40, 30], [120, 30], [40, 90], [120, 90]])
    return p, q


def test_a_hypothesis_with_w_not_positive_at_a_sample_is_invalid():
    p, q = bow_tie()
    u, v, ok = lattice(p, q, SIZE)
    e = R.scale_exponent(SIZE)
    pts = [tuple(R.normalised(t, e) for t in (u[i][0], u[i][1], v[i][0], v[i][1])) for i in range(4)]
    h = R.solve(R.system(pts))
    assert h is not None, "the solve itself succeeds"
    ws = [(h[6] * x + h[7] * y) + f64(1.0) for x, y, _, _ in pts]
    assert min(ws) < 0 < max(ws)
    assert all(R.hypothesis(0, j, u, v, ok, e) is None for j in range(16))
    m, info, mask = R.fit_homography(p, q, SIZE, hypotheses=16)
    assert info.tolist() == [FIT_DEGENERATE, 4, 0, -1, 0, 0, 0, 0] and m.tolist() == list(R.IDENTITY)


def test_a_match_behind_the_horizon_is_no_inlier():
    """h = (1, 0, 0, 0, 1, 0, -2, 0) at e = 4: x = 1 has W = -1 and X = x / W = -1 leaves no residual; x = -1/2 has W = 2, X = -1/4"""
    h = [f64(t) for t in (1, 0, 0, 0, 1, 0, -2, 0)]
    u, v = np.array([[16, 0], [-8, 0], [8, 0]], np.int64), np.array([[-16, 0], [-4, 0], [0, 0]], np.int64)
    ok = np.ones(3, bool)
    assert R.inliers(h, u, v, ok, 0, 4).tolist() == [False, True, False]          # W = -1;  W = 2, exact;  W = 0 (x = 1/2)
    assert R.inliers(h, u, v, ok, 1 << 15, 4).tolist() == [False, True, False]
    assert R.inliers(h, u, v, np.array([True, False, True]), 0, 4).tolist() == [False, False, False]


def exact_pan(n=60, seed=0):
    """matches of a whole-lattice pan: every sample of four that is not singular gives (almost) the same model"""
    rng = np.random.RandomState(seed)
    p = (np.rint(np.stack([rng.uniform(10, 170, n), rng.uniform(10, 110, n)], axis=1) * 32) / 32).astype(np.float32)
    return p, p + np.float32([1.0 + 3 / 32, -2.0 + 7 / 32])


def test_equal_counts_go_to_the_smallest_j():
    p, q = exact_pan()
    u, v, ok = lattice(p, q, SIZE)
    e = R.scale_exponent(SIZE)
    for seed in range(3):
        counts = []
        for j in range(24):
            h = R.hypothesis(seed, j, u, v, ok, e)
            counts.append(-1 if h is None else int(R.inliers(h, u, v, ok, 2, e).sum()))
        assert counts.count(max(counts)) > 1, "a tie"
        m, info, mask = R.fit_homography(p, q, SIZE, hypotheses=24, thr_q=2, refits=0, seed=seed)
        assert info[3] == counts.index(max(counts)) and info[4] == max(counts) == 60 and info[2] == sum(c >= 0 for c in counts)


def test_a_refit_on_fewer_than_four_inliers_is_skipped():
    p, q = Cs.noisy_matches(80, SIZE, 3, 0.3)
    m0, info0, _ = R.fit_homography(p, q, SIZE, hypotheses=32, thr_q=0, refits=0, seed=2)
    m2, info2, _ = R.fit_homography(p, q, SIZE, hypotheses=32, thr_q=0, refits=2, seed=2)
    assert info0[0] == info2[0] == FIT_OK and info2[4] < 4 and info2[6] == 0, "at radius 0 not even the samples need be inliers"
    assert m0.view(np.int64).tolist() == m2.view(np.int64).tolist() and info0.tolist() == info2.tolist()
    # and with a radius the refits happen and change the model
    m0, info0, _ = R.fit_homography(p, q, SIZE, hypotheses=32, thr_q=32, refits=0, seed=2)
    m2, info2, _ = R.fit_homography(p, q, SIZE, hypotheses=32, thr_q=32, refits=2, seed=2)
    assert info2[6] == 2 and info0[6] == 0 and m0.tolist() != m2.tolist() and info0[:5].tolist() == info2[:5].tolist()


def test_seed_and_hypothesis_count_matter():
    p, q = Cs.noisy_matches(120, SIZE, 4, 0.4)
    runs = {(H, seed): R.fit_homography(p, q, SIZE, hypotheses=H, thr_q=16, refits=0, seed=seed) for H in (1, 8, 64) for seed in (0, 1, 0xFFFFFFFF)}
    assert len({tuple(m.tolist()) for m, _, _ in runs.values()}) >= 6
    for seed in (0, 1, 0xFFFFFFFF):
        best = [runs[(H, seed)][1][4] for H in (1, 8, 64)]
        assert best == sorted(best), "more hypotheses never find fewer inliers"
        assert runs[(64, seed)][1][3] >= 0 and runs[(1, seed)][1][3] in (0, -1)


# The referee's worst corner error over seeds 0 .. 9 with 300 matches, 0.05 px noise, 256 hypotheses, radius 1 px and 2 refits,
# measured on the CPU: 640 x 480: 0.0358 px at 40 % outliers, 0.0417 px at 50 %; 97 x 61: 0.0660 px at 40 %, 0.0450 px at 50 %.
# (Pure inliers gave 0.023 .. 0.028 px in the prototype of this refit.)  The bound is twice the worst per size.
ACCURACY = {(640, 480): (0.0417, 0.0835), (97, 61): (0.0660, 0.1320)}


@pytest.mark.parametrize("outliers", [0.4, 0.5])
@pytest.mark.parametrize("size", list(ACCURACY))
def test_accuracy_under_outliers(size, outliers):
    worst = 0.0
    for seed in range(10):
        p, q = Cs.noisy_matches(300, size, seed, outliers)
        m, info, mask = R.fit_homography(p, q, size, hypotheses=256, thr_q=32, refits=2, seed=seed)
        err = Cs.corner_error(m, Cs.true_model(size), size)
        worst = max(worst, err)
        assert info[0] == FIT_OK and info[6] == 2 and info[5] >= 0.9 * (1 - outliers) * 300 * 0.9, (seed, info.tolist())
    print(f"{size} {outliers}: worst corner error {worst:.4f} px, measured {ACCURACY[size][0]}, bound {ACCURACY[size][1]}")
    assert worst <= ACCURACY[size][1]
