"""CPU: the NumPy referee of ofx_fit_motion (tests/fit_motion_ref.py) alone -- the sampler by hand, exact recovery of whole-pixel
pans, the FEW / DEGENERATE statuses, the status, tie and skipped-refit rules, the dependence on seed and H, and its accuracy on
synthetic matches with noise, outliers and unusable matches."""
import numpy as np
import pytest

import fit_motion_ref as R

SIZE = (192, 128)


def grid_points(nx=8, ny=5, x0=20.0, y0=16.0, step=20.0):
    return np.array([[x0 + step * i, y0 + step * j] for j in range(ny) for i in range(nx)], np.float32)


def test_the_sampler_by_hand():
    # mix(0, 0, 0, 0): h = 0 stays 0 through every step
    assert R.mix(0, 0, 0, 0) == 0
    # mix(1, 0, 0, 0): h = 1; h ^= h >> 16 -> 1; h *= 0x7FEB352D -> 0x7FEB352D; h ^= h >> 15 -> 0x7FEB352D ^ 0xFFD6 = 0x7FEBCAFB;
    h = 0x7FEB352D ^ (0x7FEB352D >> 15)
    assert h == 0x7FEBCAFB
    h = (h * 0x846CA68B) & 0xFFFFFFFF
    h ^= h >> 16
    assert R.mix(1, 0, 0, 0) == h == 0x688990C0
    assert [R.mix(0, 1, 0, 0), R.mix(0, 0, 1, 0), R.mix(0, 0, 0, 1)] == [0x6D523710, 0xC4A0E45C, 0xAA6F94B3]
    # the first indices (j = 0 .. 3, k = 0 .. 2, attempt 0), worked out with an independent uint32 implementation
    assert [R.sample_index(0, j, k, 0, 100) for j in range(4) for k in range(3)] == [0, 76, 72, 42, 19, 53, 67, 16, 30, 13, 64, 17]
    assert [R.sample_index(12345, j, k, 0, 1000) for j in range(4) for k in range(3)] == [567, 818, 274, 111, 200, 156, 29, 610, 215, 710, 376, 908]
    assert [R.sample_index(7, 0, 0, a, 10) for a in range(8)] == [5, 0, 2, 4, 8, 4, 7, 3]
    assert all(0 <= R.sample_index(s, j, 2, 7, 1) < 1 for s in (0, 1, 0xFFFFFFFF) for j in (0, 4095))
    assert max(R.sample_index(0xFFFFFFFF, j, 0, 0, 1 << 20) for j in range(4096)) < 1 << 20


@pytest.mark.parametrize("model", ["translation", "similarity", "affine"])
def test_a_whole_pixel_pan_is_recovered_exactly(model):
    p = grid_points()
    q = p + np.float32([4.0, -3.0])
    m, info, mask = R.fit_motion(p, q, SIZE, model=model, hypotheses=16, thr_q=0, refits=2, seed=3)
    assert info[0] == R.FIT_OK and info[1] == 40 and info[4] == 40 and info[5] == 40 and info[6] == 2 and info[7] == 0
    assert m.tolist() == [1.0, 0.0, 4.0, 0.0, 1.0, -3.0]
    assert mask.tolist() == [1] * 40
    if model == "similarity":
        assert np.signbit(m[1]) and not np.signbit(m[3]), "similarity: b = -sb is -0.0 for sb = +0"
        m0, _, _ = R.fit_motion(p, q, SIZE, model=model, hypotheses=16, thr_q=0, refits=0, seed=3)
        assert m0.tolist() == [1.0, 0.0, 4.0, 0.0, 1.0, -3.0] and np.signbit(m0[1])


def degenerate_cases():
    p = grid_points()
    same = np.tile(np.float32([[50.0, 40.0]]), (12, 1))
    line = np.array([[10.0 + 5 * i, 20.0 + 2 * i] for i in range(12)], np.float32)
    nan = p.copy()
    nan[:, 0] = np.nan
    return {
        "coincident, similarity": (same, same + 1, "similarity", R.FIT_DEGENERATE, 12),
        "coincident, affine": (same, same + 1, "affine", R.FIT_DEGENERATE, 12),
        "coincident, translation": (same, same + 1, "translation", R.FIT_OK, 12),
        "collinear, affine": (line, line + 2, "affine", R.FIT_DEGENERATE, 12),
        "collinear, similarity": (line, line + 2, "similarity", R.FIT_OK, 12),
        "all unusable": (nan, p, "translation", R.FIT_FEW, 0),
        "two usable, affine": (np.concatenate([p[:2], nan[:5]]), np.concatenate([p[:2], p[:5]]), "affine", R.FIT_FEW, 2),
        "outside the frame": (p + np.float32([200.0, 0.0]), p, "similarity", R.FIT_FEW, 0),
    }


@pytest.mark.parametrize("name", list(degenerate_cases()))
def test_few_and_degenerate(name):
    p, q, model, status, usable = degenerate_cases()[name]
    m, info, mask = R.fit_motion(p, q, SIZE, model=model, hypotheses=32, thr_q=0, refits=1, seed=1)
    assert info[0] == status and info[1] == usable
    if status != R.FIT_OK:
        assert m.tolist() == list(R.IDENTITY) and info.tolist() == [status, usable, 0, -1, 0, 0, 0, 0] and not mask.any()
    else:
        assert info[2] > 0 and info[3] >= 0


def test_the_status_rule_with_pair():
    p = grid_points()
    q = p + np.float32([2.0, 1.0])
    status = np.zeros(40, np.int32)
    status[:10] = (5 << 8) | 3          # lost in pair 5: alive through pairs 1 .. 4
    status[10:15] = (2 << 8) | 1        # lost in pair 2: alive through pair 1 only
    for pair, usable in ((0, 40), (1, 40), (2, 35), (4, 35), (5, 25), (9, 25)):
        _, _, ok = R.lattice(p, q, SIZE, status, pair)
        assert int(ok.sum()) == usable
        assert R.fit_motion(p, q, SIZE, status, pair, "translation", 8, 0, 0, 0)[1][1] == usable
    assert R.lattice(p, q, SIZE, None, 3)[2].all()


def test_equal_counts_go_to_the_smallest_j():
    # two clusters of duplicated matches, ten with a pan of (1, 0) and ten with (0, 1): every translation hypothesis counts 10
    p = np.tile(np.float32([[30.0, 30.0]]), (20, 1))
    q = p.copy()
    q[:10, 0] += 1
    q[10:, 1] += 1
    for seed in range(6):
        m, info, mask = R.fit_motion(p, q, SIZE, model="translation", hypotheses=16, thr_q=0, refits=0, seed=seed)
        assert info[3] == 0 and info[4] == 10 and info[2] == 16
        first = R.sample_index(seed, 0, 0, 0, 20)
        assert m.tolist() == ([1, 0, 1, 0, 1, 0] if first < 10 else [1, 0, 0, 0, 1, 1])
        assert mask.tolist() == ([1] * 10 + [0] * 10 if first < 10 else [0] * 10 + [1] * 10)
    assert {R.sample_index(seed, 0, 0, 0, 20) < 10 for seed in range(6)} == {True, False}, "both clusters win for some seed"


def test_a_skipped_refit_keeps_the_model():
    # a single usable match: the similarity and affine refits have Cxx + Cyy = 0 and are skipped, the translation refit is not
    p = grid_points()
    q = p + np.float32([2.0, 1.0])
    u, v, ok = R.lattice(p[:1], q[:1], SIZE)
    start = tuple(np.float64(t) for t in (1.0, 0.0, 64.0, 0.0, 1.0, 32.0))
    inl = R.inliers(start, u, v, ok, 0)
    assert inl.tolist() == [True]
    for model in (R.SIMILARITY, R.AFFINE):
        m, done = R.refit(model, start, u, v, inl)
        assert not done and m is start
    m, done = R.refit(R.TRANSLATION, start, u, v, inl)
    assert done and [float(t) for t in m] == [1.0, 0.0, 64.0, 0.0, 1.0, 32.0]
    m, done = R.refit(R.TRANSLATION, start, u, v, np.zeros(1, bool))
    assert not done and m is start
    # through the whole fit: coincident matches of one pan under the translation model refit; info[6] counts what ran
    same = np.tile(np.float32([[50.0, 40.0]]), (12, 1))
    assert R.fit_motion(same, same + 1, SIZE, model="translation", hypotheses=4, thr_q=0, refits=3)[1][6] == 3
    # collinear points under the similarity model: valid hypotheses, a similarity refit is fine (den > 0)
    line = np.array([[10.0 + 5 * i, 20.0 + 2 * i] for i in range(12)], np.float32)
    assert R.fit_motion(line, line + 2, SIZE, model="similarity", hypotheses=4, thr_q=0, refits=2)[1][6] == 2


def synthetic(rng, n, outliers, unusable, affine):
    """matches of a similarity (or a sheared affine map) about the image origin with 0.05 px noise, a share of uniform outliers
    and a share of unusable matches; returns (p, q, the true map, the true inliers)"""
    w, h = SIZE
    s, r = 1.03, 0.02
    A = np.array([[s * np.cos(r), -s * np.sin(r)], [s * np.sin(r), s * np.cos(r)]])
    if affine:
        A = A @ np.array([[1.0, 0.03], [0.0, 0.98]])
    t = np.array([3.3, -1.7])
    p = np.stack([rng.uniform(12, w - 13, n), rng.uniform(12, h - 13, n)], axis=1)
    q = p @ A.T + t + rng.normal(0.0, 0.05, (n, 2))
    kind = rng.permutation(n)
    out, bad = kind[:int(outliers * n)], kind[int(outliers * n):int((outliers + unusable) * n)]
    q[out] = np.stack([rng.uniform(0, w - 1, len(out)), rng.uniform(0, h - 1, len(out))], axis=1)
    q[bad[0::3]] = np.nan
    p[bad[1::3], 0] = -5.0
    q[bad[2::3], 1] = h + 7.0
    good = np.ones(n, bool)
    good[out] = good[bad] = False
    good &= (q >= 0).all(axis=1) & (q[:, 0] <= w - 1) & (q[:, 1] <= h - 1)
    return p.astype(np.float32), q.astype(np.float32), (A, t), good


def corner_error(m, truth):
    A, t = truth
    w, h = SIZE
    c = np.array([[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]], np.float64)
    got = c @ np.array([[m[0], m[1]], [m[3], m[4]]]).T + np.array([m[2], m[5]])
    return float(np.abs(got - (c @ A.T + t)).max())


@pytest.mark.parametrize("model,n,outliers,H", [("similarity", 300, 0.4, 256), ("affine", 300, 0.4, 256), ("similarity", 1000, 0.5, 512),
                                                ("affine", 1000, 0.5, 512)])
def test_accuracy_on_synthetic_matches(model, n, outliers, H):
    worst = 0.0
    for seed in range(3):
        rng = np.random.default_rng(100 + seed)
        p, q, truth, good = synthetic(rng, n, outliers, 0.2 if n == 300 else 0.1, model == "affine")
        m, info, mask = R.fit_motion(p, q, SIZE, model=model, hypotheses=H, thr_q=32, refits=2, seed=seed)
        assert info[0] == R.FIT_OK and info[6] == 2
        # every true inlier is counted: their noise of 0.05 px (sigma) is 20 sigma inside the radius of 1 px
        assert mask[good].all(), (seed, int(good.sum()), int(mask[good].sum()))
        worst = max(worst, corner_error(m, truth))
    print(f"{model} n={n}: worst corner error {worst:.4f} px")
    assert worst <= 0.1


def test_accuracy_of_the_translation_model():
    worst = 0.0
    for seed in range(3):
        rng = np.random.default_rng(200 + seed)
        w, h = SIZE
        n = 300
        p = np.stack([rng.uniform(12, w - 13, n), rng.uniform(12, h - 13, n)], axis=1)
        t = np.array([3.3, -1.7])
        q = p + t + rng.normal(0.0, 0.05, (n, 2))
        out = rng.permutation(n)[:120]
        q[out] = np.stack([rng.uniform(0, w - 1, 120), rng.uniform(0, h - 1, 120)], axis=1)
        m, info, mask = R.fit_motion(p.astype(np.float32), q.astype(np.float32), SIZE, model="translation", hypotheses=256, thr_q=32, refits=2, seed=seed)
        good = np.ones(n, bool)
        good[out] = False
        assert info[0] == R.FIT_OK and mask[good].all()
        worst = max(worst, corner_error(m, (np.eye(2), t)))
    print(f"translation: worst corner error {worst:.4f} px")
    assert worst <= 0.1


def test_another_seed_or_another_h_changes_the_best_hypothesis():
    rng = np.random.default_rng(5)
    p, q, _, _ = synthetic(rng, 300, 0.4, 0.2, False)
    # a radius of 2/32 px, about the noise: the counts tell the hypotheses apart, so a later j can beat an earlier one
    best = {(seed, H): int(R.fit_motion(p, q, SIZE, model="similarity", hypotheses=H, thr_q=2, refits=0, seed=seed)[1][3])
            for seed in (0, 1, 2) for H in (8, 256)}
    assert len({best[(s, 256)] for s in (0, 1, 2)}) > 1, best
    assert any(best[(s, 8)] != best[(s, 256)] for s in (0, 1, 2)), best


def test_compose_and_invert():
    a = np.array([1.03, -0.02, 3.3, 0.02, 1.03, -1.7])
    b = np.array([0.98, 0.05, -2.0, -0.04, 1.01, 0.5])
    ident = np.array(R.IDENTITY)
    assert R.compose(a, ident).tolist() == a.tolist() and R.compose(ident, a).tolist() == a.tolist()
    x = np.array([17.0, -4.0])
    apply = lambda m, x: np.array([m[0] * x[0] + m[1] * x[1] + m[2], m[3] * x[0] + m[4] * x[1] + m[5]])
    assert np.allclose(apply(R.compose(b, a), x), apply(b, apply(a, x)), rtol=0, atol=1e-12)
    assert np.allclose(R.compose(R.invert(a), a), ident, rtol=0, atol=1e-12)
    assert R.invert([1, 2, 0, 2, 4, 0]) is None and R.invert([np.inf, 0, 0, 0, 1, 0]) is None and R.invert([np.nan, 0, 0, 0, 1, 0]) is None
    assert R.invert([1, 0, 4, 0, 1, -3]).tolist() == [1.0, -0.0, -4.0, -0.0, 1.0, 3.0]
