"""CPU: tests/klt_ref.py against the definition "sparse Lucas-Kanade tracking" of include/ofx.h in words, and what the definition
buys on a moving texture.  NumPy only: no library, no GPU."""
import functools

import numpy as np
import pytest

import klt_ref as K

W, H = 192, 128


@functools.lru_cache(maxsize=None)
def tex(sx=0.0, sy=0.0, w=W, h=H):
    a = K.cosine_texture(w, h, sx, sy)
    a.setflags(write=False)
    return a


def alive(n):
    return np.zeros(n, np.int32)


def lattice_points(n, w, h, margin, seed=3):
    rng = np.random.RandomState(seed)
    q = np.stack([rng.randint(32 * margin, 32 * (w - margin), n), rng.randint(32 * margin, 32 * (h - margin), n)], axis=1)
    return (q.astype(np.float32) / np.float32(32)), q


def test_the_sample_is_the_bilinear_value_in_32nds_and_clamps():
    P = np.array([[10, 20], [30, 50]], np.uint8)
    assert K.sample(P, 0, 0) == 320 and K.sample(P, 32, 32) == 1600
    assert K.sample(P, 16, 0) == (16 * 32 * 10 + 16 * 32 * 20 + 16) >> 5 == 480
    assert K.sample(P, 8, 24) == (24 * 8 * 10 + 8 * 8 * 20 + 24 * 24 * 30 + 8 * 24 * 50 + 16) >> 5
    assert K.sample(P, -1, -1) == 320 and K.sample(P, -33, 5000) == 30 * 32 and K.sample(P, 33, 33) == 1600   # floor division, replicate
    assert K.sample(np.full((3, 3), 255, np.uint8), 17, 9) == 8160


def test_zero_motion_leaves_every_lattice_point_in_place_after_one_iteration():
    pts, q = lattice_points(200, W, H, 3)
    pyr = K.pyramid(tex(), 3)
    for win in (3, 9, 23):
        p, s, sad, stats = K.track_pair(pyr, pyr, pts, alive(200), 1, K.Params(win, 1, 0, 0.0, 0))
        assert (s == 0).all() and np.array_equal(p.view(np.uint32), pts.view(np.uint32)) and (sad == 0).all()
        assert stats.tolist() == [200, 0, 0, 0, 0, 600, 0]                       # one iteration per level and point


def test_whole_pixel_pans_are_recovered_exactly():
    big = K.cosine_texture(W + 32, H + 32)
    a = big[16:16 + H, 16:16 + W]
    pts = K.interior_points(W, H, 8, 5, 40)
    # pans inside what the coarsest level's window can capture on this texture (about a pixel there); beyond it Lucas-Kanade locks
    # onto another period of the texture, which is no matter of the arithmetic
    for (sx, sy), levels, win in (((1, -2), 1, 9), ((4, -4), 3, 15), ((2, 2), 2, 9), ((3, 2), 2, 5), ((4, 4), 3, 9), ((2, -2), 2, 23)):
        b = big[16 - sy:16 - sy + H, 16 - sx:16 - sx + W]                        # the content of a at (x, y) is at (x + sx, y + sy)
        p, s, sad, _ = K.track_pair(K.pyramid(a, levels), K.pyramid(b, levels), pts, alive(len(pts)), 1, K.Params(win, 20, 0, 0.0, 0))
        assert (s == 0).all()
        assert np.array_equal(p, pts + np.float32([sx, sy])), (sx, sy, np.abs(p - pts - np.float32([sx, sy])).max())
        assert (sad == 0).all()


def test_flat_window_and_single_edge_are_singular_at_level_0():
    flat = np.full((40, 40), 77, np.uint8)
    edge = np.repeat((np.arange(40) >= 20).astype(np.uint8)[None, :] * 200, 40, axis=0)      # one vertical edge: Gyy = Gxy = 0
    ramp = np.repeat((np.arange(40) * 5).astype(np.uint8)[:, None], 40, axis=1)              # a gradient in y alone
    pts = np.float32([[20, 20], [19.5, 7.25]])
    for img in (flat, edge, ramp):
        p, s, sad, stats = K.track_pair([img], [img], pts, alive(2), 7, K.Params(9, 5, 0, 0.0, 0))
        assert s.tolist() == [(7 << 8) | K.SINGULAR] * 2 and np.array_equal(p, pts) and sad.tolist() == [-1, -1]
        assert stats.tolist() == [0, 0, 2, 0, 0, 0, 0]
    # texture, but less than min_lambda asks
    p, s, _, _ = K.track_pair([tex()], [tex()], np.float32([[90, 60]]), alive(1), 1, K.Params(9, 5, 0, 1e12, 0))
    assert s.tolist() == [(1 << 8) | K.SINGULAR]


def test_a_singular_coarse_level_is_skipped_and_d_is_kept():
    a0, b0 = tex(), tex(1.0, 0.0)
    flat1 = np.full((H // 2, W // 2), 9, np.uint8)
    pts = K.interior_points(W, H, 4, 3, 40)
    prm = K.Params(9, 10, 0, 0.0, 0)
    one = K.track_pair([a0], [b0], pts, alive(12), 1, prm)
    two = K.track_pair([a0, flat1], [b0, flat1], pts, alive(12), 1, prm)
    assert (two[1] == 0).all() and np.array_equal(one[0], two[0]) and np.array_equal(one[2], two[2])
    assert one[3].tolist() == two[3].tolist()                                   # the flat level ran no iteration
    # a textured coarse level whose d is carried through a singular middle level, doubled twice
    a2, b2 = K.pyramid(a0, 3)[2], K.pyramid(tex(4.0, 0.0), 3)[2]
    flat0 = np.full((H, W), 9, np.uint8)
    p, s, _, stats = K.track_pair([flat0, flat1, a2], [flat0, flat1, b2], pts, alive(12), 1, prm)
    assert (s == ((1 << 8) | K.SINGULAR)).all() and stats[5] > 0                # lost at level 0, after iterating at level 2


def test_the_four_reasons_and_frozen_points():
    a, b = tex(), tex(3.0, 0.0)
    pa, pb = K.pyramid(a, 2), K.pyramid(b, 2)
    nan, inf = np.float32("nan"), np.float32("inf")
    pts = np.float32([[90, 60], [nan, 5], [5, inf], [-0.03125, 5], [W - 1 + 0.03125, 5], [5, H - 0.5], [-inf, 5],   # 0 tracked, 1 .. 6 START
                      [W - 2, 60], [W - 1, 30],                                                                     # 7, 8 OUT
                      [100, 70], [50, 50], [0, 0], [W - 1, H - 1]])                                                 # 9 frozen, 10 .. 12
    st = alive(len(pts))
    st[9] = (3 << 8) | K.OUT
    p, s, sad, stats = K.track_pair(pa, pb, pts, st, 5, K.Params(9, 10, 0, 0.0, 0))
    assert s[0] == 0 and np.array_equal(p[0], np.float32([93, 60])) and sad[0] >= 0
    assert s[1:7].tolist() == [(5 << 8) | K.START] * 6
    assert s[7:9].tolist() == [(5 << 8) | K.OUT] * 2
    assert s[9] == (3 << 8) | K.OUT and sad[9] == -1
    lost = s != 0
    assert np.array_equal(p[lost].view(np.uint32), pts[lost].view(np.uint32)) and (sad[lost] == -1).all()
    assert stats[0] == (s == 0).sum() and stats[1] == 6 and stats[3] == (s == ((5 << 8) | K.OUT)).sum() >= 2 and stats[1:5].sum() == lost.sum() - 1
    assert stats[6] == sad[s == 0].sum()
    # RESIDUAL: the same pair under a bound that the corner points' clamped windows miss
    bound = int(sad[0]) + 1
    assert (sad[s == 0] > bound).any()
    p2, s2, sad2, stats2 = K.track_pair(pa, pb, pts, st, 5, K.Params(9, 10, 0, 0.0, bound))
    res = (s == 0) & (sad > bound)
    assert (s2[res] == ((5 << 8) | K.RESIDUAL)).all() and (sad2[res] == -1).all() and np.array_equal(p2[res], pts[res])
    assert np.array_equal(s2[~res], s[~res]) and np.array_equal(sad2[~res], sad[~res]) and stats2[4] == res.sum()


def test_ties_of_lrintf_go_to_even():
    assert K.lattice(np.float32([1.546875, 1.515625, 1.578125, 0.015625, 0.046875]), 0).tolist() == [50, 48, 50, 0, 2]
    assert K.lattice(np.float32([1.546875, 3.0, 5.0, 7.0]), 2).tolist() == [12, 24, 40, 56]
    assert K.lattice(np.float32([3.0, 5.0, 1.0]), 6).tolist() == [2, 2, 0]        # 1.5 -> 2, 2.5 -> 2, 0.5 -> 0
    pts = np.float32([[1.546875 + 60, 40.515625]])
    p, s, _, _ = K.track_pair([tex()], [tex()], pts, alive(1), 1, K.Params(9, 1, 0, 0.0, 0))
    assert s[0] == 0 and p.tolist() == [[61.5625, 40.5]]                           # the point snaps to its lattice point


def test_a_chain_equals_its_single_pairs_however_it_is_cut():
    frames = [K.pyramid(tex(1.25 * i, -0.5 * i), 3) for i in range(5)]
    pts = np.concatenate([K.interior_points(W, H, 6, 4, 30), np.float32([[2, 2], [W - 3, H - 2], [np.nan, 0]])])
    prm = K.Params(9, 6, 1, 0.0, 0)
    whole = K.track_chain(frames, pts, alive(len(pts)), 1, prm)
    p, s = pts, alive(len(pts))
    for b in range(4):
        p, s, sad, stats = K.track_pair(frames[b], frames[b + 1], p, s, 1 + b, prm)
        assert np.array_equal(whole[2][b].view(np.uint32), p.view(np.uint32)) and np.array_equal(whole[3][b], sad)
        assert whole[4][b].tolist() == stats.tolist()
    assert np.array_equal(whole[0].view(np.uint32), p.view(np.uint32)) and np.array_equal(whole[1], s)
    first = K.track_chain(frames[:3], pts, alive(len(pts)), 1, prm)
    second = K.track_chain(frames[2:], first[0], first[1], 3, prm)
    assert np.array_equal(second[0].view(np.uint32), whole[0].view(np.uint32)) and np.array_equal(second[1], whole[1])
    assert np.array_equal(np.concatenate([first[3], second[3]]), whole[3])


def _share(sx, sy, win, levels):
    pts = K.interior_points(W, H, 10, 6, 40)
    assert len(pts) == 60
    p, s, _, _ = K.track_pair(K.pyramid(tex(), levels), K.pyramid(tex(sx, sy), levels), pts, alive(60), 1, K.Params(win, 10, 1, 0.0, 0))
    err = np.abs(p - pts - np.float32([sx, sy])).max(axis=1)
    return float(((s == 0) & (err <= 0.25)).mean()), float(np.median(err))


def test_the_pyramid_is_what_follows_a_pan_of_nine_pixels():
    """A sum of 40 cosines within +-0.6 rad/px (klt_ref.cosine_texture, 192 x 128), regenerated at the shifted coordinates; 60
    interior points, window 9, ten iterations.  Measured on this referee: 0.967 of the points within 0.25 px of (9, 5) with four
    levels, 0.150 with one; the median error at (3.3, -1.7), window 21, four levels is 0.0125 px."""
    four, _ = _share(9.0, 5.0, 9, 4)
    one, _ = _share(9.0, 5.0, 9, 1)
    print(f"within 0.25 px of (9, 5): {four:.3f} with 4 levels, {one:.3f} with 1")
    assert four >= 0.9 and one <= 0.5
    _, med = _share(3.3, -1.7, 21, 4)
    print(f"median error at (3.3, -1.7), window 21: {med:.4f} px")
    assert med <= 1.0 / 16


def test_forward_backward_marks_what_does_not_come_back():
    a, b = K.pyramid(tex(), 3), K.pyramid(tex(2.5, 1.0), 3)
    pts = np.concatenate([K.interior_points(W, H, 6, 4, 30), np.float32([[1, 1], [W - 2, 3]])])
    prm = K.Params(9, 10, 1, 0.0, 0)
    p, s, sad, _ = K.track_pair(a, b, pts, alive(len(pts)), 1, prm)
    p2, s2, sad2 = K.forward_backward(a, b, p, s, sad, pts, 0.0, 1, prm)
    back = K.track_pair(b, a, p, s, 1, prm)
    miss = (s == 0) & ((back[1] != 0) | (np.abs(back[0] - pts) > 0).any(axis=1))
    assert miss.any() and not miss.all()
    assert (s2[miss] == ((1 << 8) | K.FB)).all() and np.array_equal(p2[miss], pts[miss]) and (sad2[miss] == -1).all()
    assert np.array_equal(s2[~miss], s[~miss]) and np.array_equal(p2[~miss], p[~miss])
    wide = K.forward_backward(a, b, p, s, sad, pts, 1000.0, 1, prm)
    assert ((wide[1] != 0) == (s != 0) | ((s == 0) & (back[1] != 0))).all()


# ---- the inputs of tests/test_gpu_klt.py's regimes: what the referee alone says about them -------------------------------------------
def _same_result(a, b):
    return all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y) for x, y in zip(a, b))


def test_every_window_reaches_every_reason_on_the_hard_frame():
    """67 x 45, four levels, the four cases per window of klt_ref.combos: at each window from 3 to 19 there are tracked points and
    points lost for each of the four reasons; at 21 and 23 no window of the frame is SINGULAR any more (measured: 0 of 257), and the
    other three reasons are reached"""
    assert K.ALL_WINDOWS == (3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23)
    for win in K.ALL_WINDOWS:
        reasons = np.zeros(6, np.int64)
        for c in K.combos((win,)):
            _, _, status, _, _, want = K.hard_case(c)
            reasons += K.reasons_of(want, status)
        print(f"window {win}: tracked and lost by reason {reasons.tolist()}")
        must = [0, K.START, K.SINGULAR, K.OUT, K.RESIDUAL] if win <= 19 else [0, K.START, K.OUT, K.RESIDUAL]
        assert (reasons[must] > 0).all() and reasons[5] == 0, (win, reasons.tolist())


def test_on_the_hard_frame_no_window_gives_its_neighbours_result():
    """A launch that ran the instance of the window next to the one asked for -- the same parameters, W - 2 or W + 2 in W's place --
    must not pass: in the case of 257 points, and in the cases of 63 and 65, the referee's status or position differs for some
    point; so does the stats row.  (The case of one point is a single random point: nothing is asked of it.)"""
    for win in K.ALL_WINDOWS:
        for c in K.combos((win,))[1:]:
            pyr, pts, status, pair0, prm, want = K.hard_case(c)
            for other in (win - 2, win + 2):
                if other in K.ALL_WINDOWS:
                    got = K.track_chain(pyr, pts, status, pair0, prm._replace(window=other))
                    differ = (got[1] != want[1]) | (got[0].view(np.uint32) != want[0].view(np.uint32)).any(axis=1)
                    print(f"window {win} as {other}, {c[5]} points: {int(differ.sum())} differ")
                    assert differ.any() and not np.array_equal(got[4], want[4]), (win, other, c)


@pytest.mark.parametrize("window", K.TURN_WINDOWS)
def test_the_many_points_are_lost_in_both_pairs_and_past_the_first_visit(window):
    """klt_ref.turn_case: of the points from index 32 768 on -- those a wave takes on its second visit -- some are tracked to the end,
    some are lost for at least three different reasons, some come frozen; points are lost in both pairs; the specials stand at both
    ends"""
    pyr, pts, status, pair0, prm, want = K.turn_case(window)
    F = K.TURN_FIRST
    assert len(pts) == K.TURN_N == 32768 + 261 and F == 32768 and len(pyr) == 3 and pair0 > 1
    assert prm == K.Params(window, 4, 1, 0.0, 60 * window * window)
    sp = np.float32(K.specials(*K.HARD_SHAPE[:2])).view(np.uint32)
    assert np.array_equal(pts[1:1 + len(sp)].view(np.uint32), sp) and np.array_equal(pts[F + 3:F + 3 + len(sp)].view(np.uint32), sp)
    lattice = pts[30:F:2] * 32
    assert (lattice == np.rint(lattice)).all() and not (pts[31:F:2] * 32 == np.rint(pts[31:F:2] * 32)).all(axis=1).all()       # half on, half off
    tail, alive_in = want[1][F:], status[F:] == 0
    assert (~alive_in).sum() >= 6 and np.array_equal(tail[~alive_in], status[F:][~alive_in])                                  # frozen: kept
    assert np.array_equal(want[0][F:][~alive_in].view(np.uint32), pts[F:][~alive_in].view(np.uint32))
    assert (tail[alive_in] == 0).any()
    reasons = set((tail[alive_in] & 255).tolist()) - {0}
    assert len(reasons) >= 3, reasons
    pairs = set((tail[alive_in & (tail != 0)] >> 8).tolist())
    assert pairs == {pair0, pair0 + 1}                                                    # ... and in both pairs
    stats = want[4]
    print(f"window {window}: stats {stats.tolist()}")
    assert stats.shape == (2, 7) and (stats[:, 1:5].sum(axis=1) > 0).all() and stats[0, K.START] > 0
    assert stats[0, :5].sum() == (status == 0).sum() and stats[1, :5].sum() == stats[0, 0]


@pytest.mark.parametrize("w,h,levels", K.DEEP_SHAPES)
def test_deep_pyramids_track_lose_and_skip_their_tiny_levels(w, h, levels):
    """klt_ref.deep_cases: over a shape's cases points are tracked and go OUT, and with min_lambda the coarsest levels are SINGULAR"""
    assert levels in (6, 7, 8) and ((w >> (levels - 1)), (h >> (levels - 1))) in ((6, 2), (4, 2), (2, 1), (1, 1))
    cases = K.deep_cases(w, h, levels)
    assert len(cases) == 12 and {c[6] for c in cases} == {0, 1}
    total, with_lam = np.zeros(6, np.int64), np.zeros(6, np.int64)
    for name, pyr, pts, status, pair0, prm, loose, want in cases:
        assert len(pyr[0]) == levels and len(pts) == 129 and prm.max_iters == 10 and prm.eps_q == 1
        r = K.reasons_of(want, status)
        print(f"{name}: {r.tolist()}, iterations {int(want[4][0, 5])}")
        total += r
        if prm.min_lambda > 0:
            with_lam += r
    assert total[0] > 0 and total[K.OUT] > 0 and with_lam[K.SINGULAR] > 0
    # the pair of each shift without min_lambda is tried with the tight pitch or the padded one, and with min_lambda with the other
    assert all(a[6] != b[6] for a, b in zip(cases[0::2], cases[1::2]))


@pytest.mark.parametrize("window", K.WIDE_WINDOWS)
def test_the_widest_plane_is_followed_to_its_last_columns(window):
    pyr, pts, status, pair0, prm, want = K.wide_case(window)
    w, h = K.WIDE_W, K.WIDE_H
    assert (w, h) == (1 << 19, 3) and pyr[0][0].shape == (h, w) and len(pyr[0]) == 1
    a = pyr[0][0].astype(np.int32)
    assert a.min() == 0 and a.max() == 255 and np.abs(np.diff(a, axis=1)).max() <= 2 * 51 + 1    # a box of five: a step is a fifth of the range, stretched
    assert np.array_equal(pyr[1][0][:, 1:], pyr[0][0][:, :-1])
    assert len(pts) == 257 and (pts[:, 0] >= w - 1 - 300).all() and (pts[:, 0] <= w - 1).all()
    assert pts[:3].tolist() == [[w - 1, h - 1], [w - 1 - 1 / 32, 0], [w - 1.5, 1]]
    ok = want[1] == 0
    moved = want[0][ok] - pts[ok]
    print(f"window {window}: {int(ok.sum())} tracked, {int(((want[1] & 255) == K.OUT).sum())} OUT, median motion {np.median(moved[:, 0])}, largest x {want[0][ok, 0].max()}")
    assert ok.sum() >= 200 and ((want[1] & 255) == K.OUT).any() and want[0][ok, 0].max() > w - 4
    assert np.median(moved[:, 0]) == 1.0


def test_the_checkerboard_drives_the_sums_to_2_to_the_35():
    a = K.sat_pyramids(1, "shifted")[0][0]
    q = np.arange(-11, 12) * 32
    gx = K.sample(a, 32 * 30 + 32 + q[None, :], 32 * 20 + q[:, None]) - K.sample(a, 32 * 30 - 32 + q[None, :], 32 * 20 + q[:, None])
    assert (np.abs(gx) == 8160).all() and 2 ** 35 < int((gx * gx).sum()) == 529 * 8160 ** 2 < 2 ** 37
    assert np.array_equal(K.sat_pyramids(3, "inverse")[1][0], 255 - K.sat_pyramids(3, "inverse")[0][0])
    tracked = out = 0
    for levels in K.SAT_LEVELS:
        for kind in K.SAT_KINDS:
            for window in K.SAT_WINDOWS:
                _, pts, status, _, _, want = K.sat_case(levels, window, kind)
                r = K.reasons_of(want, status)
                print(f"{levels} levels, {kind}, window {window}: {r.tolist()}")
                assert len(pts) == 257 and r[K.OUT] > 0
                assert (r[0] > 0) != ((levels, kind, window) == (3, "inverse", 23))       # there every point goes OUT: kept
                tracked, out = tracked + int(r[0]), out + int(r[K.OUT])
    assert tracked > 0 and out > 0
