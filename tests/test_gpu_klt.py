"""GPU: sparse Lucas-Kanade tracking -- ofx_track_points, engine.track_points and engine.video_klt -- against tests/klt_ref.py.
Every comparison is exact, floats by their bits, and no point is excluded.  Outputs sit in buffers of 0x5A, the planes at odd
addresses in larger buffers whose surroundings (pad columns included) differ between runs, so that a tap outside a plane, or a
store outside an output, shows."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import klt_ref as K
from test_gpu_interp import AROUND_P, FILL, Guarded, Plane, same

pytestmark = pytest.mark.gpu

OFX_E_INVALID = 1
SHAPES = [(1, 1, 1), (2, 3, 1), (5, 4, 1), (33, 17, 3), (67, 45, 4), (262, 74, 5)]          # (w, h, levels)
NAN, INF = K.NAN, K.INF


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cuda_optical_flow_2_amd import engine

    return engine


# ---- inputs, made once and shared: tests/klt_ref.py has them, for tests/test_klt_ref.py too ---------------------------------------
hard_pyramids, smooth_pyramid, points_for, lam_for, combos, want_chain = K.hard_pyramids, K.smooth_pyramid, K.points_for, K.lam_for, K.combos, K.want_chain


# ---- a launch on guarded buffers ------------------------------------------------------------------------------------------------------
class Clip:
    """the planes of some frames' pyramids on the device, each at an odd address inside `around`; loose: padded pitches"""

    def __init__(self, pyramids, loose, around):
        self.levels = len(pyramids[0])
        self.h, self.w = pyramids[0][0].shape
        self.pitches = [pyramids[0][k].shape[1] + ((3 * k + 5) if loose else 0) for k in range(self.levels)]
        self.planes = [[Plane(np.asarray(p[k]), self.pitches[k], 1 + 2 * ((f + k) % 3) + (6 if loose else 0), around) for k in range(self.levels)]
                       for f, p in enumerate(pyramids)]

    def desc(self, lib, f0=0, n_frames=None):
        n_frames = len(self.planes) - f0 if n_frames is None else n_frames
        self._table = (C.c_void_p * (n_frames * self.levels))(*[pl.ptr for fr in self.planes[f0:f0 + n_frames] for pl in fr])
        self._pitches = (C.c_int * self.levels)(*self.pitches)
        return lib.TrackClip(self.w, self.h, self.levels, n_frames, self._table, self._pitches)


def _put(g, arr):
    import torch

    raw = torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).cuda()
    g.flat[g.lead * g.size: g.lead * g.size + raw.numel()] = raw


def run(eng, clip, prm, pair0, pts, status, f0=0, n_frames=None, hist=True, sad=True, stats=True, expect=0):
    """one ofx_track_points call; returns (points, status, history, sad, stats) as arrays (None where not asked), having checked that
    nothing around them was written"""
    import torch

    lib = eng._lib
    n = len(pts)
    pairs = (len(clip.planes) - f0 if n_frames is None else n_frames) - 1
    g_pts, g_st = Guarded(np.float32, 1, 1, 2 * n, 2 * n, 2), Guarded(np.int32, 1, 1, n, n, 1)
    _put(g_pts, pts), _put(g_st, status)
    g_hist = Guarded(np.float32, 1, pairs, 2 * n, 2 * n, 4) if hist else None
    g_sad = Guarded(np.int32, 1, pairs, n, n, 3) if sad else None
    g_stats = Guarded(np.int64, 1, pairs, 7, 7, 1) if stats else None
    p = lib.TrackParams(prm.window, prm.max_iters, prm.eps_q, prm.max_sad, prm.min_lambda)
    d = clip.desc(lib, f0, n_frames)
    rc = lib.load().ofx_track_points(C.byref(d), C.byref(p), pair0, g_pts.ptr, g_st.ptr, n, g_hist.ptr if hist else None, g_sad.ptr if sad else None,
                                     g_stats.ptr if stats else None, eng._stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, (rc, lib.load().ofx_last_error())
    out = []
    for g, shape in ((g_pts, (n, 2)), (g_st, (n,)), (g_hist, (pairs, n, 2)), (g_sad, (pairs, n)), (g_stats, (pairs, 7))):
        if g is None:
            out.append(None)
            continue
        got, clean = g.host()
        assert clean, "a store outside an output"
        out.append(got.reshape(shape))
    return out


def check(got, want, what, names=("points", "status", "history", "sad", "stats")):
    """got: run()'s outputs (None: not asked for); want: klt_ref.track_chain's"""
    for g, w, name in zip(got, want, names):
        if g is not None:
            same(g, w, f"{what}: {name}")


# ---- 1. one pair --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,levels", SHAPES)
def test_a_pair_on_the_hard_frame_equals_the_referee(eng, w, h, levels):
    """windows 3, 9, 23 (at 67 x 45 every window 3 .. 23: each instance of klt_kernel<R>, M = 1 .. 9 window pixels per lane) x 1,
    63, 65, 257 points -- ragged waves and blocks -- with one and 32 iterations, eps_q 0 and 1, min_lambda and max_sad off and on;
    each once with tight pitches and once with padded ones, the surroundings of the planes differing.  tests/test_klt_ref.py shows
    that at 67 x 45 the referee's result at a window is not its result at a neighbouring one."""
    pa, pb = hard_pyramids(w, h, levels)
    windows = K.ALL_WINDOWS if (w, h, levels) == K.HARD_SHAPE else (3, 9, 23)
    reasons = np.zeros(6, np.int64)
    clips = [Clip([pa, pb], loose, AROUND_P[loose]) for loose in (0, 1)]
    for i, c in enumerate(combos(windows)):
        prm, n = K.Params(*c[:5]), c[5]
        pts, status = points_for(w, h, n, seed=w)
        want = want_chain(("hard", w, h, levels, c), [pa, pb], pts, status, 3, prm)
        reasons += np.bincount(want[1][status == 0] & 255, minlength=6)[:6]
        for loose in ((0, 1) if i % 2 == 0 else (1,)):
            check(run(eng, clips[loose], prm, 3, pts, status), want, f"{w}x{h} {c} loose {loose}")
    print(f"{w}x{h}: tracked and lost by reason {reasons.tolist()}")
    if w >= 33:
        assert (reasons[:5] > 0).all(), f"the cases do not reach every reason: {reasons.tolist()}"


@pytest.mark.parametrize("w,h,levels", SHAPES[4:])
def test_a_pair_on_the_smooth_texture_equals_the_referee(eng, w, h, levels):
    """sub-pixel and nine-pixel shifts, which the pyramid has to carry down"""
    lost = 0
    for sx, sy in ((0.4, -0.3), (9.0, 5.0), (-2.75, 1.5)):
        pa, pb = smooth_pyramid(w, h, levels, 0.0, 0.0), smooth_pyramid(w, h, levels, sx, sy)
        clip = Clip([pa, pb], sx > 1, AROUND_P[1 + (sx > 1)])
        for win in (9, 21):
            prm = K.Params(win, 10, 1, 0.0, 0)
            pts, status = points_for(w, h, 129, seed=int(sx * 4))
            want = want_chain(("smooth", w, h, sx, sy, win), [pa, pb], pts, status, 1, prm)
            check(run(eng, clip, prm, 1, pts, status), want, f"{w}x{h} shift ({sx}, {sy}) window {win}")
            lost += int((want[1][status == 0] != 0).sum())
    assert lost > 0                                               # the motion drives points OUT


# ---- 1b. the regimes of csrc/klt.hip beyond the everyday ones; tests/test_klt_ref.py holds the conditions on these inputs ----------------
@pytest.mark.parametrize("window", K.TURN_WINDOWS)
def test_more_points_than_waves_are_taken_in_turn(eng, window):
    """32 768 + 261 points on two pairs: the launch has 8192 blocks of four waves, so 261 waves come round a second time (the stride
    of the point loop) and 66 blocks gather more points than they have waves in their LDS counters before the one global atomic.  The stats are
    sums over all points: a point visited twice or not at all shows there as well as in its own row."""
    pyr, pts, status, pair0, prm, want = K.turn_case(window)
    assert len(pts) == K.TURN_N == 4 * 8192 + 261 and pair0 > 1
    lost = want[4][:, 1:5].sum(axis=1)
    assert (lost > 0).all() and (want[1][K.TURN_FIRST:] == 0).any() and len(set((want[1][K.TURN_FIRST:][status[K.TURN_FIRST:] == 0] & 255).tolist()) - {0}) >= 3
    print(f"window {window}: stats {want[4].tolist()}")
    loose = int(window == 5)
    check(run(eng, Clip(pyr, loose, AROUND_P[loose]), prm, pair0, pts, status), want, f"{K.TURN_N} points, window {window}")


def _max_levels():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ofx.h")).read()
    return int(re.search(r"#define\s+OFX_TRACK_MAX_LEVELS\s+(\d+)\b", text).group(1))


@pytest.mark.parametrize("w,h,levels", K.DEEP_SHAPES)
def test_pyramids_of_6_7_and_8_levels_equal_the_referee(eng, w, h, levels):
    """up to OFX_TRACK_MAX_LEVELS levels -- the whole plane table of the kernel arguments -- down to coarsest levels of 6 x 2, 4 x 2,
    2 x 1 and 1 x 1 pixels, where every tap of a patch is clamped; without min_lambda those throw most points far OUT (d of many
    pixels, doubled level by level), with it they are SINGULAR and skipped"""
    assert _max_levels() == 8 == max(s[2] for s in K.DEEP_SHAPES)
    assert (w >> (levels - 1)) >= 1 and (h >> (levels - 1)) >= 1 and levels >= 6
    reasons = np.zeros(6, np.int64)
    clips = {}
    for name, pyr, pts, status, pair0, prm, loose, want in K.deep_cases(w, h, levels):
        key = (id(pyr[1]), loose)
        if key not in clips:
            clips[key] = Clip(pyr, loose, AROUND_P[(loose + levels) % 3])
        reasons += K.reasons_of(want, status)
        check(run(eng, clips[key], prm, pair0, pts, status), want, name)
    print(f"{w}x{h}x{levels}: tracked and lost by reason {reasons.tolist()}")
    assert reasons[0] > 0 and reasons[K.OUT] > 0 and reasons[K.SINGULAR] > 0


@pytest.mark.parametrize("window", K.WIDE_WINDOWS)
def test_the_widest_plane_is_tracked_at_its_right_edge(eng, window):
    """w = 2^19, the widest the call accepts: lattice coordinates up to 2^24 - 32, where float32 is exact to the unit and no
    further.  Both the tight pitch and a padded one, at odd addresses"""
    pyr, pts, status, pair0, prm, want = K.wide_case(window)
    assert pyr[0][0].shape == (3, 1 << 19)
    ok = want[1] == 0
    assert ok.sum() >= 200 and ((want[1] & 255) == K.OUT).any() and want[0][ok, 0].max() > (1 << 19) - 4
    for loose in (0, 1):
        check(run(eng, Clip(pyr, loose, AROUND_P[1 + loose]), prm, pair0, pts, status), want, f"w = 2^19, window {window}, loose {loose}")


@pytest.mark.parametrize("levels", K.SAT_LEVELS)
def test_a_checkerboard_of_full_contrast_equals_the_referee(eng, levels):
    """|gx| = 8160 at every window pixel: window sums of 2^35 at window 23 and lane partial sums within a factor 3.6 of int32 --
    the largest that an image can make them"""
    for kind in K.SAT_KINDS:
        clip = None
        for window in K.SAT_WINDOWS:
            pyr, pts, status, pair0, prm, want = K.sat_case(levels, window, kind)
            clip = clip or Clip(pyr, kind == "inverse", AROUND_P[levels % 3])
            check(run(eng, clip, prm, pair0, pts, status), want, f"checkerboard {kind}, {levels} levels, window {window}")


# ---- 2. chains ------------------------------------------------------------------------------------------------------------------------
def test_chains_of_1_2_and_16_pairs_equal_single_pair_launches(eng):
    """17 frames of the texture drifting by (0.7, -0.4) px per frame: the chain of 16 pairs in one launch, cut into 2 + 1 + 13, and
    pair by pair, all against the referee's chain; history, sad and stats each on and off"""
    w, h, levels, n = 67, 45, 4, 65
    pyr = [smooth_pyramid(w, h, levels, 0.7 * i, -0.4 * i) for i in range(17)]
    prm = K.Params(9, 8, 1, lam_for(9) / 2, 100 * 81)
    pts, status = points_for(w, h, n, seed=5)
    want = want_chain("chain", pyr, pts, status, 7, prm)
    assert (np.bincount(want[1][status == 0] & 255, minlength=5)[:5] > 0).all()              # tracked to the end, and every reason
    assert len(set(want[4][:, 0].tolist())) >= 8                                              # points are lost all along the chain
    clip = Clip(pyr, 1, 0xFF)
    check(run(eng, clip, prm, 7, pts, status), want, "16 pairs")
    for hist, sad, stats in ((False, False, False), (True, False, False), (False, True, False), (False, False, True)):
        check(run(eng, clip, prm, 7, pts, status, hist=hist, sad=sad, stats=stats), want, f"16 pairs, outputs {hist} {sad} {stats}")
    for cuts in ((2, 1, 13), (1,) * 16):
        p, s, f0 = pts, status, 0
        for c in cuts:
            got = run(eng, clip, prm, 7 + f0, p, s, f0=f0, n_frames=c + 1)
            check(got[2:], [want[2][f0:f0 + c], want[3][f0:f0 + c], want[4][f0:f0 + c]], f"cuts {cuts}: pairs from {f0}", ("history", "sad", "stats"))
            p, s, f0 = got[0], got[1], f0 + c
        check([p, s], want[:2], f"cuts {cuts}: the end")


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------------------
def test_a_refused_call_writes_nothing(eng):
    import torch

    lib = eng._lib
    L = lib.load()
    w, h, levels, n = 33, 17, 3, 63
    pa, pb = hard_pyramids(w, h, levels)
    clip = Clip([pa, pb], 0, 0x00)
    pts, status = points_for(w, h, n)
    good = dict(window=9, max_iters=10, eps_q=1, max_sad=0, min_lambda=0.0)
    cases = [(dict(window=8), b"window"), (dict(window=25), b"window"), (dict(max_iters=0), b"max_iters"), (dict(max_iters=33), b"max_iters"),
             (dict(eps_q=-1), b"eps_q"), (dict(min_lambda=float("nan")), b"min_lambda"), (dict(max_sad=-1), b"max_sad"), (dict(pair0=0), b"pair0"),
             (dict(n=0), b"n_points"), (dict(levels=9), b"levels"), (dict(levels=6), b"coarsest"), (dict(n_frames=1), b"n_frames"),
             (dict(pitch1=15), b"pitch"), (dict(off_points=4), b"8-byte"), (dict(off_status=2), b"4-byte"), (dict(off_stats=4), b"d_stats"),
             (dict(null_plane=True), b"null")]
    for kw, word in cases:
        g_pts, g_st = Guarded(np.float32, 1, 1, 2 * n, 2 * n, 2), Guarded(np.int32, 1, 1, n, n, 1)
        g_hist, g_sad, g_stats = Guarded(np.float32, 1, 1, 2 * n, 2 * n, 4), Guarded(np.int32, 1, 1, n, n, 3), Guarded(np.int64, 1, 1, 7, 7, 1)
        d = clip.desc(lib)
        d.levels, d.n_frames = kw.get("levels", levels), kw.get("n_frames", 2)
        if "pitch1" in kw:
            clip._pitches[1] = kw["pitch1"]
        if "null_plane" in kw:
            clip._table[4] = None
        p = lib.TrackParams(**{**good, **{k: v for k, v in kw.items() if k in good}})
        rc = L.ofx_track_points(C.byref(d), C.byref(p), kw.get("pair0", 1), g_pts.ptr + kw.get("off_points", 0), g_st.ptr + kw.get("off_status", 0),
                                kw.get("n", n), g_hist.ptr, g_sad.ptr, g_stats.ptr + kw.get("off_stats", 0), eng._stream_ptr())
        msg = L.ofx_last_error()
        torch.cuda.synchronize()
        assert rc == OFX_E_INVALID and word in msg, (kw, rc, msg)
        for g in (g_pts, g_st, g_hist, g_sad, g_stats):
            assert (g.flat.cpu().numpy() == FILL).all(), f"{kw}: something was written"
    prm = K.Params(**good)
    check(run(eng, clip, prm, 1, pts, status), K.track_chain([pa, pb], pts, status, 1, prm), "after the refusals")


# ---- 4. the Python surface ------------------------------------------------------------------------------------------------------------
def test_engine_track_points_with_and_without_the_round_trip(eng):
    import torch

    w, h, levels, win = 192, 128, 4, 9
    a, b = K.cosine_texture(w, h), K.cosine_texture(w, h, 2.5, 1.0)
    pa, pb = eng.klt_pyramid(a, levels).host(), eng.klt_pyramid(b, levels).host()
    assert [p.shape for p in pa] == [(h >> k, w >> k) for k in range(levels)]
    pts = np.concatenate([K.interior_points(w, h, 12, 8, 12), np.float32([[1, 1], [w - 2, 3], [0, 0], [NAN, 4], [w - 1, h - 1]])])
    prm = K.Params(win, 10, 1, 0.0, 0)
    want = K.track_pair(pa, pb, pts, np.zeros(len(pts), np.int32), 1, prm)
    got = eng.track_points(a, b, pts, levels, win)
    for g, wv, name in zip(got, want, ("positions", "status", "sad")):
        assert isinstance(g, np.ndarray)
        same(g, wv, name)
    for fb_max in (0.0, 0.25):
        fb = K.forward_backward(pa, pb, want[0], want[1], want[2], pts, fb_max, 1, prm)
        assert (fb[1] == ((1 << 8) | K.FB)).any() and (fb[1] == 0).any()
        got = eng.track_points(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), torch.from_numpy(pts).cuda(), levels, win, fb_max=fb_max)
        for g, wv, name in zip(got, fb, ("positions", "status", "sad")):
            assert g.is_cuda
            same(g.cpu().numpy(), wv, f"fb_max {fb_max}: {name}")
    prm = K.Params(21, 3, 0, lam_for(21), 500 * 441)
    want = K.track_pair(pa[:2], pb[:2], pts, np.zeros(len(pts), np.int32), 1, prm)
    got = eng.track_points(a, b, pts, 2, 21, max_iters=3, eps=0.0, min_lambda=prm.min_lambda, max_sad=prm.max_sad)
    for g, wv, name in zip(got, want, ("positions", "status", "sad")):
        same(g, wv, f"every parameter: {name}")
    with pytest.raises(eng.OfxError):
        eng.track_points(a, b, pts, levels, 8)


def test_engine_video_klt_equals_the_referees_chain(eng):
    import torch

    w, h, levels, win, N = 192, 128, 3, 9, 6
    frames = np.stack([K.cosine_texture(w, h, 1.25 * i, -0.5 * i) for i in range(N)])
    clip = torch.from_numpy(frames).cuda()
    pyr = [eng.klt_pyramid(f, levels).host() for f in frames]
    prm = K.Params(win, 10, 1, 0.0, 0)
    pts = np.concatenate([K.interior_points(w, h, 9, 6, 10), np.float32([[w - 3, 5], [2, h - 2]])])
    want = K.track_chain(pyr, pts, np.zeros(len(pts), np.int32), 1, prm)
    for batch in (16, 2, 1):
        pos, status, sad, stats = eng.video_klt(clip, pts, levels, win, batch=batch, return_stats=True)
        same(pos[0].cpu().numpy(), pts, "the seeds")
        same(pos[1:].cpu().numpy(), want[2], f"batch {batch}: positions")
        same(status.cpu().numpy(), want[1], f"batch {batch}: status")
        same(sad.cpu().numpy(), want[3], f"batch {batch}: sad")
        same(stats.cpu().numpy(), want[4], f"batch {batch}: stats")
    seeds, _ = eng.good_features(frames[0], win, 16)
    assert len(seeds) >= 20
    auto = eng.video_klt(clip, None, levels, win)
    want = K.track_chain(pyr, seeds, np.zeros(len(seeds), np.int32), 1, prm)
    same(auto[0][0].cpu().numpy(), seeds, "the seeds of good_features")
    same(auto[0][1:].cpu().numpy(), want[2], "seeded: positions")
    same(auto[1].cpu().numpy(), want[1], "seeded: status")
