"""GPU: the stream pipeline's sampled output stage -- the arrow field of main.cu:123-169 and tracked points, read from the flow
pyramids of every pair a call completes by ONE launch (ofx_session_stream_arrows / _stream_tracks), the stateless calls
underneath (ofx_sample_arrows / ofx_advect_points) and engine.video_arrows / video_tracks on top.  The referee is
tests/sampled_ref.py (plain NumPy) on oracle.compose_flow of the pair-at-a-time flows; every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import sampled_ref as R
from cuda_optical_flow_2_amd import synth

pytestmark = pytest.mark.gpu

GUARD = 64  # 4-byte words of 0x5A before and after every output
_vp = C.c_void_p


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cuda_optical_flow_2_amd import engine

    return engine


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype}{got.shape} vs {want.dtype}{want.shape}"
    a, b = got.view(np.uint32), want.view(np.uint32)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        raise AssertionError(f"{what}: {len(bad)}/{a.size} words differ, first at {bad[:3].tolist()}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}")


class Guarded:
    """n slots of `shape` 4-byte elements, `pad` more words between slots (beyond the 16-byte rounding), GUARD words before
    and after, everything filled with 0x5A bytes."""

    def __init__(self, n, shape, dtype, pad=0):
        import torch

        assert pad % 4 == 0
        self.slot = int(np.prod(shape))
        self.stride = (self.slot + 3) // 4 * 4 + pad
        self.flat = torch.empty(2 * GUARD + n * self.stride, dtype=dtype, device="cuda")
        self.flat.view(torch.uint8).fill_(0x5A)
        inner = tuple(int(np.prod(shape[i + 1:])) for i in range(len(shape)))
        self.ring = self.flat.as_strided((n,) + tuple(shape), (self.stride,) + inner, GUARD)
        self.outside = np.ones(self.flat.numel(), bool)
        for i in range(n):
            self.outside[GUARD + i * self.stride:GUARD + i * self.stride + self.slot] = False

    def check_guards(self, what):
        raw = self.flat.cpu().numpy().view(np.uint32)
        bad = np.flatnonzero(self.outside & (raw != 0x5A5A5A5A))
        assert bad.size == 0, f"{what}: {bad.size} guard / padding words overwritten, first at {bad[:4].tolist()}"

    def host(self):
        return self.ring.cpu().numpy()


def _upload(pyr):
    import torch

    keep, ptrs = [], (_vp * 12)()
    for k, p in enumerate(pyr):
        if p is not None:
            t = torch.from_numpy(np.ascontiguousarray(p)).cuda()
            keep.append(t)
            ptrs[k] = t.data_ptr()
    return keep, ptrs


def _field(oracle, pyr, L, lv):
    """oracle.compose_flow of a pyramid whose levels below `lv` are absent"""
    h, w, _ = pyr[lv].shape
    filled = [p if p is not None else np.zeros(((h << lv) >> k, (w << lv) >> k, 2), np.float32) for k, p in enumerate(pyr)]
    return oracle.compose_flow(filled, L, lv)


# ---- the stateless calls ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("arrow_res", R.ARROW_RES, ids=str)
@pytest.mark.parametrize("case", R.STATELESS_CASES, ids=lambda c: "x".join(map(str, c)))
def test_sample_arrows(eng, oracle, case, arrow_res):
    import torch

    W, H, L, lv = case
    pyr, res, w, h = R.arrow_case(case, arrow_res)
    want = R.arrows(_field(oracle, pyr, L, lv), res)
    assert eng.arrow_grid(w, h, res) == R.arrow_grid(w, h, res)
    keep, ptrs = _upload(pyr)
    out = Guarded(1, want.shape, torch.int32)
    lib = eng._lib.load()
    eng.check(lib.ofx_sample_arrows(ptrs, w, h, L, lv, res, out.ring.data_ptr(), eng._stream_ptr()), "ofx_sample_arrows")
    torch.cuda.synchronize()
    same_bits(out.host()[0], want, f"{case} arrow_res {res}")
    out.check_guards(f"{case} arrow_res {res}")


@pytest.mark.parametrize("n_points", [1, 1000, 1 << 21])
@pytest.mark.parametrize("case", R.STATELESS_CASES, ids=lambda c: "x".join(map(str, c)))
def test_advect_points(eng, oracle, case, n_points):
    import torch

    W, H, L, lv = case
    pyrs, pts, w, h = R.track_case(case, n_points)
    d_pts, d_st = Guarded(1, (n_points, 2), torch.float32), Guarded(1, (n_points,), torch.int32)
    d_pts.ring[0].copy_(torch.from_numpy(pts))
    d_st.ring.zero_()
    lib = eng._lib.load()
    st = np.zeros(n_points, np.int32)
    for q, pyr in enumerate(pyrs):
        pts, st = R.advect(_field(oracle, pyr, L, lv), pts, st, q + 1)
        keep, ptrs = _upload(pyr)
        eng.check(lib.ofx_advect_points(ptrs, w, h, L, lv, q + 1, d_pts.ring.data_ptr(), d_st.ring.data_ptr(), n_points, eng._stream_ptr()),
                  "ofx_advect_points")
        torch.cuda.synchronize()
        same_bits(d_pts.host()[0], pts, f"{case} n {n_points}: positions after pair {q + 1}")
        same_bits(d_st.host()[0], st, f"{case} n {n_points}: status after pair {q + 1}")
    d_pts.check_guards("points")
    d_st.check_guards("status")


def test_stateless_refusals(eng):
    import torch

    lib = eng._lib.load()
    pyr = R.synth_pyramid(64, 48, 3, 0, 1, 1.0)
    keep, ptrs = _upload(pyr)
    dst = torch.zeros(64 * 48 * 4, dtype=torch.int32, device="cuda")
    pts = torch.zeros((4, 2), dtype=torch.float32, device="cuda")
    st = torch.zeros(4, dtype=torch.int32, device="cuda")
    assert lib.ofx_sample_arrows(ptrs, 64, 48, 3, 0, 65, dst.data_ptr(), None) == 1       # offset would be 0
    assert lib.ofx_sample_arrows(ptrs, 64, 48, 3, 0, 0, dst.data_ptr(), None) == 1
    assert lib.ofx_sample_arrows(ptrs, 64, 48, 3, 0, 30, dst.data_ptr() + 4, None) == 1   # misaligned
    assert lib.ofx_sample_arrows(ptrs, 62, 48, 3, 0, 30, dst.data_ptr(), None) == 1       # level 1 would be odd
    assert lib.ofx_sample_arrows(ptrs, 64, 48, 3, 3, 30, dst.data_ptr(), None) == 1
    assert lib.ofx_advect_points(ptrs, 64, 48, 3, 0, 0, pts.data_ptr(), st.data_ptr(), 4, None) == 1   # pair 0 is "alive"
    assert lib.ofx_advect_points(ptrs, 64, 48, 3, 0, 1, pts.data_ptr(), st.data_ptr(), 0, None) == 1
    assert lib.ofx_advect_points(ptrs, 64, 48, 3, 0, 1, pts.data_ptr() + 4, st.data_ptr(), 4, None) == 1
    ptrs[1] = None
    assert lib.ofx_advect_points(ptrs, 64, 48, 3, 0, 1, pts.data_ptr(), st.data_ptr(), 4, None) == 1   # a level is missing
    torch.cuda.synchronize()
    assert int(dst.abs().sum()) == 0 and int(st.abs().sum()) == 0


# ---- the stream pipeline ------------------------------------------------------------------------------------------------------

def _frames(w, h, nf, pitch, seed=41):
    import torch

    out = []
    for i in range(nf):
        buf = torch.full((h, pitch), 0x5A, dtype=torch.uint8, device="cuda")
        buf[:, :w] = torch.from_numpy(synth.smooth_pair(w, h, 1.2 * i, -0.6 * i, seed=seed)[1]).cuda()
        out.append(buf[:, :w])
    return out


def _colour_clip(w, h, nf, seed=21):
    out = []
    for i in range(nf):
        g = synth.smooth_pair(w, h, 1.3 * i, -0.7 * i, seed=seed)[1].astype(np.int32)
        out.append(np.stack([np.clip(g + 11, 0, 255), np.clip(g - 5, 0, 255), np.clip(g + (i % 3), 0, 255)], axis=2).astype(np.uint8))
    return out


def _chain(lib, src3, w, h, dst1, dst_pitch, bilateral=True):
    """the three-launch chain the front end fuses: grayscale_avg -> bilateral(g, g) 9 x 9 (2, 10) -> channel 0"""
    import torch

    g = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
    assert lib.ofx_grayscale_avg_3ch(src3.data_ptr(), g.data_ptr(), w, h, None) == 0
    if bilateral:
        f = torch.empty_like(g)
        assert lib.ofx_bilateral_3ch(g.data_ptr(), g.data_ptr(), f.data_ptr(), w, h, 9, 9, 2.0, 10.0, None) == 0
        g = f
    assert lib.ofx_extract_ch0(g.data_ptr(), dst1.data_ptr(), w, h, dst_pitch, None) == 0


def _plain(eng, frames, w, h, L, win, mode, iters=1):
    """Per-level flows of every pair through the pair-at-a-time path."""
    import torch

    s = eng.Session(w, h, L, win, mode, iters=iters)
    s.set_frame_device(frames[0]); s.build_pyramid(); s.swap()
    want = {}
    for i in range(1, len(frames)):
        s.set_frame_device(frames[i]); s.build_pyramid(); s.run_flow()
        torch.cuda.synchronize()
        want[i] = [s.flow_host(k) for k in range(L)]
        s.swap()
    s.close()
    return want


def _drive(submits, drains, frames, on_done):
    """Feed every frame to every session (lock-step), then drain; on_done(pair) after each call that completed pairs."""
    for f in frames:
        d = {sub(f) for sub in submits}
        assert len(d) == 1
        d = d.pop()
        if d >= 1:
            on_done(d)
    while True:
        d = {dr() for dr in drains}
        assert len(d) == 1
        d = d.pop()
        if d == -2:
            return
        if d >= 1:   # (a drain tick may complete nothing: -1)
            on_done(d)


class Outputs:
    """A session's sampled outputs in guarded buffers."""

    def __init__(self, s, w, h, level, arrow_res, pts, n_slots, pad=0, arrows=True, tracks=True, history=True):
        import torch

        lw, lh = w >> level, h >> level
        self.s, self.n_slots = s, n_slots
        self.arrows = self.points = self.status = self.hist = None
        if arrows:
            _, ny, nx = R.arrow_grid(lw, lh, arrow_res)
            self.arrows = Guarded(n_slots, (ny, nx, 4), torch.int32, pad)
            s.stream_arrows(self.arrows.ring, level, arrow_res)
        if tracks:
            n = len(pts)
            self.points, self.status = Guarded(1, (n, 2), torch.float32), Guarded(1, (n,), torch.int32)
            self.hist = Guarded(n_slots, (n, 2), torch.float32, pad) if history else None
            self.reset(pts)
            s.stream_tracks(self.points.ring[0], self.status.ring[0], self.hist.ring if history else None, level)

    def reset(self, pts):
        import torch

        self.points.ring[0].copy_(torch.from_numpy(pts))
        self.status.ring.zero_()

    def check_guards(self, what):
        for name in ("arrows", "points", "status", "hist"):
            if getattr(self, name) is not None:
                getattr(self, name).check_guards(f"{what}: {name}")


def _session(eng, w, h, L, win, mode, iters, B, kind):
    colour = kind == "colour"
    borrow, two = kind != "copied", kind in ("two_stage", "colour")
    s = eng.Session(w, h, L, win, mode, iters=iters, stream_batch=B, borrow_frames=borrow, two_stage=two)
    if colour:
        s.stream_frontend("bilateral", 9, 2.0, 10.0, first_grey=True)
    return s, (s.stream_submit_3ch if colour else s.stream_submit)


def _clip_for(eng, w, h, nf, kind, iters, seed):
    """(the frames a session of this kind is fed, the grey frames the pair-at-a-time referee runs on)"""
    import torch

    if kind != "colour":
        pitch = eng.pitch_for(w) if iters > 1 else (w + 3) // 4 * 4 + 8
        frames = _frames(w, h, nf, pitch, seed)
        return frames, frames
    lib = eng._lib.load()
    clip = [torch.from_numpy(f).cuda() for f in _colour_clip(w, h, nf, seed)]
    grey = torch.zeros((nf, h, eng.pitch_for(w)), dtype=torch.uint8, device="cuda")
    for i, f in enumerate(clip):
        _chain(lib, f, w, h, grey[i], eng.pitch_for(w), bilateral=i > 0)
    torch.cuda.synchronize()
    return clip, [grey[i, :, :w] for i in range(nf)]


# (w, h, levels, window, mode, iters, frames, B, frame kind, level, arrow_res)
CONFIGS = [
    (640, 480, 3, 7, "lk_float", 1, 11, 1, "copied", 0, 30),
    (640, 480, 4, 7, "compat_cpu", 1, 13, 2, "borrowed", 1, 30),
    (1000, 564, 3, 9, "lk_float", 1, 19, 8, "two_stage", 0, 30),         # coarsest 250 x 141
    (1000, 568, 4, 9, "lk_float", 3, 12, 8, "two_stage", 1, 7),          # coarsest 125 x 71
    (640, 480, 4, 7, "lk_float", 3, 10, 2, "copied", 0, 640),            # an arrow per pixel
    (320, 240, 3, 5, "compat_cpu", 1, 21, 8, "borrowed", 0, 30),         # 20 pairs: two and a half ticks of eight
    (320, 240, 4, 9, "lk_float", 1, 12, 2, "colour", 0, 30),
    (192, 128, 3, 9, "lk_float", 3, 14, 8, "colour", 1, 7),
]


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "-".join(map(str, c)))
def test_stream_arrows_and_tracks_equal_the_referee(eng, oracle, cfg):
    import torch

    w, h, L, win, mode, iters, nf, B, kind, level, res = cfg
    lw, lh = w >> level, h >> level
    frames, grey = _clip_for(eng, w, h, nf, kind, iters, seed=31 + B)
    want = _plain(eng, grey, w, h, L, win, mode, iters)
    fields = [oracle.compose_flow(want[p], L, level) for p in range(1, nf)]
    pts = R.synth_points(lw, lh, 700, seed=B)
    ref_arrows = [R.arrows(Cf, res) for Cf in fields]
    _, ref_st, ref_hist = R.track(fields, pts)
    # session 0: rings of exactly B slots, read as the pairs complete; session 1: more slots than pairs and a padded stride, read at the end
    sess, subs, outs = [], [], []
    for n_slots, pad in ((B, 0), (nf + 1, 8)):
        s, sub = _session(eng, w, h, L, win, mode, iters, B, kind)
        outs.append(Outputs(s, w, h, level, res, pts, n_slots, pad))
        s.stream_begin()
        sess.append(s)
        subs.append(sub)
    s0, o0 = sess[0], outs[0]
    seen = 0

    def on_done(d):
        nonlocal seen
        torch.cuda.synchronize()
        assert 1 <= d - seen <= B
        ring, hist = o0.arrows.host(), o0.hist.host()
        for p in range(seen + 1, d + 1):
            same_bits(s0.arrows_of(p).cpu().numpy(), ref_arrows[p - 1], f"arrows_of({p})")
            same_bits(ring[(p - 1) % B], ref_arrows[p - 1], f"arrow slot of pair {p}")
            same_bits(hist[(p - 1) % B], ref_hist[p - 1], f"history slot of pair {p}")
        same_bits(o0.points.host()[0], ref_hist[d - 1], f"positions after pair {d}")
        # the validity window of arrows_of: the newest B pairs
        for p in (0, d - B, d + 1):
            with pytest.raises(eng.OfxError, match=r"code 1"):
                s0.arrows_of(p)
        if d - B + 1 >= 1:
            s0.arrows_of(d - B + 1)
        seen = d

    _drive(subs, [s.stream_drain for s in sess], frames, on_done)
    torch.cuda.synchronize()
    assert seen == nf - 1
    ring, hist = outs[1].arrows.host(), outs[1].hist.host()
    for p in range(1, nf):
        same_bits(ring[p - 1], ref_arrows[p - 1], f"{kind} B={B}: arrows of pair {p}")
        same_bits(hist[p - 1], ref_hist[p - 1], f"{kind} B={B}: history of pair {p}")
    for o in outs:
        same_bits(o.points.host()[0], ref_hist[-1], "final positions")
        same_bits(o.status.host()[0], ref_st, "final status")
        o.check_guards(f"{kind} B={B}")
    for s in sess:
        s.close()


def test_tracks_do_not_depend_on_stream_batch(eng):
    import torch

    w, h, L, win, nf = 640, 480, 4, 7, 20
    frames = _frames(w, h, nf, (w + 3) // 4 * 4 + 8, seed=13)
    pts = R.synth_points(w, h, 5000, seed=4)
    sess, outs = [], []
    for B in (1, 8):
        s = eng.Session(w, h, L, win, "lk_float", stream_batch=B, borrow_frames=True, two_stage=True)
        outs.append(Outputs(s, w, h, 0, 30, pts, nf - 1, arrows=False))
        s.stream_begin()
        sess.append(s)
    for s in sess:   # (B = 1 and B = 8 complete pairs at different calls: each on its own)
        for f in frames:
            s.stream_submit(f)
        while s.stream_drain() != -2:
            pass
    torch.cuda.synchronize()
    hist = [o.hist.host() for o in outs]
    same_bits(hist[1], hist[0], "history, B = 8 vs B = 1")
    same_bits(outs[1].points.host(), outs[0].points.host(), "positions, B = 8 vs B = 1")
    same_bits(outs[1].status.host(), outs[0].status.host(), "status, B = 8 vs B = 1")
    same_bits(hist[0][nf - 2], outs[0].points.host()[0], "the last history slot is the final state")
    assert not np.array_equal(hist[0][0], hist[0][nf - 2])
    for o in outs:
        o.check_guards("batch independence")
    for s in sess:
        s.close()


def test_compose_ring_arrows_and_tracks_together(eng, oracle):
    """All three outputs on at once: each equals its run alone, and the ring's contents the per-pair route on flow_of."""
    import torch

    w, h, L, win, B, nf, level, res = 640, 480, 4, 7, 4, 14, 0, 30
    frames = _frames(w, h, nf, (w + 3) // 4 * 4 + 8, seed=19)
    pts = R.synth_points(w, h, 900, seed=8)
    lib = eng._lib.load()

    def make(ring_on, arrows, tracks):
        s = eng.Session(w, h, L, win, "lk_float", stream_batch=B, borrow_frames=True, two_stage=True)
        ring = Guarded(nf - 1, (h, w, 2), torch.float32) if ring_on else None
        if ring_on:
            s.stream_compose(ring.ring, level)
        o = Outputs(s, w, h, level, res, pts, nf - 1, 4, arrows=arrows, tracks=tracks)
        s.stream_begin()
        return s, ring, o

    runs = [make(True, True, True), make(True, False, False), make(False, True, False), make(False, False, True)]
    s_all = runs[0][0]
    via_flow_of, seen = {}, 0

    def on_done(d):
        nonlocal seen
        for p in range(seen + 1, d + 1):
            ptrs = (_vp * 12)()
            for k in range(level, L):
                ptrs[k] = s_all.flow_of(p, k)[0].data_ptr()
            out = torch.empty((h, w, 2), dtype=torch.float32, device="cuda")
            eng.check(lib.ofx_compose_flow(ptrs, w, h, L, level, out.data_ptr(), eng._stream_ptr()), "ofx_compose_flow")
            via_flow_of[p] = out
        seen = d

    _drive([r[0].stream_submit for r in runs], [r[0].stream_drain for r in runs], frames, on_done)
    torch.cuda.synchronize()
    assert seen == nf - 1
    ring_all = runs[0][1].host()
    same_bits(ring_all, runs[1][1].host(), "compose ring: with the sampled stage vs alone")
    for p in range(1, nf):
        same_bits(ring_all[p - 1], via_flow_of[p].cpu().numpy(), f"compose ring slot of pair {p} vs ofx_compose_flow on flow_of")
    same_bits(runs[0][2].arrows.host(), runs[2][2].arrows.host(), "arrows: all on vs alone")
    same_bits(runs[0][2].hist.host(), runs[3][2].hist.host(), "history: all on vs alone")
    same_bits(runs[0][2].points.host(), runs[3][2].points.host(), "positions: all on vs alone")
    same_bits(runs[0][2].status.host(), runs[3][2].status.host(), "status: all on vs alone")
    # and they are the referee's
    fields = [ring_all[p - 1] for p in range(1, nf)]
    want = _plain(eng, frames, w, h, L, win, "lk_float")
    for p in range(1, nf):
        same_bits(fields[p - 1], oracle.compose_flow(want[p], L, level), f"field of pair {p}")
        same_bits(runs[0][2].arrows.host()[p - 1], R.arrows(fields[p - 1], res), f"arrows of pair {p}")
    _, ref_st, ref_hist = R.track(fields, pts)
    same_bits(runs[0][2].hist.host(), np.stack(ref_hist), "history")
    same_bits(runs[0][2].status.host()[0], ref_st, "status")
    for s, ring, o in runs:
        if ring is not None:
            ring.check_guards("compose ring")
        o.check_guards("together")
        s.close()


def test_dense_tracking_a_point_per_pixel_at_1080p(eng, oracle):
    import torch

    w, h, L, win, B, nf = 1920, 1080, 4, 7, 8, 9
    frames = _frames(w, h, nf, eng.pitch_for(w), seed=37)
    ys, xs = np.mgrid[0:h, 0:w]
    pts = np.stack([xs.ravel() + 0.5, ys.ravel() + 0.5], axis=1).astype(np.float32)
    s = eng.Session(w, h, L, win, "lk_float", stream_batch=B, borrow_frames=True, two_stage=True)
    o = Outputs(s, w, h, 0, 30, pts, B, arrows=False)
    s.stream_begin()
    for f in frames:
        s.stream_submit(f)
    while s.stream_drain() != -2:
        pass
    torch.cuda.synchronize()
    got_pts, got_st, got_hist = o.points.host()[0], o.status.host()[0], o.hist.host()
    o.check_guards("dense")
    s.close()
    want = _plain(eng, frames, w, h, L, win, "lk_float")
    ref_pts, ref_st, ref_hist = R.track([oracle.compose_flow(want[p], L, 0) for p in range(1, nf)], pts)
    same_bits(got_pts, ref_pts, "dense: final positions")
    same_bits(got_st, ref_st, "dense: status")
    for p in range(1, nf):
        same_bits(got_hist[(p - 1) % B], ref_hist[p - 1], f"dense: history of pair {p}")
    assert (ref_st == 0).any() and not np.array_equal(ref_pts, pts)


def test_a_second_stream_reuses_the_settings_and_counts_pairs_from_one(eng):
    import torch

    w, h, L, win, B, nf = 320, 240, 3, 7, 4, 11
    frames = _frames(w, h, nf, (w + 3) // 4 * 4 + 8, seed=23)
    pts = R.synth_points(w, h, 400, seed=2)
    s = eng.Session(w, h, L, win, "lk_float", stream_batch=B, borrow_frames=True, two_stage=True)
    o = Outputs(s, w, h, 0, 30, pts, nf - 1)
    runs = []
    for rep in range(2):
        o.reset(pts)       # (the caller owns points and status: stream_begin does not touch them)
        s.stream_begin()
        with pytest.raises(eng.OfxError):
            s.arrows_of(1)                       # nothing sampled yet in this stream
        last = -1
        for f in frames:
            last = max(last, s.stream_submit(f))
        while True:
            d = s.stream_drain()
            if d == -2:
                break
            last = max(last, d)
        torch.cuda.synchronize()
        assert last == nf - 1
        runs.append((o.arrows.host().copy(), o.hist.host().copy(), o.points.host().copy(), o.status.host().copy()))
        o.arrows.ring.fill_(-7)
        o.hist.ring.fill_(-7.0)
    for a, b in zip(runs[0], runs[1]):
        same_bits(b, a, "second stream vs first")
    st = runs[0][3][0]
    assert st.min() >= 0 and st.max() <= nf - 1 and (st > 0).any()
    o.check_guards("two streams")
    s.close()


def test_refusals(eng):
    import torch
    from cuda_optical_flow_2_amd.parallel import ShardPlan

    w, h, L, win, B = 320, 240, 3, 7, 4
    s = eng.Session(w, h, L, win, "lk_float", stream_batch=B)
    lib, hd = s.L, s._h
    _, ny, nx = R.arrow_grid(w, h, 30)
    slot = ny * nx * 16
    ring = torch.zeros(2 * B * slot, dtype=torch.int32, device="cuda")
    pts = torch.zeros((16, 2), dtype=torch.float32, device="cuda")
    st = torch.zeros(16, dtype=torch.int32, device="cuda")
    hist = torch.zeros((B, 16, 2), dtype=torch.float32, device="cuda")
    base = ring.data_ptr()
    assert lib.ofx_session_stream_arrows(hd, 0, w + 1, base, 16 * h * w, B) == 1      # arrow_res > w
    assert lib.ofx_session_stream_arrows(hd, 1, w // 2 + 1, base, 16 * h * w, B) == 1  # ... the level's w
    assert lib.ofx_session_stream_arrows(hd, 0, 0, base, slot, B) == 1                # arrow_res < 1
    assert lib.ofx_session_stream_arrows(hd, 0, -3, base, slot, B) == 1
    assert lib.ofx_session_stream_arrows(hd, 0, 30, base, slot, B - 1) == 1           # fewer slots than stream_batch
    assert lib.ofx_session_stream_arrows(hd, 0, 30, base + 4, slot, B) == 1           # misaligned ring
    assert lib.ofx_session_stream_arrows(hd, 0, 30, base, slot + 8, B) == 1           # stride not a multiple of 16
    assert lib.ofx_session_stream_arrows(hd, 0, 30, base, slot - 16, B) == 1          # stride shorter than a slot
    assert lib.ofx_session_stream_arrows(hd, L, 30, base, slot, B) == 1               # level out of range
    assert lib.ofx_session_stream_tracks(hd, 0, pts.data_ptr(), None, 16, None, 0, 0) == 1             # no status
    assert lib.ofx_session_stream_tracks(hd, 0, pts.data_ptr(), st.data_ptr(), 0, None, 0, 0) == 1     # no points
    assert lib.ofx_session_stream_tracks(hd, -1, pts.data_ptr(), st.data_ptr(), 16, None, 0, 0) == 1
    assert lib.ofx_session_stream_tracks(hd, 0, pts.data_ptr(), st.data_ptr(), 16, hist.data_ptr(), 128, B - 1) == 1
    assert lib.ofx_session_stream_tracks(hd, 0, pts.data_ptr(), st.data_ptr(), 16, hist.data_ptr() + 8, 128, B) == 1
    assert lib.ofx_session_stream_tracks(hd, 0, pts.data_ptr(), st.data_ptr(), 16, hist.data_ptr(), 120, B) == 1
    out = _vp()
    assert lib.ofx_session_arrows_of(hd, 1, C.byref(out), None, None) == 4            # no ring
    # once a stream has frames: OFX_E_STATE, for setting and for turning off
    assert lib.ofx_session_stream_arrows(hd, 0, 30, base, slot, B) == 0
    assert lib.ofx_session_stream_tracks(hd, 0, pts.data_ptr(), st.data_ptr(), 16, hist.data_ptr(), 128, B) == 0
    s.stream_begin()
    assert lib.ofx_session_stream_arrows(hd, 0, 30, base, slot, B) == 0               # right after stream_begin: still allowed
    frames = _frames(w, h, 3, w, seed=5)
    s.stream_submit(frames[0])
    assert lib.ofx_session_stream_arrows(hd, 0, 30, base, slot, B) == 4
    assert lib.ofx_session_stream_arrows(hd, 0, 30, None, 0, 0) == 4
    assert lib.ofx_session_stream_tracks(hd, 0, pts.data_ptr(), st.data_ptr(), 16, None, 0, 0) == 4
    assert lib.ofx_session_stream_tracks(hd, 0, None, None, 0, None, 0, 0) == 4
    for f in frames[1:]:
        s.stream_submit(f)
    while s.stream_drain() != -2:
        pass
    torch.cuda.synchronize()
    # between streams both may be changed again, and turned off
    s.stream_arrows(None)
    s.stream_tracks(None, None)
    assert lib.ofx_session_arrows_of(hd, 1, C.byref(out), None, None) == 4
    s.close()
    # a sharded session: unsupported, both outputs
    plan = ShardPlan(w, h, L, win, 0, 2)
    s = eng.Session(w, h, L, win, "lk_float", shard=plan, local_corner=True, stream_batch=2)
    assert s.L.ofx_session_stream_arrows(s._h, 0, 30, base, slot, B) == 3
    assert s.L.ofx_session_stream_tracks(s._h, 0, pts.data_ptr(), st.data_ptr(), 16, None, 0, 0) == 3
    s.close()


# ---- the clip calls -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,level,iters", [("grey", 0, 1), ("grey", 1, 3), ("grey_odd_pitch", 0, 1), ("colour", 0, 1), ("colour", 1, 1)])
def test_video_arrows_and_tracks_equal_the_referee_on_video_flow(eng, kind, level, iters):
    import torch

    w, h, L, win, N, res = 320, 240, 4, 9, 7, 30
    if kind == "colour":
        clip = torch.from_numpy(np.stack(_colour_clip(w, h, N, seed=61))).cuda()
    else:
        pitch = w + 1 if kind == "grey_odd_pitch" else w
        store = torch.full((N, h, pitch), 0x5A, dtype=torch.uint8, device="cuda")
        for i in range(N):
            store[i, :, :w] = torch.from_numpy(synth.smooth_pair(w, h, 0.9 * i, 0.5 * i, seed=17)[1]).cuda()
        clip = store[:, :, :w]
    flows = eng.video_flow(clip, L, win, level=level, iters=iters).cpu().numpy()
    lw, lh = w >> level, h >> level
    got = eng.video_arrows(clip, L, win, level=level, arrow_res=res, iters=iters)
    assert got.dtype == torch.int32 and tuple(got.shape) == (N - 1,) + R.arrow_grid(lw, lh, res)[1:] + (4,)
    got = got.cpu().numpy()
    for p in range(1, N):
        same_bits(got[p - 1], R.arrows(flows[p - 1], res), f"video_arrows {kind} level {level}: pair {p}")
    pts = R.synth_points(lw, lh, 333, seed=6)     # (an odd count: the frames of the result sit on a padded stride)
    for batch in (None, 2):
        pos, st = eng.video_tracks(clip, pts, L, win, level=level, iters=iters, batch=batch)
        assert tuple(pos.shape) == (N, 333, 2) and tuple(st.shape) == (333,) and st.dtype == torch.int32
        ref_pts, ref_st, ref_hist = R.track([flows[p - 1] for p in range(1, N)], pts)
        same_bits(pos.cpu().numpy(), np.stack([pts] + ref_hist), f"video_tracks {kind} level {level} batch {batch}: positions")
        same_bits(st.cpu().numpy(), ref_st, f"video_tracks {kind} level {level} batch {batch}: status")
