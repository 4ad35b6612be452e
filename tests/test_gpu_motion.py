"""GPU: motion compensation -- the stateless launch (ofx_motion_compensate) against tests/motion_ref.py, the stream pipeline's
stage (ofx_session_stream_motion) against the two existing launches (engine.shift_1ch, then engine.warp_u8) on what a
pair-at-a-time session of the same parameters holds, and engine.video_motion on top.  Every comparison is exact.

The stream cases: the issue names eight dimensions (clip, size, window, B, pipeline kind, iters, level, mode).  What decides
which buffers the launch reads is iters x B x kind -- the flow set a tick ends in, the image sets and shift-vector slots in use,
whose pitch a borrowed level 0 has -- so ALL 24 of those combinations run; the other five dimensions only change the numbers in
those buffers and are dealt over the 24 so that every value meets every iters, every B and both kinds at least once.

Where the two per-pair pitches are told apart: only in the stateless test (prev at w + 11, next at w + 22).  The borrowed frames
of one stream must share a pitch (ofx_session_stream_submit refuses anything else), so in every stream case prev's pitch equals
next's; the stream stage and the stateless call run the same kernel on the same argument block, and that is what the stream
cases rely on.  Across streams the pitch does change: two values over the borrowed configurations, and a second stream with
another pitch on one session."""
import ctypes as C
import functools

import numpy as np
import pytest

import motion_ref as R
from cuda_optical_flow_2_amd import synth

pytestmark = pytest.mark.gpu

_vp = C.c_void_p
FILL = 0x5A


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cuda_optical_flow_2_amd import engine

    return engine


def same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype}{got.shape} vs {want.dtype}{want.shape}"
    a, b = (got.view(np.uint32), want.view(np.uint32)) if got.dtype == np.float32 else (got, want)   # (floats by their bits: NaN == NaN)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        raise AssertionError(f"{what}: {len(bad)}/{got.size} differ, first at {bad[:3].tolist()}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}")


# ---- 1. the stateless launch ----------------------------------------------------------------------------------------------------

class Embedded:
    """An (h, w) u8 plane as a sub-view of a larger buffer: `pitch` bytes from row to row, `lead` bytes before it, two spare rows
    after it; every byte that is not a pixel holds `around`."""

    def __init__(self, arr, pitch, lead, around):
        import torch

        h, w = arr.shape
        host = np.full(lead + (h + 2) * pitch, around, np.uint8)
        rows = np.lib.stride_tricks.as_strided(host[lead:], (h, w), (pitch, 1))
        rows[...] = arr
        self.t = torch.from_numpy(host).cuda()
        self.ptr, self.pitch = self.t.data_ptr() + lead, pitch


class GuardedImage:
    """n slots of rows x w bytes, rows `pitch` apart, slots `stride` apart, `lead` bytes before and 64 after, all 0x5A."""

    def __init__(self, n, rows, w, pitch, stride=None, lead=64):
        import torch

        self.n, self.rows, self.w, self.pitch, self.lead = n, rows, w, pitch, lead
        self.stride = stride if stride is not None else (rows * pitch + 15) // 16 * 16
        self.flat = torch.full((lead + n * self.stride + 64,), FILL, dtype=torch.uint8, device="cuda")
        self.ring = self.flat.as_strided((n, rows, w), (self.stride, pitch, 1), lead)
        self.ptr = self.flat.data_ptr() + lead

    def host(self):
        """(the pixels [n, rows, w], True when every other byte still holds 0x5A)"""
        raw = self.flat.cpu().numpy()
        px = np.lib.stride_tricks.as_strided(raw[self.lead:], (self.n, self.rows, self.w), (self.stride, self.pitch, 1))
        got = px.copy()
        px[...] = FILL
        return got, bool((raw == FILL).all())


class GuardedStats:
    def __init__(self, n):
        import torch

        self.n = n
        self.flat = torch.full((4 * n + 8,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        self.ring = self.flat[4:4 + 4 * n].view(n, 4)

    def host(self):
        raw = self.flat.cpu().numpy()
        return raw[4:4 + 4 * self.n].reshape(self.n, 4).copy(), bool((raw[:4] == 0x5A5A5A5A5A5A5A5A).all() and (raw[-4:] == 0x5A5A5A5A5A5A5A5A).all())


@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_stateless_equals_the_referee(eng, size):
    import torch

    lib = eng._lib.load()
    n = 0
    for name, w, h, prev1, next1, flow, uv, scale in R.stateless_cases():
        if (w, h) != size:
            continue
        want_mc, want_st = R.motion(prev1, next1, flow, uv, scale)
        tf = torch.from_numpy(flow).cuda()
        tuv = None if uv is None else torch.tensor(list(uv), dtype=torch.float32, device="cuda")
        uvp = None if tuv is None else tuv.data_ptr()
        # the planes sit in larger buffers whose other bytes differ between the runs: a tap outside a plane would show
        runs = []
        for around, dst_pitch, lead in ((FILL, w + 9, 61), (0xC3, (w + 3) // 4 * 4 + 8, 64), (0x00, 0, 64)):
            p = Embedded(prev1, w + 11, 5, around)
            q = Embedded(next1, w + 22, 3, around)
            img = GuardedImage(1, h, w, dst_pitch, lead=lead) if dst_pitch else None     # (byte stores / dword stores / no image)
            st = GuardedStats(1) if around != 0xC3 else None                              # (stats / no stats / stats only)
            eng.check(lib.ofx_motion_compensate(p.ptr, p.pitch, q.ptr, q.pitch, w, h, tf.data_ptr(), uvp, float(scale),
                                                img.ptr if img else None, dst_pitch, st.ring.data_ptr() if st else None, eng._stream_ptr()),
                      "ofx_motion_compensate")
            runs.append((around, img, st))
        torch.cuda.synchronize()
        for around, img, st in runs:
            what = f"{name} (surroundings {around:#x})"
            if img:
                got, clean = img.host()
                same(got[0], want_mc, f"{what}: mc")
                assert clean, f"{what}: bytes outside the image's pixels were written"
            if st:
                got, clean = st.host()
                same(got[0], want_st, f"{what}: stats")
                assert clean, f"{what}: words around the stats were written"
        n += 1
    assert n == 8 * len(R.FLOW_KINDS)


def test_engine_helper_equals_the_two_launches(eng):
    w, h = 257, 40
    prev1, next1 = R.planes(w, h, 3)
    flow, scale = R.flow_case("nonfinite", w, h, 3)
    for uv in (None, (3.7, -2.2)):
        mc, st = eng.motion_compensate(prev1, next1, flow, uv, float(scale))
        sh = next1 if uv is None else eng.shift_1ch(next1, uv)
        want = eng.warp_u8(sh, flow, float(scale))
        same(mc, want, f"uv {uv}: mc vs shift_1ch + warp_u8")
        same(st, R.sums(prev1, next1, want, R.warp(sh, flow, scale)[1]), f"uv {uv}: stats")
        assert st[3] > 0


# ---- 2. the stream stage --------------------------------------------------------------------------------------------------------

SIZES = [(256, 64), (136, 72)]
LEVELS, NF = 3, 11    # 2 B + 3 frames at B = 4


@functools.lru_cache(maxsize=None)
def _clip(kind, w, h):
    if kind == "smooth":
        return tuple(synth.smooth_pair(w, h, 1.2 * i, -0.6 * i, seed=41)[1] for i in range(NF))
    out = []
    for i in range(NF):     # uniform noise with flat patches: windows without gradient, a NaN flow there
        f = synth.random_pair(w, h, seed=50 + i)[0]
        f[8:40, 16:56] = 128
        f[h - 20:, w - 30:] = 7
        out.append(f)
    return tuple(out)


def _frames(clip, w, pitch):
    import torch

    out = []
    for f in clip:
        buf = torch.full((f.shape[0], pitch), FILL, dtype=torch.uint8, device="cuda")
        buf[:, :w] = torch.from_numpy(f).cuda()
        out.append(buf[:, :w])
    return out


_REF = {}


def _reference(eng, kind, w, h, win, mode, iters):
    """Per pair and level (0, 1): (mc, stats) by the two existing launches on what a pair-at-a-time session holds."""
    import torch

    key = (kind, w, h, win, mode, iters)
    if key in _REF:
        return _REF[key]
    frames = _frames(_clip(kind, w, h), w, eng.pitch_for(w))
    s = eng.Session(w, h, LEVELS, win, mode, iters=iters)
    s.set_frame_device(frames[0]); s.build_pyramid(); s.swap()
    want = {}
    for p in range(1, NF):
        s.set_frame_device(frames[p]); s.build_pyramid(); s.run_flow()
        torch.cuda.synchronize()
        for lv in (0, 1):
            wl = w >> lv
            flow = s.flow_host(lv)
            prev1, next1 = (s.plane(i, lv)[0][:, :wl].cpu().numpy() for i in (0, 1))
            sh = eng.shift_1ch(next1, s.uv(lv).cpu().numpy()) if lv < LEVELS - 1 else next1
            mc = eng.warp_u8(sh, flow, eng.ITER_SCALE)
            want[p, lv] = (mc, R.sums(prev1, next1, mc, R.warp(sh, flow, eng.ITER_SCALE)[1]), flow)
        s.swap()
    s.close()
    _REF[key] = want
    return want


def _configs():
    out, i = [], 0
    for iters in (1, 2, 3, 4):
        for B in (1, 2, 4):
            for kind in ("copied", "borrowed"):
                size = SIZES[(i + iters) % 2]
                win = (5, 9)[(i // 2 + B) % 2]
                level = (i // 3 + iters) % 2
                mode = ("lk_float", "lk_float_fast")[(i // 5) % 2]
                clip = "random" if i % 5 == 3 else "smooth"
                out.append((iters, B, kind, size[0], size[1], win, level, mode, clip))
                i += 1
    return out


def test_the_configs_cover_every_value():
    cfg = _configs()
    for col, values in ((0, (1, 2, 3, 4)), (1, (1, 2, 4)), (2, ("copied", "borrowed")), (3, (256, 136)), (5, (5, 9)), (6, (0, 1)),
                        (7, ("lk_float", "lk_float_fast")), (8, ("smooth", "random"))):
        assert {c[col] for c in cfg} == set(values)
        for col2, values2 in ((0, (1, 2, 3, 4)), (1, (1, 2, 4)), (2, ("copied", "borrowed"))):
            if col > 2 and col != 8:
                for v in values:
                    assert {c[col2] for c in cfg if c[col] == v} == set(values2), (col, v, col2)


def _session(eng, w, h, win, mode, iters, B, kind):
    borrow = kind == "borrowed"
    return eng.Session(w, h, LEVELS, win, mode, iters=iters, stream_batch=B, borrow_frames=borrow, two_stage=borrow)


def _run(s, frames, on_done):
    s.stream_begin()
    for f in frames:
        d = s.stream_submit(f)
        if d >= 1:
            on_done(d)
    while True:
        d = s.stream_drain()
        if d == -2:
            return
        if d >= 1:
            on_done(d)


@pytest.mark.parametrize("cfg", _configs(), ids=lambda c: "-".join(map(str, c)))
def test_stream_stage_equals_the_two_launches_on_the_plain_session(eng, cfg):
    import torch

    iters, B, kind, w, h, win, level, mode, clipkind = cfg
    want = _reference(eng, clipkind, w, h, win, mode, iters)
    nf = 2 * B + 3
    wl, hl = w >> level, h >> level
    # borrowed frames at iters = 1 may have any pitch that is a multiple of 4: two different ones over the configs
    pitch = eng.pitch_for(w) if iters > 1 or kind == "copied" else (w + 3) // 4 * 4 + (8 if B != 2 else 24)
    frames = _frames(_clip(clipkind, w, h)[:nf], w, pitch)
    s = _session(eng, w, h, win, mode, iters, B, kind)
    # a ring of exactly B slots (they wrap), rows padded, slots on a padded stride
    rp = (wl + 3) // 4 * 4 + 4
    img = GuardedImage(B, hl, wl, rp, stride=(hl * rp + 15) // 16 * 16 + 48)
    st = GuardedStats(B)
    s.stream_motion(img.ring, st.ring, level)
    seen, nan_pairs = 0, 0

    def on_done(d):
        nonlocal seen, nan_pairs
        torch.cuda.synchronize()
        assert 1 <= d - seen <= B
        got_img, clean = img.host()
        got_st, clean_st = st.host()
        assert clean and clean_st, f"after pair {d}: bytes outside the slots' pixels / stats were written"
        for p in range(seen + 1, d + 1):
            mc, sums, flow = want[p, level]
            same(s.flow_of(p, level)[0].cpu().numpy(), flow, f"pair {p}: the flow itself")
            same(got_img[(p - 1) % B], mc, f"pair {p}: ring slot")
            same(got_st[(p - 1) % B], sums, f"pair {p}: stats slot")
            view, sv = s.motion_of(p)
            same(view.cpu().numpy(), mc, f"motion_of({p})")
            same(sv.cpu().numpy(), sums, f"motion_of({p}) stats")
            nan_pairs += int(sums[3] > 0)
        for p in (0, d - B, d + 1):
            with pytest.raises(eng.OfxError, match=r"code 1"):
                s.motion_of(p)
        seen = d

    _run(s, frames, on_done)
    assert seen == nf - 1
    if clipkind == "random":
        assert nan_pairs > 0, "the flat patches were meant to give NaN flows"
    s.close()


def test_image_only_and_stats_only_and_a_second_stream_with_another_pitch(eng):
    import torch

    w, h, win, B, level = 136, 72, 9, 2, 0
    want = _reference(eng, "smooth", w, h, win, "lk_float", 1)
    nf = 2 * B + 3
    for ring_on, stats_on in ((True, False), (False, True)):
        s = _session(eng, w, h, win, "lk_float", 1, B, "borrowed")
        img = GuardedImage(nf - 1, h, w, 140) if ring_on else None
        st = GuardedStats(nf - 1) if stats_on else None
        s.stream_motion(img.ring if img else None, st.ring if st else None, level)
        for pitch in (144, 160):        # the setting stays in effect; the second stream's frames have another pitch
            _run(s, _frames(_clip("smooth", w, h)[:nf], w, pitch), lambda d: None)
            torch.cuda.synchronize()
            view, sv = s.motion_of(nf - 1)
            assert (view is None) == (not ring_on) and (sv is None) == (not stats_on)
            if img:
                got, clean = img.host()
                assert clean
                for p in range(1, nf):
                    same(got[p - 1], want[p, level][0], f"image only, pitch {pitch}: pair {p}")
                img.ring.fill_(0)
            if st:
                got, clean = st.host()
                assert clean
                for p in range(1, nf):
                    same(got[p - 1], want[p, level][1], f"stats only, pitch {pitch}: pair {p}")
                st.ring.fill_(-1)
        s.close()


def test_with_the_compose_ring_and_arrows_on_all_three_are_unchanged(eng):
    import torch

    w, h, win, B, level, iters = 256, 64, 9, 4, 0, 3
    nf = 2 * B + 3
    frames = _frames(_clip("smooth", w, h)[:nf], w, eng.pitch_for(w))
    _, ny, nx = eng.arrow_grid(w, h, 30)

    def run(compose, arrows, motion):
        s = _session(eng, w, h, win, "lk_float", iters, B, "borrowed")
        out = {}
        if compose:
            out["compose"] = torch.full((nf - 1, h, w, 2), 7.0, dtype=torch.float32, device="cuda")
            s.stream_compose(out["compose"], level)
        if arrows:
            out["arrows"] = torch.full((nf - 1, ny, nx, 4), 7, dtype=torch.int32, device="cuda")
            s.stream_arrows(out["arrows"], level, 30)
        if motion:
            out["img"], out["st"] = GuardedImage(nf - 1, h, w, w + 4), GuardedStats(nf - 1)
            s.stream_motion(out["img"].ring, out["st"].ring, level)
        _run(s, frames, lambda d: None)
        torch.cuda.synchronize()
        s.close()
        return out

    both, c, a, m = run(True, True, True), run(True, False, False), run(False, True, False), run(False, False, True)
    assert torch.equal(both["compose"].view(torch.int32), c["compose"].view(torch.int32)), "compose ring: with the motion stage vs alone"
    assert torch.equal(both["arrows"], a["arrows"]), "arrows: with the motion stage vs alone"
    (gi, ci), (gs, cs) = both["img"].host(), both["st"].host()
    (wi, _), (ws, _) = m["img"].host(), m["st"].host()
    assert ci and cs
    same(gi, wi, "motion image: all on vs alone")
    same(gs, ws, "motion stats: all on vs alone")
    want = _reference(eng, "smooth", w, h, win, "lk_float", iters)
    for p in range(1, nf):
        same(gi[p - 1], want[p, level][0], f"pair {p}: image")
        same(gs[p - 1], want[p, level][1], f"pair {p}: stats")


def test_refusals(eng):
    import torch
    from cuda_optical_flow_2_amd.parallel import ShardPlan

    w, h, L, win, B = 320, 240, 3, 7, 4
    s = eng.Session(w, h, L, win, "lk_float", stream_batch=B)
    lib, hd = s.L, s._h
    ring = torch.zeros(2 * B * h * 336 + 64, dtype=torch.uint8, device="cuda")
    stats = torch.zeros((2 * B + 1, 4), dtype=torch.int64, device="cuda")
    base, sb, slot = ring.data_ptr(), stats.data_ptr(), h * 320
    sc = eng.ITER_SCALE
    out, pitch, so = _vp(), C.c_int(), _vp()
    assert lib.ofx_session_motion_of(hd, 1, C.byref(out), C.byref(pitch), C.byref(so)) == 4    # the stage is off
    assert lib.ofx_session_stream_motion(hd, L, sc, base, 320, slot, B, sb) == 1              # level out of range
    assert lib.ofx_session_stream_motion(hd, -1, sc, base, 320, slot, B, sb) == 1
    assert lib.ofx_session_stream_motion(hd, 0, sc, base, 316, slot, B, sb) == 1              # pitch below the width
    assert lib.ofx_session_stream_motion(hd, 0, sc, base, 322, h * 322 + 14, B, sb) == 1      # pitch not a multiple of 4
    assert lib.ofx_session_stream_motion(hd, 0, sc, base + 8, 320, slot, B, sb) == 1          # ring not 16-byte aligned
    assert lib.ofx_session_stream_motion(hd, 0, sc, base, 320, slot + 8, B, sb) == 1          # stride not a multiple of 16
    assert lib.ofx_session_stream_motion(hd, 0, sc, base, 320, slot - 16, B, sb) == 1         # stride shorter than a slot
    assert lib.ofx_session_stream_motion(hd, 0, sc, base, 320, slot, B - 1, sb) == 1          # fewer slots than stream_batch
    assert lib.ofx_session_stream_motion(hd, 0, sc, None, 0, 0, B - 1, sb) == 1               # ... stats only, too
    assert lib.ofx_session_stream_motion(hd, 0, sc, base, 320, slot, B, sb + 4) == 1          # stats not 8-byte aligned
    assert lib.ofx_session_motion_of(hd, 1, None, None, None) == 4                             # nothing was set by any of those
    assert lib.ofx_session_stream_motion(hd, 1, sc, base, 160, 120 * 160, B, sb) == 0         # level 1: its own width and rows
    assert lib.ofx_session_stream_motion(hd, 0, sc, base, 320, slot, B, sb) == 0
    assert lib.ofx_session_motion_of(hd, 1, None, None, None) == 1                             # on, but no pair yet
    s.stream_begin()
    assert lib.ofx_session_stream_motion(hd, 0, sc, base, 320, slot, B, sb) == 0              # right after stream_begin: still allowed
    frames = _frames([synth.smooth_pair(w, h, 1.0 * i, 0.5 * i, seed=5)[1] for i in range(3)], w, w)
    s.stream_submit(frames[0])
    assert lib.ofx_session_stream_motion(hd, 0, sc, base, 320, slot, B, sb) == 4              # once the stream has frames
    assert lib.ofx_session_stream_motion(hd, 0, sc, None, 0, 0, 0, None) == 4
    for f in frames[1:]:
        s.stream_submit(f)
    while s.stream_drain() != -2:
        pass
    torch.cuda.synchronize()
    assert lib.ofx_session_motion_of(hd, 2, C.byref(out), C.byref(pitch), C.byref(so)) == 0
    assert out.value == base + slot and pitch.value == 320 and so.value == sb + 32
    assert stats[:2, 0].tolist() == [w * h, w * h] and int(stats[2:].abs().sum()) == 0
    s.stream_motion(None, None)                                                                 # between streams: off again
    assert lib.ofx_session_motion_of(hd, 1, None, None, None) == 4
    s.close()
    # sharded sessions and partial frames: unsupported
    plan = ShardPlan(w, h, L, win, 0, 2)
    s = eng.Session(w, h, L, win, "lk_float", shard=plan, local_corner=True, stream_batch=2)
    assert s.L.ofx_session_stream_motion(s._h, 0, sc, base, 320, slot, B, sb) == 3
    assert s.L.ofx_session_stream_motion(s._h, 0, sc, None, 0, 0, 0, None) == 0                # turning it off is no request
    s.close()
    s = eng.Session(w, h, L, win, "lk_float", shard=plan, local_corner=True, stream_batch=2, borrow_frames=True, frames_partial=True)
    assert s.L.ofx_session_stream_motion(s._h, 0, sc, base, 320, slot, B, sb) == 3
    s.close()


# ---- 3. the clip call -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("level,iters", [(0, 1), (1, 3)])
def test_video_motion_equals_the_per_pair_results(eng, level, iters):
    import torch

    w, h, win = 256, 64, 9
    want = _reference(eng, "smooth", w, h, win, "lk_float", iters)
    clip = torch.from_numpy(np.stack(_clip("smooth", w, h))).cuda()
    got = {}
    for batch in (1, 4):
        mc, st = eng.video_motion(clip, LEVELS, win, level=level, iters=iters, batch=batch)
        assert mc.dtype == torch.uint8 and tuple(mc.shape) == (NF - 1, h >> level, w >> level)
        assert st.dtype == torch.int64 and tuple(st.shape) == (NF - 1, 4)
        got[batch] = (mc.cpu().numpy(), st.cpu().numpy())
        for p in range(1, NF):
            same(got[batch][0][p - 1], want[p, level][0], f"batch {batch}: pair {p}: image")
            same(got[batch][1][p - 1], want[p, level][1], f"batch {batch}: pair {p}: stats")
    same(got[4][0], got[1][0], "B = 4 vs B = 1: images")
    same(got[4][1], got[1][1], "B = 4 vs B = 1: stats")
    # the flow does its job on a translating texture: the compensated error is below the raw one
    assert (got[1][1][:, 2] < got[1][1][:, 1]).all()
