"""GPU: the stream pipeline's output stage -- the composed dense field (main.cu:138-147) of every pair the pipeline completes,
written by one batched launch per completing call into a ring the caller owns (ofx_session_stream_compose), and
engine.video_flow on top of it.  The referee is oracle.compose_flow of the plain pair-at-a-time flows, bit for bit."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_same
from cuda_optical_flow_2_amd import synth

pytestmark = pytest.mark.gpu

GUARD = 64  # floats of 0x5A guard before and after every ring


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cuda_optical_flow_2_amd import engine

    return engine


def _frames(w, h, nf, pitch, seed=41):
    import torch

    out = []
    for i in range(nf):
        buf = torch.full((h, pitch), 0x5A, dtype=torch.uint8, device="cuda")
        buf[:, :w] = torch.from_numpy(synth.smooth_pair(w, h, 1.2 * i, -0.6 * i, seed=seed)[1]).cuda()
        out.append(buf[:, :w])
    return out


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


class Ring:
    """n slots of [rows, w, 2] float32 with `pad` floats of padding after each slot (beyond the 16-byte rounding) and GUARD
    floats before and after, all filled with 0x5A bytes."""

    def __init__(self, n, rows, w, pad=0):
        import torch

        self.slot = rows * w * 2
        self.stride = (self.slot + 3) // 4 * 4 + pad
        self.flat = torch.empty(2 * GUARD + n * self.stride, dtype=torch.float32, device="cuda")
        self.flat.view(torch.uint8).fill_(0x5A)
        self.ring = self.flat.as_strided((n, rows, w, 2), (self.stride, 2 * w, 2, 1), GUARD)
        self.outside = np.ones(self.flat.numel(), bool)
        for i in range(n):
            self.outside[GUARD + i * self.stride:GUARD + i * self.stride + self.slot] = False

    def check_guards(self, what):
        raw = self.flat.cpu().numpy().view(np.uint32)
        bad = np.flatnonzero(self.outside & (raw != 0x5A5A5A5A))
        assert bad.size == 0, f"{what}: {bad.size} guard / padding words overwritten, first at {bad[:4].tolist()}"


def _drive(sessions, frames, on_done):
    """Feed every frame to every session (lock-step), then drain; on_done(pair) after each call that completed pairs."""
    for f in frames:
        d = {s.stream_submit(f) for s in sessions}
        assert len(d) == 1
        d = d.pop()
        if d >= 1:
            on_done(d)
    while True:
        d = {s.stream_drain() for s in sessions}
        assert len(d) == 1
        d = d.pop()
        if d == -2:
            return
        if d >= 1:   # (a drain tick may complete nothing: -1)
            on_done(d)


def _compose_flow_of(eng, s, pair, L, level, w, rows):
    """ofx_compose_flow on the pair's flow_of pointers (the existing per-pair route), into a fresh tensor."""
    import torch

    lib = eng._lib.load()
    ptrs = (C.c_void_p * eng._lib.OFX_MAX_LEVELS)()
    for k in range(level, L):
        ptrs[k] = s.flow_of(pair, k)[0].data_ptr()
    out = torch.empty((rows, w, 2), dtype=torch.float32, device="cuda")
    eng.check(lib.ofx_compose_flow(ptrs, w, rows, L, level, out.data_ptr(), eng._stream_ptr()), "ofx_compose_flow")
    return out


# (w, h, levels, window, mode, iters, frames, B, frame kind)
CONFIGS = [
    (640, 480, 3, 7, "lk_float", 1, 11, 1, "copied"),
    (640, 480, 4, 7, "compat_cpu", 1, 13, 2, "borrowed"),
    (1000, 564, 3, 9, "lk_float", 1, 19, 8, "two_stage"),          # coarsest 250 x 141
    (1000, 568, 4, 7, "compat_cpu", 1, 21, 16, "copied"),          # coarsest 125 x 71: a 71 000-byte slot, padded stride
    (1000, 568, 4, 9, "lk_float_fast", 3, 12, 8, "two_stage"),
    (640, 480, 4, 7, "lk_float", 3, 10, 2, "copied"),
    (1000, 564, 3, 7, "lk_float_fast", 1, 9, 4, "borrowed"),
    (320, 240, 3, 5, "lk_float", 1, 37, 16, "two_stage"),          # more than two ticks of sixteen, 36 not a multiple of B
]


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "-".join(map(str, c)))
def test_slots_equal_the_oracle_composition_of_the_plain_path(eng, oracle, cfg):
    import torch

    w, h, L, win, mode, iters, nf, B, kind = cfg
    borrow, two = kind != "copied", kind == "two_stage"
    pitch = eng.pitch_for(w) if iters > 1 else (w + 3) // 4 * 4 + 8
    frames = _frames(w, h, nf, pitch)
    want = _plain(eng, frames, w, h, L, win, mode, iters)
    levels = sorted({0, 1, L - 1})
    sess, rings = [], []
    for lv in levels:
        s = eng.Session(w, h, L, win, mode, iters=iters, stream_batch=B, borrow_frames=borrow, two_stage=two)
        r = Ring(nf - 1, h >> lv, w >> lv, pad=4 * lv)
        s.stream_compose(r.ring, lv)
        s.stream_begin()
        sess.append(s)
        rings.append(r)
    via_flow_of = {}
    seen = 0

    def on_done(d):
        nonlocal seen
        for p in range(seen + 1, d + 1):
            via_flow_of[p] = [_compose_flow_of(eng, s, p, L, lv, w >> lv, h >> lv) for s, lv in zip(sess, levels)]
        seen = d

    _drive(sess, frames, on_done)
    torch.cuda.synchronize()
    assert seen == nf - 1
    for i, lv in enumerate(levels):
        got = rings[i].ring.cpu().numpy()
        for p in range(1, nf):
            ref = oracle.compose_flow(want[p], L, lv)
            assert_same(got[p - 1], ref, f"{kind} B={B} pair {p} level {lv}")
            assert_same(sess[i].composed_of(p).cpu().numpy(), ref, f"composed_of({p}) level {lv}")
            assert_same(via_flow_of[p][i].cpu().numpy(), ref, f"ofx_compose_flow of flow_of({p}) level {lv}")
        rings[i].check_guards(f"level {lv}")
    for s in sess:
        s.close()


@pytest.mark.parametrize("extra", [0, 1, "3B"])
def test_ring_wraps_and_stays_in_bounds(eng, oracle, extra):
    """A ring shorter than the stream: slot (p - 1) mod n_slots, read when the pair is reported; nothing outside the slots
    (guards, the padding of a stride larger than the slot) is touched."""
    import torch

    w, h, L, win, B, nf = 320, 240, 3, 7, 4, 31
    n_slots = 3 * B if extra == "3B" else B + extra
    frames = _frames(w, h, nf, (w + 3) // 4 * 4 + 8, seed=7)
    want = _plain(eng, frames, w, h, L, win, "lk_float")
    s = eng.Session(w, h, L, win, "lk_float", stream_batch=B, borrow_frames=True, two_stage=True)
    r = Ring(n_slots, h, w, pad=12)
    s.stream_compose(r.ring, 0)
    s.stream_begin()
    checked, seen = [], 0

    def on_done(d):
        nonlocal seen
        torch.cuda.synchronize()
        for p in range(seen + 1, d + 1):
            got = s.composed_of(p).cpu().numpy()
            assert_same(got, oracle.compose_flow(want[p], L, 0), f"n_slots {n_slots}: pair {p}")
            assert_same(r.ring[(p - 1) % n_slots].cpu().numpy(), got, f"slot of pair {p}")
            checked.append(p)
        seen = d

    _drive([s], frames, on_done)
    assert checked == list(range(1, nf))
    r.check_guards(f"n_slots {n_slots}")
    s.close()


@pytest.mark.parametrize("iters,level", [(1, 0), (1, 1), (3, 0)])
def test_sharded_ranks_compose_their_own_rows(eng, oracle, iters, level):
    """Four logical ranks (row shards, local corner flows): each composes its own rows; stacked, they are the unsharded field."""
    import torch
    from cuda_optical_flow_2_amd.parallel import ShardPlan

    w, h, L, win, R, B, nf = 640, 480, 4, 7, 4, 2, 8
    frames = _frames(w, h, nf, eng.pitch_for(w), seed=29)
    want = _plain(eng, frames, w, h, L, win, "lk_float", iters)
    ranks, rings = [], []
    for r in range(R):
        plan = ShardPlan(w, h, L, win, r, R, iters=iters)
        s = eng.Session(w, h, L, win, "lk_float", shard=plan, local_corner=True, stream_batch=B, iters=iters)
        rows = plan.own[level][1] - plan.own[level][0]
        ring = Ring(nf - 1, rows, w >> level)
        s.stream_compose(ring.ring, level)
        s.stream_begin()
        ranks.append(s)
        rings.append(ring)
    _drive(ranks, frames, lambda d: None)
    torch.cuda.synchronize()
    for p in range(1, nf):
        full = np.concatenate([rg.ring[p - 1].cpu().numpy() for rg in rings], axis=0)
        assert_same(full, oracle.compose_flow(want[p], L, level), f"{R} ranks iters={iters}: pair {p} level {level}")
    for rg in rings:
        rg.check_guards("rank ring")
    for s in ranks:
        assert s.corner_status() == 0
        s.close()


def test_sharded_plan_breaking_the_own_row_rule_is_refused(eng):
    import torch
    from cuda_optical_flow_2_amd.parallel import ShardPlan

    w, h, L, win = 640, 480, 4, 7
    plan = ShardPlan(w, h, L, win, 1, 4)
    c0, c1 = plan.own[L - 1]
    plan.own[L - 1] = (c0, c1 - 1)   # level 0's last own rows would read a coarsest row this rank does not compute
    s = eng.Session(w, h, L, win, "lk_float", shard=plan, local_corner=True, stream_batch=2)
    rows = plan.own[0][1] - plan.own[0][0]
    ring = torch.zeros((2, rows, w, 2), dtype=torch.float32, device="cuda")
    with pytest.raises(eng.OfxError, match=r"code 3"):
        s.stream_compose(ring, 0)
    # level L - 1 reads nothing coarser: allowed
    s.stream_compose(torch.zeros((2, c1 - 1 - c0, w >> (L - 1), 2), dtype=torch.float32, device="cuda"), L - 1)
    s.close()


def test_off_by_default_and_one_launch_per_completing_call(eng):
    import torch

    w, h, L, win, B, nf = 640, 480, 4, 7, 4, 15
    frames = _frames(w, h, nf, (w + 3) // 4 * 4 + 8, seed=3)
    off = eng.Session(w, h, L, win, "lk_float", stream_batch=B, borrow_frames=True, two_stage=True)
    on = eng.Session(w, h, L, win, "lk_float", stream_batch=B, borrow_frames=True, two_stage=True)
    ring = torch.empty((nf - 1, h, w, 2), dtype=torch.float32, device="cuda")
    on.stream_compose(ring, 0)
    for s in (off, on):
        s.timing(1000)
        s.stream_begin()
    calls = 0
    seen = 0

    def on_done(d):
        nonlocal calls, seen
        calls += 1
        for p in range(seen + 1, d + 1):
            for k in range(L):
                assert_same(on.flow_of(p, k)[0].cpu().numpy(), off.flow_of(p, k)[0].cpu().numpy(), f"pair {p} level {k}")
        seen = d

    _drive([off, on], frames, on_done)
    torch.cuda.synchronize()
    assert seen == nf - 1 and calls >= 2
    assert off.timing_read_kind("compose")[2] == 0
    assert on.timing_read_kind("compose")[2] == calls
    # the dominant set (ofx_session_timing_read) leaves the compose launches out: both count the same launches
    assert off.timing_read()[2] == on.timing_read()[2]
    off.close()
    on.close()


def test_argument_and_state_errors(eng):
    import torch

    w, h, L, win, B = 320, 240, 3, 7, 4
    s = eng.Session(w, h, L, win, "lk_float", stream_batch=B)
    lib, hd = s.L, s._h
    buf = torch.zeros(2 * (8 * h * w * 2) + 64, dtype=torch.float32, device="cuda")
    base, slot = buf.data_ptr(), h * w * 8
    assert lib.ofx_session_stream_compose(hd, 0, base + 4, slot + 16, B) == 1      # ring not 16-byte aligned
    assert lib.ofx_session_stream_compose(hd, 0, base, slot + 8, B) == 1          # stride not a multiple of 16
    assert lib.ofx_session_stream_compose(hd, 0, base, slot - 16, B) == 1         # stride shorter than a slot
    assert lib.ofx_session_stream_compose(hd, 0, base, slot, B - 1) == 1          # fewer slots than stream_batch
    assert lib.ofx_session_stream_compose(hd, L, base, slot, B) == 1              # level out of range
    assert lib.ofx_session_stream_compose(hd, -1, base, slot, B) == 1
    assert b"slots" in lib.ofx_last_error() or b"level" in lib.ofx_last_error()
    out = C.c_void_p()
    assert lib.ofx_session_composed_of(hd, 1, C.byref(out), None, None) == 4      # no ring
    ring = buf[:B * h * w * 2].view(B, h, w, 2)
    s.stream_compose(ring, 0)
    s.stream_begin()
    frames = _frames(w, h, 2 * B + 2, w, seed=5)
    s.stream_submit(frames[0])
    assert lib.ofx_session_stream_compose(hd, 0, base, slot, B) == 4              # the stream has a frame already
    assert lib.ofx_session_stream_compose(hd, 0, None, 0, 0) == 4
    last = -1
    for f in frames[1:]:
        last = max(last, s.stream_submit(f))
    while True:
        d = s.stream_drain()
        if d == -2:
            break
        last = max(last, d)
    assert last == 2 * B + 1
    assert lib.ofx_session_composed_of(hd, last, C.byref(out), None, None) == 0
    assert lib.ofx_session_composed_of(hd, last - B, C.byref(out), None, None) == 1   # overwritten by pair last
    assert lib.ofx_session_composed_of(hd, last + 1, C.byref(out), None, None) == 1
    assert lib.ofx_session_composed_of(hd, 0, C.byref(out), None, None) == 1
    with pytest.raises(eng.OfxError):
        s.composed_of(1)
    # between streams the ring may be changed again, and turned off
    s.stream_compose(None)
    s.close()


@pytest.mark.parametrize("iters", [1, 5])
@pytest.mark.parametrize("size,levels,layout", [((640, 480), 4, "contiguous"), ((640, 480), 4, "wide_pitch"), ((1000, 564), 3, "contiguous"),
                                                ((1000, 564), 3, "odd_pitch")])
@pytest.mark.parametrize("N", [2, 7, 20])
def test_video_flow_equals_the_oracle(eng, oracle, N, size, levels, layout, iters):
    import torch

    w, h = size
    win = 9
    # contiguous / wide_pitch: read in place, or (iters > 1 and a pitch other than the width rounded up to 64) copied by the
    # session; odd_pitch: not 4-byte aligned rows, copied into a pitched buffer first
    pitch = {"contiguous": w, "wide_pitch": w + 64, "odd_pitch": w + 1}[layout]
    store = torch.full((N, h, pitch), 0x5A, dtype=torch.uint8, device="cuda")
    for i in range(N):
        store[i, :, :w] = torch.from_numpy(synth.smooth_pair(w, h, 0.9 * i, 0.5 * i, seed=17)[1]).cuda()
    clip = store[:, :, :w]
    got = eng.video_flow(clip, levels, win, iters=iters).cpu().numpy()
    assert got.shape == (N - 1, h, w, 2)
    want = _plain(eng, [clip[i] for i in range(N)], w, h, levels, win, "lk_float", iters)
    for p in range(1, N):
        assert_same(got[p - 1], oracle.compose_flow(want[p], levels, 0), f"video_flow {layout} N={N} iters={iters}: pair {p}")


def test_video_flow_level_with_a_padded_slot(eng, oracle):
    """Level 3 of 1000 x 568 is 125 x 71: 71 000-byte slots, so the result is a view of a padded buffer."""
    import torch

    w, h, L, N = 1000, 568, 4, 6
    clip = torch.stack([torch.from_numpy(synth.smooth_pair(w, h, 1.1 * i, -0.4 * i, seed=23)[1]).cuda() for i in range(N)])
    got = eng.video_flow(clip, L, 7, level=L - 1)
    assert tuple(got.shape) == (N - 1, h >> 3, w >> 3, 2) and got.stride(0) % 4 == 0
    want = _plain(eng, [clip[i] for i in range(N)], w, h, L, 7, "lk_float")
    got = got.cpu().numpy()
    for p in range(1, N):
        assert_same(got[p - 1], oracle.compose_flow(want[p], L, L - 1), f"level {L - 1}: pair {p}")


def test_video_flow_one_4k_tick_of_the_benchmarked_configuration(eng, oracle):
    """bench.py's configuration (5 levels, 9 x 9, five iterations, eight pairs per tick): one tick's worth of pairs."""
    import torch

    w, h, L, win, iters, B, N = 3840, 2160, 5, 9, 5, 8, 9
    clip = torch.stack([torch.from_numpy(synth.smooth_pair(w, h, 1.3 * i, 0.7 * i, seed=11)[1]).cuda() for i in range(N)])
    got = eng.video_flow(clip, L, win, iters=iters, batch=B)
    picks = [1, 4, 8]
    for p in picks:
        want = _plain(eng, [clip[p - 1], clip[p]], w, h, L, win, "lk_float", iters)[1]
        assert_same(got[p - 1].cpu().numpy(), oracle.compose_flow(want, L, 0), f"4K pair {p}")
