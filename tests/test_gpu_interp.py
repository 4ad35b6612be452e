"""GPU: the pixel displacement -- the stateless launch (ofx_flow_displacement) and the stream pipeline's stage
(ofx_session_stream_displacement) -- and frame interpolation -- the stateless launch (ofx_interpolate_frames), the batched one
(ofx_interpolate_frames_batch) and engine.video_interpolate -- against tests/interp_ref.py.  Every comparison is exact, floats by
their bits.  Outputs sit in buffers of 0x5A, inputs in larger buffers whose surroundings differ between runs, so that a tap outside
an input, or a store outside an output, shows."""
import ctypes as C
import functools

import numpy as np
import pytest

import interp_ref as R

pytestmark = pytest.mark.gpu

_vp = C.c_void_p
FILL = 0x5A
FILL64 = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cuda_optical_flow_2_amd import engine

    return engine


def same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype}{got.shape} vs {want.dtype}{want.shape}"
    a, b = (got.view(np.uint32), want.view(np.uint32)) if got.dtype == np.float32 else (got, want)   # (floats by their bits)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        raise AssertionError(f"{what}: {len(bad)}/{got.size} differ, first at {bad[:3].tolist()}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}")


class Field:
    """A [h, w, 2] float32 field inside a larger buffer: `lead` floats before it (even: 8-byte aligned; a multiple of 4: 16-byte)
    and 64 after it, all holding the bit pattern `around`."""

    def __init__(self, arr, lead, around):
        import torch

        assert lead % 2 == 0
        host = np.full(lead + arr.size + 64, around, np.uint32)
        host[lead:lead + arr.size] = np.ascontiguousarray(arr, np.float32).reshape(-1).view(np.uint32)
        self.t = torch.from_numpy(host.view(np.int32)).cuda()
        self.ptr = self.t.data_ptr() + 4 * lead


class Plane:
    """A [h, w] uint8 plane with rows `pitch` bytes apart inside a larger buffer: `lead` bytes before it, `trail` (64) after its
    last row, and the pad columns of every row, all holding the byte `around`."""

    def __init__(self, arr, pitch, lead, around, trail=64):
        import torch

        h, w = arr.shape
        assert pitch >= w
        host = np.full(lead + h * pitch + trail, around, np.uint8)
        np.lib.stride_tricks.as_strided(host[lead:], (h, w), (pitch, 1))[...] = arr
        self.t = torch.from_numpy(host).cuda()
        self.ptr, self.pitch = self.t.data_ptr() + lead, pitch


class Guarded:
    """n slots of rows x w items of `dtype`, rows `pitch` items apart, slots `stride` items apart (default: 20 items between a
    slot's end and the next slot), `lead` items before and 64 after, every byte 0x5A."""

    def __init__(self, dtype, n, rows, w, pitch, lead, stride=None):
        import torch

        self.n, self.rows, self.w, self.pitch, self.lead = n, rows, w, pitch, lead
        self.stride = rows * pitch + 20 if stride is None else stride
        self.size = np.dtype(dtype).itemsize
        self.dtype = dtype
        self.flat = torch.full(((lead + n * self.stride + 64) * self.size,), FILL, dtype=torch.uint8, device="cuda")
        self.ptr = self.flat.data_ptr() + lead * self.size

    def slot(self, i):
        return self.ptr + i * self.stride * self.size

    def host(self):
        """(the items [n, rows, w], True when every other byte still holds 0x5A)"""
        raw = self.flat.cpu().numpy().view(self.dtype)
        px = np.lib.stride_tricks.as_strided(raw[self.lead:], (self.n, self.rows, self.w),
                                             (self.stride * self.size, self.pitch * self.size, self.size))
        got = px.copy()
        px[...] = np.frombuffer(bytes([FILL]) * self.size, self.dtype)[0]
        return got, bool((raw.view(np.uint8) == FILL).all())


AROUND_F = [0x7FC00000, 0x7149F2CA, 0x00000000]      # a NaN, 1e30, 0: what surrounds the fields in the three runs
AROUND_P = [0x00, 0xFF, 0x5A]                        # and the planes (their pad columns included)


def _times(times):
    t = np.ascontiguousarray(times, np.float32)
    return t, t.ctypes.data_as(C.POINTER(C.c_float))


# ---- 1. displacement, stateless -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", R.SIZES + [(132, 7)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_displacement_equals_the_referee(eng, size):
    import torch

    lib = eng._lib.load()
    w, h = size
    runs = []
    for ui, uv in enumerate(R.UV_CASES):
        tuv = None if uv is None else torch.tensor(list(uv), dtype=torch.float32, device="cuda")
        for kind in ("iter", "nonfinite"):
            flow = R.flow_case(kind, w, h)
            want = R.displacement(flow, uv, R.ITER_SCALE)
            # (flow lead, dst lead) in floats: both 16-byte aligned; a merely 8-byte aligned destination; a merely 8-byte aligned flow
            for fl, dl in ((4, 4), (4, 2), (2, 4)):
                f = Field(flow, fl, AROUND_F[(ui + fl) % 3])
                d = Guarded(np.float32, 1, h, 2 * w, 2 * w, dl)
                eng.check(lib.ofx_flow_displacement(f.ptr, w, h, None if tuv is None else tuv.data_ptr(), float(R.ITER_SCALE), d.ptr,
                                                    eng._stream_ptr()), "ofx_flow_displacement")
                runs.append((f"{w}x{h} uv {uv} {kind} leads {fl}/{dl}", f, tuv, d, want))
    torch.cuda.synchronize()
    for what, _, _, d, want in runs:
        got, clean = d.host()
        same(got[0].reshape(h, w, 2), want, what)
        assert clean, f"{what}: bytes around the field were written"
    assert len(runs) == len(R.UV_CASES) * 2 * 3


def test_displacement_engine_helper(eng):
    w, h = 257, 40
    flow = R.flow_case("nonfinite", w, h)
    same(eng.flow_displacement(flow, (3.7, -2.2)), R.displacement(flow, (3.7, -2.2), R.ITER_SCALE), "uv (3.7, -2.2)")
    same(eng.flow_displacement(flow), R.displacement(flow, None, R.ITER_SCALE), "no uv")
    same(eng.flow_displacement(flow, (-0.5, 2.0), scale=1.0), R.displacement(flow, (-0.5, 2.0), 1.0), "scale 1")


# ---- 2. interpolation, stateless ------------------------------------------------------------------------------------------------

SHAPES = ["bytes+stats", "dwords", "pitches+stats"]


def _outputs(shape, n_pairs, T, w, h, consecutive_stats=True):
    """(frames, stats) buffers of one of the three output shapes: frames has n_pairs * T slots (a pair's T frames follow each other,
    the slot stride is the time stride), stats n_pairs slots of [T, 4]"""
    st = Guarded(np.int64, n_pairs, T, 4, 4, 4, 4 * T if consecutive_stats else None)
    if shape == "bytes+stats":         # an odd pitch from an odd address, an odd time stride: byte stores
        pitch = (w + 9) | 1
        return Guarded(np.uint8, n_pairs * T, h, w, pitch, 61, h * pitch + 5), st
    if shape == "dwords":              # pitch, address and time stride 4-byte aligned: dword stores; no stats
        pitch = (w + 3) // 4 * 4 + 8
        return Guarded(np.uint8, n_pairs * T, h, w, pitch, 64), None
    return Guarded(np.uint8, n_pairs * T, h, w, w, 16, h * w), st      # tightly packed frames


def _inputs(w, h, kind, seed, run, lead=2):
    """(plane a, plane b, field ab, field ba) on the device for run 0, 1 or 2: a_pitch != b_pitch, both above w, the pad columns
    and the surroundings holding what the run says"""
    a, b = R.planes(w, h, seed)
    dab, dba = R.field_case(kind, w, h, seed)
    ap, bp = ((w + 3, w + 8), (w + 8, w + 4), (w + 13, w + 1))[run]
    return (Plane(a, ap, 3 + run, AROUND_P[run]), Plane(b, bp, 64, AROUND_P[(run + 1) % 3]),
            Field(dab, lead, AROUND_F[run]), Field(dba, lead + 4, AROUND_F[(run + 1) % 3]))


def _launch(eng, inp, w, h, times, frames, stats, slot=0, stats_slot=0):
    lib = eng._lib.load()
    t, tp = _times(times)
    pa, pb, fab, fba = inp
    eng.check(lib.ofx_interpolate_frames(pa.ptr, pa.pitch, pb.ptr, pb.pitch, w, h, fab.ptr, fba.ptr, tp, len(t), frames.slot(slot), frames.pitch,
                                         frames.stride, stats.slot(stats_slot) if stats else None, eng._stream_ptr()), "ofx_interpolate_frames")


def _check(what, frames, stats, want, first=0, T=None, pair=0):
    got, clean = frames.host()
    T = len(want[0]) if T is None else T
    same(got[first:first + T], want[0], f"{what}: frames")
    assert clean, f"{what}: bytes around the frames were written"
    if stats is not None:
        got, clean = stats.host()
        same(got[pair], want[1], f"{what}: stats")
        assert clean, f"{what}: bytes around the stats were written"


@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_stateless_equals_the_referee(eng, size):
    import torch

    w, h = size
    runs = []
    for kind in R.KINDS:
        for ts, times in enumerate(R.TIME_SETS):
            want = R.reference(kind, w, h, ts)
            for si, shape in enumerate(SHAPES):
                # (the surroundings rotate with the kind and the time set: every output shape meets all three patterns)
                inp = _inputs(w, h, kind, 0, (si + R.KINDS.index(kind) + ts) % 3)
                frames, stats = _outputs(shape, 1, len(times), w, h)
                _launch(eng, inp, w, h, times, frames, stats)
                runs.append((f"{w}x{h} {kind} times {ts} ({shape})", inp, frames, stats, want))
    torch.cuda.synchronize()
    for what, _, frames, stats, want in runs:
        _check(what, frames, stats, want)
    assert len(runs) == len(R.KINDS) * len(R.TIME_SETS) * 3


def test_whole_quads_and_16_byte_aligned_fields(eng):
    """132 x 7: every quad is whole, and with the fields 16-byte aligned every field load is an aligned 16-byte load"""
    import torch

    w, h = 132, 7
    runs = []
    for ki, kind in enumerate(("inverse", "nonfinite", "edge", "borders")):
        for si, shape in enumerate(SHAPES):
            inp = _inputs(w, h, kind, 0, (si + ki) % 3, lead=4)      # (every shape meets all three surroundings)
            frames, stats = _outputs(shape, 1, 3, w, h)
            _launch(eng, inp, w, h, R.TIME_SETS[1], frames, stats)
            runs.append((f"{w}x{h} {kind} ({shape})", inp, frames, stats, R.reference(kind, w, h, 1)))
    torch.cuda.synchronize()
    for what, _, frames, stats, want in runs:
        _check(what, frames, stats, want)


def test_engine_helper(eng):
    w, h = 257, 40
    a, b = R.planes(w, h)
    for kind in ("nonfinite", "borders"):
        dab, dba = R.field_case(kind, w, h)
        frames, stats = eng.interpolate_frames(a, b, dab, dba, R.TIME_SETS[2])
        want = R.reference(kind, w, h, 2)
        same(frames, want[0], f"{kind}: frames"); same(stats, want[1], f"{kind}: stats")
    frames, stats = eng.interpolate_frames(a, b, dab, dba, [0.5])
    same(frames, R.reference("borders", w, h, 0)[0], "one time")


# ---- 3. the batched launch ------------------------------------------------------------------------------------------------------

BATCH_KINDS = ["inverse", "borders", "nonfinite"]


def _batch(eng, w, h, pairs, times, shape, slots):
    """pairs: (kind, seed); slots: which slot of the output buffers pair i writes.  Returns (frames, stats)."""
    import torch

    lib = eng._lib.load()
    n, T = len(pairs), len(times)
    inp = [_inputs(w, h, kind, seed, i % 3) for i, (kind, seed) in enumerate(pairs)]
    frames, stats = _outputs(shape, max(slots) + 1, T, w, h, consecutive_stats=tuple(slots) == tuple(range(n)))
    t, tp = _times(times)
    ptrs = lambda f: (_vp * n)(*[f(i) for i in range(n)])
    ints = lambda f: (C.c_int * n)(*[f(i) for i in range(n)])
    eng.check(lib.ofx_interpolate_frames_batch(ptrs(lambda i: inp[i][0].ptr), ints(lambda i: inp[i][0].pitch), ptrs(lambda i: inp[i][1].ptr),
                                               ints(lambda i: inp[i][1].pitch), n, w, h, ptrs(lambda i: inp[i][2].ptr), ptrs(lambda i: inp[i][3].ptr),
                                               tp, T, ptrs(lambda i: frames.slot(slots[i] * T)), frames.pitch, frames.stride,
                                               ptrs(lambda i: stats.slot(slots[i])) if stats else None, eng._stream_ptr()),
              "ofx_interpolate_frames_batch")
    torch.cuda.synchronize()
    return frames, stats


@pytest.mark.parametrize("slots", [(0, 1, 2), (4, 0, 2)], ids=["consecutive", "scattered"])
def test_batch_of_three_kinds_equals_the_single_calls(eng, slots):
    w, h, times = 257, 40, R.TIME_SETS[1]
    T = len(times)
    pairs = [(kind, 0) for kind in BATCH_KINDS]
    a, b = R.planes(w, h)
    singles = [eng.interpolate_frames(a, b, *R.field_case(kind, w, h), times) for kind, _ in pairs]
    for i, (kind, _) in enumerate(pairs):
        want = R.reference(kind, w, h, 1)
        same(singles[i][0], want[0], f"{kind}: the single call's frames"); same(singles[i][1], want[1], f"{kind}: its stats")
    for shape in SHAPES:
        frames, stats = _batch(eng, w, h, pairs, times, shape, slots)
        got_f, clean = frames.host()
        assert clean, f"{shape}: bytes around the frames were written"
        free = sorted(set(range(max(slots) + 1)) - set(slots))
        for i in range(len(pairs)):
            same(got_f[slots[i] * T:(slots[i] + 1) * T], singles[i][0], f"{shape}: pair {i}: frames")
        for s in free:      # a slot no pair writes is left alone
            assert (got_f[s * T:(s + 1) * T] == FILL).all()
        if stats is not None:
            got_s, clean = stats.host()
            assert clean, f"{shape}: bytes around the stats were written"
            for i in range(len(pairs)):
                same(got_s[slots[i]], singles[i][1], f"{shape}: pair {i}: stats")
            assert (got_s[free] == FILL64).all()      # (not even zeroed)


def test_batch_of_sixteen_pairs_at_eight_times(eng):
    w, h, times = 67, 33, R.TIME_SETS[2]
    pairs = [(BATCH_KINDS[i % 3], i // 3) for i in range(16)]
    for shape in SHAPES[:2]:
        frames, stats = _batch(eng, w, h, pairs, times, shape, tuple(range(16)))
        got_f, clean = frames.host()
        assert clean, f"{shape}: bytes around the frames were written"
        got_s = None
        if stats is not None:
            got_s, clean = stats.host()
            assert clean, f"{shape}: bytes around the stats were written"
        for i, (kind, seed) in enumerate(pairs):
            want = R.reference(kind, w, h, 2, seed)
            same(got_f[8 * i:8 * i + 8], want[0], f"{shape}: pair {i} ({kind}, seed {seed}): frames")
            if got_s is not None:
                same(got_s[i], want[1], f"{shape}: pair {i} ({kind}, seed {seed}): stats")


# ---- 4. the stream pipeline's stage ---------------------------------------------------------------------------------------------

W, H, LEVELS, WIN, NF = 128, 96, 3, 9, 6


@functools.lru_cache(maxsize=None)
def _clip():
    import torch
    from cuda_optical_flow_2_amd import synth

    return torch.from_numpy(np.stack([synth.smooth_pair(W, H, 1.2 * i, -0.6 * i, seed=41)[1] for i in range(NF)])).cuda()


@functools.lru_cache(maxsize=None)
def _pairwise(iters):
    """per pair p = 1 .. NF-1 and level: (flow, uv or None) of a plain pair-at-a-time Session, as host arrays"""
    import torch
    from cuda_optical_flow_2_amd import engine

    pitch = engine.pitch_for(W)
    frames = []
    for f in _clip():
        buf = torch.zeros((H, pitch), dtype=torch.uint8, device="cuda")
        buf[:, :W] = f
        frames.append(buf[:, :W])
    s = engine.Session(W, H, LEVELS, WIN, "lk_float", iters=iters)
    s.set_frame_device(frames[0]); s.build_pyramid(); s.swap()
    out = {}
    for p in range(1, NF):
        s.set_frame_device(frames[p]); s.build_pyramid(); s.run_flow()
        torch.cuda.synchronize()
        for lv in range(LEVELS):
            out[p, lv] = (s.flow_host(lv), s.uv(lv).cpu().numpy() if lv < LEVELS - 1 else None)      # (the coarsest level has no shift)
        s.swap()
    s.close()
    return out


@pytest.mark.parametrize("level", [0, 1, 2])
@pytest.mark.parametrize("batch", [1, 2, None])
@pytest.mark.parametrize("iters", [1, 3])
def test_stage_equals_the_referee_on_the_plain_session(eng, iters, batch, level):
    import torch

    want = _pairwise(iters)
    got = eng.video_displacement(_clip(), LEVELS, WIN, level=level, iters=iters, batch=batch)
    assert got.dtype == torch.float32 and tuple(got.shape) == (NF - 1, H >> level, W >> level, 2)
    got = got.cpu().numpy()
    for p in range(1, NF):
        flow, uv = want[p, level]
        same(got[p - 1], R.displacement(flow, uv, R.ITER_SCALE), f"iters {iters} batch {batch} level {level}: pair {p}")
    if level == 0:
        print(f"iters {iters} batch {batch}: median displacement of pair 1: {np.median(got[0].reshape(-1, 2), axis=0).tolist()} (true [1.2, -0.6])")


def test_stage_on_a_session_slots_that_wrap_and_refusals(eng):
    import torch
    from cuda_optical_flow_2_amd.parallel import ShardPlan

    B, level, iters = 2, 1, 1
    wl, hl = W >> level, H >> level
    want = _pairwise(iters)
    s = eng.Session(W, H, LEVELS, WIN, "lk_float", iters=iters, stream_batch=B)
    lib, hd = s.L, s._h
    ring = Guarded(np.float32, B, hl, 2 * wl, 2 * wl, 4, stride=hl * wl * 2 + 12)      # exactly B slots: they wrap; a padded stride
    base, stride = ring.ptr, ring.stride * 4
    out = _vp()
    assert lib.ofx_session_displacement_of(hd, 1, C.byref(out)) == 4                              # the stage is off
    sc = float(R.ITER_SCALE)
    assert lib.ofx_session_stream_displacement(hd, LEVELS, sc, base, stride, B) == 1              # level out of range
    assert lib.ofx_session_stream_displacement(hd, -1, sc, base, stride, B) == 1
    assert lib.ofx_session_stream_displacement(hd, level, sc, base + 8, stride, B) == 1           # ring not 16-byte aligned
    assert lib.ofx_session_stream_displacement(hd, level, sc, base, stride + 8, B) == 1           # stride not a multiple of 16
    assert lib.ofx_session_stream_displacement(hd, level, sc, base, hl * wl * 8 - 16, B) == 1     # stride shorter than a slot
    assert lib.ofx_session_stream_displacement(hd, level, sc, base, stride, B - 1) == 1           # fewer slots than stream_batch
    assert lib.ofx_session_stream_displacement(hd, level, float("nan"), base, stride, B) == 1
    assert lib.ofx_session_displacement_of(hd, 1, None) == 4                                       # nothing was set by any of those
    tens = ring.flat.view(torch.float32)[ring.lead:].as_strided((B, hl, wl, 2), (ring.stride, 2 * wl, 2, 1))
    assert tens.data_ptr() == base
    s.stream_displacement(tens, level)
    assert lib.ofx_session_displacement_of(hd, 1, None) == 1                                       # on, but no pair yet
    pitch = eng.pitch_for(W)
    frames = []
    for f in _clip():
        buf = torch.zeros((H, pitch), dtype=torch.uint8, device="cuda")
        buf[:, :W] = f
        frames.append(buf[:, :W])
    seen = 0

    def on_done(d):
        nonlocal seen
        torch.cuda.synchronize()
        got, clean = ring.host()
        assert clean, f"after pair {d}: bytes outside the slots were written"
        for p in range(max(seen + 1, d - B + 1), d + 1):
            flow, uv = want[p, level]
            ref = R.displacement(flow, uv, R.ITER_SCALE)
            same(got[(p - 1) % B].reshape(hl, wl, 2), ref, f"pair {p}: ring slot")
            assert lib.ofx_session_displacement_of(hd, p, C.byref(out)) == 0 and out.value == ring.slot((p - 1) % B)
            same(s.displacement_of(p).cpu().numpy(), ref, f"displacement_of({p})")
        for p in (0, d - B, d + 1):
            assert lib.ofx_session_displacement_of(hd, p, C.byref(out)) == 1
        seen = d

    s.stream_begin()
    assert lib.ofx_session_stream_displacement(hd, level, sc, base, stride, B) == 0               # right after stream_begin: still allowed
    for i, f in enumerate(frames):
        d = s.stream_submit(f)
        if i == 0:
            assert lib.ofx_session_stream_displacement(hd, level, sc, base, stride, B) == 4       # once the stream has frames
            assert lib.ofx_session_stream_displacement(hd, 0, sc, None, 0, 0) == 4
        if d >= 1:
            on_done(d)
    while True:
        d = s.stream_drain()
        if d == -2:
            break
        if d >= 1:
            on_done(d)
    assert seen == NF - 1
    s.stream_displacement(None)                                                                     # between streams: off again
    assert lib.ofx_session_displacement_of(hd, 1, None) == 4
    s.close()
    # sharded sessions and partial frames: unsupported
    w, h, win = 320, 240, 7
    plan = ShardPlan(w, h, LEVELS, win, 0, 2)
    big = torch.zeros(2 * h * w * 2, dtype=torch.float32, device="cuda")
    s = eng.Session(w, h, LEVELS, win, "lk_float", shard=plan, local_corner=True, stream_batch=2)
    assert s.L.ofx_session_stream_displacement(s._h, 0, sc, big.data_ptr(), h * w * 8, 2) == 3
    assert s.L.ofx_session_stream_displacement(s._h, 0, sc, None, 0, 0) == 0                      # turning it off is no request
    s.close()
    s = eng.Session(w, h, LEVELS, win, "lk_float", shard=plan, local_corner=True, stream_batch=2, borrow_frames=True, frames_partial=True)
    assert s.L.ofx_session_stream_displacement(s._h, 0, sc, big.data_ptr(), h * w * 8, 2) == 3
    s.close()


# ---- 5. the clip call -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _clip_displacements(iters):
    from cuda_optical_flow_2_amd import engine

    clip = _clip()
    return (engine.video_displacement(clip, LEVELS, WIN, iters=iters).cpu().numpy(),
            engine.video_displacement(clip.flip(0).contiguous(), LEVELS, WIN, iters=iters).cpu().numpy())


@pytest.mark.parametrize("iters", [1, 3])
def test_video_interpolate_equals_the_referee_on_video_displacement(eng, iters):
    import torch

    clip = _clip()
    fwd, bwd = _clip_displacements(iters)
    out, stats, ring_f, ring_b = eng.video_interpolate(clip, LEVELS, WIN, factor=4, iters=iters, return_stats=True, return_displacements=True)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (NF - 1, 3, H, W) and stats.dtype == torch.int64 and tuple(stats.shape) == (NF - 1, 3, 4)
    same(ring_f.cpu().numpy(), fwd, "the forward ring vs video_displacement of the clip")
    same(ring_b.cpu().numpy(), bwd, "the backward ring vs video_displacement of the reversed clip")
    host = clip.cpu().numpy()
    times = [np.float32(k / 4) for k in (1, 2, 3)]
    want = [R.interpolate_times(host[p], host[p + 1], fwd[p], bwd[NF - 2 - p], times) for p in range(NF - 1)]
    out, stats = out.cpu().numpy(), stats.cpu().numpy()
    for p in range(NF - 1):
        same(out[p], want[p][0], f"pair {p}: frames"); same(stats[p], want[p][1], f"pair {p}: stats")
    print(f"iters {iters}: stats of pair 0: {stats[0].tolist()}")
    # a clip whose row pitch exceeds W (a column slice of a wider tensor): the frames are read in place at that pitch
    wide = torch.full((NF, H, W + 24), 0xA5, dtype=torch.uint8, device="cuda")
    wide[:, :, 8:8 + W] = clip
    out2 = eng.video_interpolate(wide[:, :, 8:8 + W], LEVELS, WIN, factor=4, iters=iters)
    same(out2.cpu().numpy(), out, "a clip with a row pitch above W")
    # factor 2, and batch 1: the middle frames are the same
    out3 = eng.video_interpolate(clip, LEVELS, WIN, factor=2, iters=iters, batch=1)
    assert tuple(out3.shape) == (NF - 1, 1, H, W)
    same(out3.cpu().numpy()[:, 0], out[:, 1], "factor 2 vs the middle frame of factor 4")


def test_refusals(eng):
    clip = _clip()
    colour = clip[:3, :, :, None].expand(3, H, W, 3).contiguous()
    with pytest.raises(AssertionError, match="grey clips only"):
        eng.video_interpolate(colour, LEVELS, WIN)
    for factor in (1, 10, 2.5):
        with pytest.raises(AssertionError, match="factor"):
            eng.video_interpolate(clip, LEVELS, WIN, factor=factor)
    with pytest.raises(AssertionError, match="at least two"):
        eng.video_interpolate(clip[:1], LEVELS, WIN)


# ---- 6. quality, and identical frames -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("step", R.Q_STEPS, ids=str)
def test_interpolating_beats_a_cross_fade(eng, step, iters):
    """The CPU experiment of tests/test_interp_ref.py through engine.video_interpolate: every in-between frame is closer to the true
    frame than the cross-fade of its two neighbours -- "better than not using the flow at all"."""
    import torch

    frames = R.quality_clip(step)
    clip = torch.from_numpy(np.stack(frames[::4])).cuda()
    out = eng.video_interpolate(clip, R.Q_LEVELS, R.Q_WIN, factor=4, iters=iters).cpu().numpy()
    ratios = []
    for p in (0, 1):
        for k in (1, 2, 3):
            truth = frames[4 * p + k]
            s_int, s_fade = R.sad(out[p, k - 1], truth), R.sad(R.cross_fade(frames[4 * p], frames[4 * p + 4], np.float32(k / 4)), truth)
            ratios.append(s_int / s_fade)
    print(f"step {step} iters {iters}: SAD(interp) / SAD(cross-fade) = {min(ratios):.2f} .. {max(ratios):.2f}  ({[round(r, 3) for r in ratios]})")
    assert max(ratios) < 1.0, ratios


def test_identical_frames(eng):
    """min_det > 0: every flow is exactly (0, 0), so is every displacement; every in-between frame is the frame itself"""
    clip = _clip()[:1].expand(4, H, W).contiguous()
    out, stats, fwd, bwd = eng.video_interpolate(clip, LEVELS, WIN, factor=3, min_det=1.0, return_stats=True, return_displacements=True)
    assert int((fwd != 0).sum()) == 0 and int((bwd != 0).sum()) == 0
    assert stats.cpu().numpy().tolist() == [[[W * H, 0, 0, 0]] * 2] * 3
    out = out.cpu().numpy()
    for p in range(3):
        for k in range(2):
            same(out[p, k], clip[0].cpu().numpy(), f"pair {p} time {k}")
