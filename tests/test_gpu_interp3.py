"""GPU: colour frame interpolation -- the stateless launch (ofx_interpolate_frames_3ch), the batched one
(ofx_interpolate_frames_3ch_batch), engine.interpolate_frames_colour, engine.video_interpolate_colour and
engine.video_interpolate_colour_dense -- against tests/interp3_ref.py.  Every comparison is exact.  The method is
test_gpu_interp.py's: outputs sit in buffers of 0x5A that are checked clean afterwards, inputs in larger buffers whose surroundings
differ between runs (planes: 0x00, 0xFF, 0x5A; fields: a NaN, 1e30, 0), so that a tap outside an input, or a store outside an
output, shows."""
import ctypes as C
import functools

import numpy as np
import pytest

import interp3_ref as R3
import interp_ref as R
from test_gpu_interp import AROUND_F, AROUND_P, Field, Guarded, same

pytestmark = pytest.mark.gpu

_vp = C.c_void_p


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cuda_optical_flow_2_amd import engine

    return engine


class Plane3:
    """A [h, w, 3] uint8 plane with rows `pitch` bytes apart inside a larger buffer: `lead` bytes before it (the buffer itself is
    at least 256-byte aligned: lead % 4 is the plane's misalignment), 64 after its last row, and the pad bytes of every row, all
    holding the byte `around`."""

    def __init__(self, arr, pitch, lead, around, trail=64):
        import torch

        h, w, _ = arr.shape
        assert arr.shape == (h, w, 3) and pitch >= 3 * w
        host = np.full(lead + h * pitch + trail, around, np.uint8)
        np.lib.stride_tricks.as_strided(host[lead:], (h, 3 * w), (pitch, 1))[...] = arr.reshape(h, 3 * w)
        self.t = torch.from_numpy(host).cuda()
        assert self.t.data_ptr() % 4 == 0
        self.ptr, self.pitch = self.t.data_ptr() + lead, pitch


def _times(times):
    t = np.ascontiguousarray(times, np.float32)
    return t, t.ctypes.data_as(C.POINTER(C.c_float))


def _frames_of(g, w):
    """(the frames [slots, h, w, 3] of a Guarded buffer of rows 3 * w bytes wide, clean)"""
    got, clean = g.host()
    return got.reshape(got.shape[0], got.shape[1], w, 3), clean


# ---- 1. the stateless call ------------------------------------------------------------------------------------------------------

LAYOUTS = ["tight 0/1, dst tight odd address, odd time stride, stats", "tight 2/3, dst dwords, no stats",
           "padded, dst tight aligned address, stats", "padded, dst aligned but an odd time stride, stats"]


def _layout(li, run, a, b, w, h, T):
    """(plane a, plane b, frames, stats or None) of layout li with the surroundings of run 0, 1 or 2"""
    ar = (AROUND_P[run], AROUND_P[(run + 1) % 3])
    row = 3 * w
    rounded = (row + 3) // 4 * 4 + 8
    st = Guarded(np.int64, 1, T, 4, 4, 4, 4 * T)
    if li == 0:      # dst_pitch = 3 * w from an odd address: the byte path, whatever 3 * w is
        return Plane3(a, row, 0, ar[0]), Plane3(b, row, 1, ar[1]), Guarded(np.uint8, T, h, row, row, 61, h * row + 5), st
    if li == 1:      # destination, pitch and time stride 4-byte aligned: whole quads leave as three dwords
        return Plane3(a, row, 2, ar[0]), Plane3(b, row, 3, ar[1]), Guarded(np.uint8, T, h, row, rounded, 64), None
    if li == 2:      # tightly packed frames: dwords only where 3 * w is a multiple of 4
        return Plane3(a, row + 5, 3 + run, ar[0]), Plane3(b, row + 8, 64, ar[1]), Guarded(np.uint8, T, h, row, row, 16, h * row), st
    return Plane3(a, row + 8, 64 + run, ar[0]), Plane3(b, row + 5, 7, ar[1]), Guarded(np.uint8, T, h, row, rounded, 64, h * rounded + 21), st


def _launch(eng, pa, pb, fab, fba, w, h, times, frames, stats, slot=0, stats_slot=0):
    lib = eng._lib.load()
    t, tp = _times(times)
    eng.check(lib.ofx_interpolate_frames_3ch(pa.ptr, pa.pitch, pb.ptr, pb.pitch, w, h, fab.ptr, fba.ptr, tp, len(t), frames.slot(slot), frames.pitch,
                                             frames.stride, stats.slot(stats_slot) if stats else None, eng._stream_ptr()), "ofx_interpolate_frames_3ch")


@pytest.mark.parametrize("size", R.SIZES + [(132, 7)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_stateless_equals_the_referee(eng, size):
    import torch

    w, h = size
    a, b = R3.planes3(w, h)
    runs = []
    for ki, kind in enumerate(R.KINDS):
        dab, dba = R.field_case(kind, w, h)
        for ts, times in enumerate(R.TIME_SETS):
            want = R3.reference3(kind, w, h, ts)
            for li in range(len(LAYOUTS)):
                run = (li + ki + ts) % 3      # (the surroundings rotate: every layout meets all three patterns)
                pa, pb, frames, stats = _layout(li, run, a, b, w, h, len(times))
                fab, fba = Field(dab, 2 + 2 * (li & 1), AROUND_F[run]), Field(dba, 6, AROUND_F[(run + 1) % 3])
                _launch(eng, pa, pb, fab, fba, w, h, times, frames, stats)
                runs.append((f"{w}x{h} {kind} times {ts} ({LAYOUTS[li]})", (pa, pb, fab, fba), frames, stats, want))
    torch.cuda.synchronize()
    for what, _, frames, stats, want in runs:
        got, clean = _frames_of(frames, w)
        same(got, want[0], f"{what}: frames")
        assert clean, f"{what}: bytes around the frames were written"
        if stats is not None:
            got, clean = stats.host()
            same(got[0], want[1], f"{what}: stats")
            assert clean, f"{what}: bytes around the stats were written"
    assert len(runs) == len(R.KINDS) * len(R.TIME_SETS) * len(LAYOUTS)


# ---- 2. the batched call --------------------------------------------------------------------------------------------------------

BATCH_KINDS = ["inverse", "borders", "nonfinite", "edge"]


@pytest.mark.parametrize("n", [1, 3, 16])
def test_batch_equals_the_single_calls(eng, n):
    """every pair has its own planes, pitches and fields; the batched result is the single calls', bit for bit -- and the referee's"""
    import torch

    lib = eng._lib.load()
    w, h, times = 67, 33, R.TIME_SETS[1]
    T, row = len(times), 3 * 67
    t, tp = _times(times)
    inp = []
    for i in range(n):
        kind, seed = BATCH_KINDS[i % 4], i // 4
        a, b = R3.planes3(w, h, seed)
        dab, dba = R.field_case(kind, w, h, seed)
        run = i % 3
        inp.append((Plane3(a, row + (0, 5, 8, 1)[i % 4], i % 4, AROUND_P[run]), Plane3(b, row + (3, 0, 4, 9)[i % 4], 3 - i % 4, AROUND_P[(run + 1) % 3]),
                    Field(dab, 2, AROUND_F[run]), Field(dba, 6, AROUND_F[(run + 1) % 3]), (kind, seed)))
    single = Guarded(np.uint8, n * T, h, row, row, 61, h * row + 5)
    single_st = Guarded(np.int64, n, T, 4, 4, 4, 4 * T)
    for i in range(n):
        _launch(eng, *inp[i][:4], w, h, times, single, single_st, slot=i * T, stats_slot=i)
    ptrs = lambda f: (_vp * n)(*[f(i) for i in range(n)])
    ints = lambda f: (C.c_int * n)(*[f(i) for i in range(n)])
    outs = []
    for with_stats, (pitch, lead, extra) in ((True, (row, 61, 5)), (True, ((row + 3) // 4 * 4, 64, 20)), (False, (row + 7, 3, 2))):
        frames = Guarded(np.uint8, n * T, h, row, pitch, lead, h * pitch + extra)
        stats = Guarded(np.int64, n, T, 4, 4, 4, 4 * T) if with_stats else None
        eng.check(lib.ofx_interpolate_frames_3ch_batch(ptrs(lambda i: inp[i][0].ptr), ints(lambda i: inp[i][0].pitch), ptrs(lambda i: inp[i][1].ptr),
                                                       ints(lambda i: inp[i][1].pitch), n, w, h, ptrs(lambda i: inp[i][2].ptr),
                                                       ptrs(lambda i: inp[i][3].ptr), tp, T, ptrs(lambda i: frames.slot(i * T)), frames.pitch,
                                                       frames.stride, ptrs(lambda i: stats.slot(i)) if stats else None, eng._stream_ptr()),
                  "ofx_interpolate_frames_3ch_batch")
        outs.append((frames, stats))
    torch.cuda.synchronize()
    want_f, clean = _frames_of(single, w)
    assert clean, "single calls: bytes around the frames were written"
    want_s, clean = single_st.host()
    assert clean, "single calls: bytes around the stats were written"
    for i in range(n):
        kind, seed = inp[i][4]
        ref = R3.reference3(kind, w, h, 1, seed)
        same(want_f[i * T:(i + 1) * T], ref[0], f"pair {i} ({kind}, seed {seed}): the single call's frames")
        same(want_s[i], ref[1], f"pair {i} ({kind}, seed {seed}): the single call's stats")
    for oi, (frames, stats) in enumerate(outs):
        got, clean = _frames_of(frames, w)
        assert clean, f"batch of {n}, output {oi}: bytes around the frames were written"
        same(got, want_f, f"batch of {n}, output {oi}: frames")
        if stats is not None:
            got, clean = stats.host()
            assert clean, f"batch of {n}, output {oi}: bytes around the stats were written"
            same(got, want_s, f"batch of {n}, output {oi}: stats")


# ---- 3. equal channels, 4. the engine's helper ----------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["borders", "edge"])
def test_equal_channels_equal_the_grey_launch(eng, kind):
    """GPU against GPU: every output channel is ofx_interpolate_frames on that plane"""
    w, h = 257, 40
    a, b = R.planes(w, h)
    dab, dba = R.field_case(kind, w, h)
    grey_f, grey_s = eng.interpolate_frames(a, b, dab, dba, R.TIME_SETS[2])
    col_f, col_s = eng.interpolate_frames_colour(np.repeat(a[:, :, None], 3, 2), np.repeat(b[:, :, None], 3, 2), dab, dba, R.TIME_SETS[2])
    assert col_f.shape == (8, h, w, 3)
    for c in range(3):
        same(col_f[..., c], grey_f, f"{kind}: channel {c}")
    same(col_s, grey_s, f"{kind}: stats")


def test_engine_helper(eng):
    w, h = 257, 40
    a, b = R3.planes3(w, h)
    dab, dba = R.field_case("nonfinite", w, h)
    frames, stats = eng.interpolate_frames_colour(a, b, dab, dba, R.TIME_SETS[2])
    want = R3.reference3("nonfinite", w, h, 2)
    assert frames.dtype == np.uint8 and stats.dtype == np.int64
    same(frames, want[0], "frames"); same(stats, want[1], "stats")
    frames, stats = eng.interpolate_frames_colour(a, b, dab, dba, [0.5])
    same(frames, R3.reference3("nonfinite", w, h, 0)[0], "one time")


# ---- 5. the clip call -----------------------------------------------------------------------------------------------------------

W, H, LEVELS, WIN, NF = 128, 96, 3, 9, 6      # test_gpu_interp.py's clip


@functools.lru_cache(maxsize=None)
def _clip_host():
    from cuda_optical_flow_2_amd import synth

    return np.ascontiguousarray(np.stack([np.stack([synth.smooth_pair(W, H, 1.2 * i, -0.6 * i, seed=s)[1] for s in R3.Q_SEEDS], axis=2)
                                          for i in range(NF)]))


@functools.lru_cache(maxsize=None)
def _clip():
    import torch

    return torch.from_numpy(_clip_host()).cuda()


def _check_against_rings(what, host, out, stats, fwd, bwd, factor):
    times = [np.float32(k / factor) for k in range(1, factor)]
    n = len(host)
    for p in range(n - 1):
        want = R3.interpolate3_times(host[p], host[p + 1], fwd[p], bwd[n - 2 - p], times)
        same(out[p], want[0], f"{what}: pair {p}: frames")
        if stats is not None:
            same(stats[p], want[1], f"{what}: pair {p}: stats")


@pytest.mark.parametrize("iters", [1, 3])
def test_video_interpolate_colour_equals_the_referee_on_video_displacement(eng, iters):
    import torch

    clip, host = _clip(), _clip_host()
    fwd = eng.video_displacement(clip, LEVELS, WIN, iters=iters, frontend="grey").cpu().numpy()
    bwd = eng.video_displacement(clip.flip(0).contiguous(), LEVELS, WIN, iters=iters, frontend="grey").cpu().numpy()
    out, stats, ring_f, ring_b = eng.video_interpolate_colour(clip, LEVELS, WIN, factor=4, iters=iters, return_stats=True, return_displacements=True)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (NF - 1, 3, H, W, 3)
    assert stats.dtype == torch.int64 and tuple(stats.shape) == (NF - 1, 3, 4)
    same(ring_f.cpu().numpy(), fwd, "the forward ring vs video_displacement of the clip")
    same(ring_b.cpu().numpy(), bwd, "the backward ring vs video_displacement of the reversed clip")
    out, stats = out.cpu().numpy(), stats.cpu().numpy()
    _check_against_rings(f"iters {iters}", host, out, stats, fwd, bwd, 4)
    print(f"iters {iters}: stats of pair 0: {stats[0].tolist()}")
    # a column slice of a wider tensor, 3 * 3 = 9 bytes in: no frame is 4-byte aligned, and the frames are read in place
    wide = torch.full((NF, H, W + 8, 3), 0xA5, dtype=torch.uint8, device="cuda")
    wide[:, :, 3:3 + W] = clip
    view = wide[:, :, 3:3 + W]
    assert view.data_ptr() % 4 == 1 and view.stride(1) == 3 * (W + 8)
    out2 = eng.video_interpolate_colour(view, LEVELS, WIN, factor=4, iters=iters)
    same(out2.cpu().numpy(), out, "a clip that is a column slice of a wider tensor")
    assert int((wide[:, :, :3] != 0xA5).sum()) == 0 and int((wide[:, :, 3 + W:] != 0xA5).sum()) == 0
    # factor 2, and batch 1: the middle frames are the same
    out3 = eng.video_interpolate_colour(clip, LEVELS, WIN, factor=2, iters=iters, batch=1)
    assert tuple(out3.shape) == (NF - 1, 1, H, W, 3)
    same(out3.cpu().numpy()[:, 0], out[:, 1], "factor 2 vs the middle frame of factor 4")


def test_video_interpolate_colour_with_the_bilateral_front_end(eng):
    clip, host = _clip()[:4], _clip_host()[:4]
    out, stats, fwd, bwd = eng.video_interpolate_colour(clip, LEVELS, WIN, factor=3, frontend="bilateral", return_stats=True, return_displacements=True)
    assert tuple(out.shape) == (3, 2, H, W, 3)
    _check_against_rings("bilateral", host, out.cpu().numpy(), stats.cpu().numpy(), fwd.cpu().numpy(), bwd.cpu().numpy(), 3)


# ---- 6. the dense clip call -----------------------------------------------------------------------------------------------------

def test_video_interpolate_colour_dense(eng):
    import torch

    clip, host = _clip()[:4], _clip_host()[:4]
    grey = torch.from_numpy(np.stack([R3.grey(f) for f in host])).cuda()
    fwd = eng.video_displacement_dense(grey, LEVELS, WIN).cpu().numpy()
    bwd = eng.video_displacement_dense(grey.flip(0).contiguous(), LEVELS, WIN).cpu().numpy()
    out, stats, ring_f, ring_b = eng.video_interpolate_colour_dense(clip, LEVELS, WIN, factor=3, return_stats=True, return_displacements=True)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (3, 2, H, W, 3)
    same(ring_f.cpu().numpy(), fwd, "the forward ring vs video_displacement_dense of the grey clip")
    same(ring_b.cpu().numpy(), bwd, "the backward ring vs video_displacement_dense of the reversed grey clip")
    _check_against_rings("dense", host, out.cpu().numpy(), stats.cpu().numpy(), fwd, bwd, 3)
    # a clip no frame of which is 4-byte aligned: the grey clip is made from a padded copy, the colour frames are read in place
    wide = torch.full((4, H, W + 8, 3), 0xA5, dtype=torch.uint8, device="cuda")
    wide[:, :, 3:3 + W] = clip
    out2 = eng.video_interpolate_colour_dense(wide[:, :, 3:3 + W], LEVELS, WIN, factor=3)
    same(out2.cpu().numpy(), out.cpu().numpy(), "a clip that is a column slice of a wider tensor")


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------

def test_refusals(eng):
    clip = _clip()
    for fn in (eng.video_interpolate_colour, eng.video_interpolate_colour_dense):
        with pytest.raises(AssertionError, match="colour clips only"):
            fn(clip[..., 0].contiguous(), LEVELS, WIN)
        for factor in (1, 10, 2.5):
            with pytest.raises(AssertionError, match="factor"):
                fn(clip, LEVELS, WIN, factor=factor)
        with pytest.raises(AssertionError, match="at least two"):
            fn(clip[:1], LEVELS, WIN)
    with pytest.raises(AssertionError, match="main_cu"):
        eng.video_interpolate_colour(clip, LEVELS, WIN, frontend="main_cu")
    with pytest.raises(AssertionError, match="grey clips only"):      # the grey call still refuses colour, and names the new one
        eng.video_interpolate(clip, LEVELS, WIN)


# ---- 8. quality, 9. identical frames --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("step", R.Q_STEPS, ids=str)
def test_interpolating_every_channel_beats_a_cross_fade(eng, step, iters):
    """The CPU experiment of tests/test_interp3_ref.py through engine.video_interpolate_colour.  The GPU flows are the oracle's bit
    for bit, so the ratios are that test's: step (0.6, -0.3): 0.26 .. 0.46 (iters 1), 0.29 .. 0.49 (iters 3); step (1.0, 0.5):
    0.21 .. 0.80, 0.18 .. 0.51."""
    import torch

    frames = R3.colour_quality_clip(step)
    clip = torch.from_numpy(np.stack(frames[::4])).cuda()
    out = eng.video_interpolate_colour(clip, R.Q_LEVELS, R.Q_WIN, factor=4, iters=iters).cpu().numpy()
    ratios = []
    for p in (0, 1):
        for k in (1, 2, 3):
            for c in range(3):
                truth = frames[4 * p + k][..., c]
                fade = R.cross_fade(frames[4 * p][..., c], frames[4 * p + 4][..., c], np.float32(k / 4))
                ratios.append(R.sad(out[p, k - 1][..., c], truth) / R.sad(fade, truth))
    print(f"step {step} iters {iters}: SAD(interp) / SAD(cross-fade) per channel = {min(ratios):.2f} .. {max(ratios):.2f}  ({[round(r, 3) for r in ratios]})")
    assert len(ratios) == 18 and max(ratios) < 1.0, ratios


def test_identical_frames(eng):
    """min_det > 0: every flow is exactly (0, 0), so is every displacement; every in-between frame is the frame itself"""
    clip = _clip()[:1].expand(4, H, W, 3).contiguous()
    out, stats, fwd, bwd = eng.video_interpolate_colour(clip, LEVELS, WIN, factor=3, min_det=1.0, return_stats=True, return_displacements=True)
    assert int((fwd != 0).sum()) == 0 and int((bwd != 0).sum()) == 0
    assert stats.cpu().numpy().tolist() == [[[W * H, 0, 0, 0]] * 2] * 3
    out = out.cpu().numpy()
    for p in range(3):
        for k in range(2):
            same(out[p, k], _clip_host()[0], f"pair {p} time {k}")
