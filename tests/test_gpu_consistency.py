"""GPU: the forward-backward check -- the stateless launch (ofx_flow_consistency) and the batched one
(ofx_flow_consistency_batch) against tests/consistency_ref.py, and engine.video_consistency against the referee applied to
engine.video_flow of the clip and of the reversed clip.  Every comparison is exact, floats by their bits."""
import ctypes as C
import functools

import numpy as np
import pytest

import consistency_ref as R
from cuda_optical_flow_2_amd import synth

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


# ---- 1. the stateless launch ----------------------------------------------------------------------------------------------------

class Field:
    """A [h, w, 2] float32 field inside a larger buffer: `lead` floats before it (even: 8-byte aligned) and 64 after it, all
    holding the bit pattern `around`."""

    def __init__(self, arr, lead, around):
        import torch

        assert lead % 2 == 0
        host = np.full(lead + arr.size + 64, around, np.uint32)
        host[lead:lead + arr.size] = np.ascontiguousarray(arr, np.float32).reshape(-1).view(np.uint32)
        self.t = torch.from_numpy(host.view(np.int32)).cuda()
        self.ptr = self.t.data_ptr() + 4 * lead


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


def _outputs(shape, n, w, h):
    """(mask, err, stats) buffers of one of the three output shapes"""
    if shape == "bytes+stats":         # mask at pitch w + 9 from an odd address: byte stores
        return Guarded(np.uint8, n, h, w, w + 9, 61, h * (w + 9) + 5), None, Guarded(np.int64, n, 1, 4, 4, 4, 4)
    if shape == "dwords+err":          # mask at a 4-byte aligned pitch and address: dword stores; err 4-byte aligned only
        return Guarded(np.uint8, n, h, w, (w + 3) // 4 * 4 + 8, 64), Guarded(np.float32, n, h, w, w, 3), None
    return None, None, Guarded(np.int64, n, 1, 4, 4, 4, 4)     # (the stats slots follow each other: one memset for a run of them)


SHAPES = ["bytes+stats", "dwords+err", "stats"]
AROUND = [0x7FC00000, 0x7149F2CA, 0x00000000]      # a NaN, 1e30, 0: what surrounds the fields in the three runs


def _check(what, bufs, want, i=0, slot=0):
    mask, err, stats = bufs
    for buf, ref, name in ((mask, want[0], "mask"), (err, want[1], "err"), (stats, want[2], "stats")):
        if buf is None:
            continue
        got, clean = buf.host()
        same(got[slot] if name != "stats" else got[slot][0], ref, f"{what}: {name}")
        assert clean, f"{what}: bytes around the {name} were written"


@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_stateless_equals_the_referee(eng, size):
    import torch

    lib = eng._lib.load()
    w, h = size
    n = 0
    for kind in R.KINDS:
        fwd, bwd, scale = R.field_case(kind, w, h)
        for ti, (alpha, beta) in enumerate(R.tolerances(scale)):
            want = R.reference(kind, w, h, ti)
            runs = []
            for shape, around in zip(SHAPES, AROUND):
                # the fields sit in larger buffers whose other words differ between the runs: a tap outside a field would show
                f, b = Field(fwd, 2, around), Field(bwd, 6, around)
                bufs = _outputs(shape, 1, w, h)
                mask, err, stats = bufs
                eng.check(lib.ofx_flow_consistency(f.ptr, b.ptr, w, h, float(scale), float(alpha), float(beta), mask.ptr if mask else None,
                                                   mask.pitch if mask else 0, err.ptr if err else None, stats.ptr if stats else None,
                                                   eng._stream_ptr()), "ofx_flow_consistency")
                runs.append((shape, bufs, f, b))
            torch.cuda.synchronize()
            for shape, bufs, _, _ in runs:
                _check(f"{w}x{h} {kind} alpha {float(alpha)} beta {float(beta)} ({shape})", bufs, want)
            n += 1
    assert n == 2 * len(R.KINDS)


@pytest.mark.parametrize("lead", [4, 1], ids=["err-16-byte-aligned", "err-4-byte-aligned"])
def test_err_of_a_width_that_is_a_multiple_of_four(eng, lead):
    """Where err is 16-byte aligned and w a multiple of 4 the launch stores e four floats at a time: none of the shared sizes
    but 4 x 1 gets there."""
    import torch

    lib = eng._lib.load()
    w, h = 132, 7
    for kind in ("inverse", "nonfinite", "edge"):
        fwd, bwd, scale = R.field_case(kind, w, h)
        alpha, beta = R.tolerances(scale)[0]
        f, b = Field(fwd, 2, AROUND[0]), Field(bwd, 2, AROUND[0])
        mask, err = Guarded(np.uint8, 1, h, w, w, 64), Guarded(np.float32, 1, h, w, w, lead)
        eng.check(lib.ofx_flow_consistency(f.ptr, b.ptr, w, h, float(scale), float(alpha), float(beta), mask.ptr, w, err.ptr, None,
                                           eng._stream_ptr()), "ofx_flow_consistency")
        torch.cuda.synchronize()
        _check(f"{w}x{h} {kind}", (mask, err, None), R.reference(kind, w, h, 0))


def test_engine_helper(eng):
    w, h = 257, 40
    fwd, bwd, scale = R.field_case("nonfinite", w, h)
    want = R.reference("nonfinite", w, h, 0)
    mask, stats, err = eng.flow_consistency(fwd, bwd, want_err=True)
    same(mask, want[0], "mask"); same(stats, want[2], "stats"); same(err, want[1], "err")
    mask, stats = eng.flow_consistency(fwd, bwd, alpha=0.0, beta_px2=0.0)
    same(mask, R.reference("nonfinite", w, h, 1)[0], "mask at (0, 0)")
    fwd, bwd, scale = R.field_case("edge", w, h)
    mask, stats = eng.flow_consistency(fwd, bwd, scale=1.0)
    same(mask, R.reference("edge", w, h, 0)[0], "edge: mask"); same(stats, R.reference("edge", w, h, 0)[2], "edge: stats")


# ---- 2. the batched launch ------------------------------------------------------------------------------------------------------

BATCH_KINDS = ["inverse", "borders", "nonfinite"]      # (one launch has one scale: the kinds in OFX_ITER_SCALE units)


def _batch(eng, w, h, pairs, shape, slots):
    """pairs: (kind, seed); slots: which slot of the n-slot output buffers pair i writes.  Returns the buffers."""
    import torch

    lib = eng._lib.load()
    n = len(pairs)
    fields = [R.field_case(kind, w, h, seed) for kind, seed in pairs]
    scale = fields[0][2]
    alpha, beta = R.tolerances(scale)[0]
    dev = [(Field(f, 2, AROUND[i % 3]), Field(b, 2, AROUND[(i + 1) % 3])) for i, (f, b, _) in enumerate(fields)]
    bufs = _outputs(shape, max(slots) + 1, w, h)
    mask, err, stats = bufs
    arr = lambda buf: None if buf is None else (_vp * n)(*[buf.slot(s) for s in slots])
    eng.check(lib.ofx_flow_consistency_batch((_vp * n)(*[d[0].ptr for d in dev]), (_vp * n)(*[d[1].ptr for d in dev]), n, w, h, float(scale),
                                             float(alpha), float(beta), arr(mask), mask.pitch if mask else 0, arr(err), arr(stats),
                                             eng._stream_ptr()), "ofx_flow_consistency_batch")
    torch.cuda.synchronize()
    return bufs


def _single(eng, w, h, kind, seed):
    """(mask, err, stats) of one pair by the stateless call"""
    fwd, bwd, scale = R.field_case(kind, w, h, seed)
    return eng.flow_consistency(fwd, bwd, float(scale), want_err=True)


@pytest.mark.parametrize("slots", [(0, 1, 2), (4, 0, 2)], ids=["consecutive", "scattered"])
def test_batch_of_three_kinds_equals_the_single_calls(eng, slots):
    w, h = 257, 40
    pairs = [(kind, 0) for kind in BATCH_KINDS]
    for shape in SHAPES:
        mask, err, stats = _batch(eng, w, h, pairs, shape, slots)
        got = {name: buf.host() for name, buf in (("mask", mask), ("err", err), ("stats", stats)) if buf is not None}
        for name, (_, clean) in got.items():
            assert clean, f"{shape}: bytes around the {name} slots were written"
        for i, (kind, seed) in enumerate(pairs):
            m1, s1, e1 = _single(eng, w, h, kind, seed)
            want = R.reference(kind, w, h, 0, seed)
            same(m1, want[0], f"{kind}: the single call's mask"); same(e1, want[1], f"{kind}: its err"); same(s1, want[2], f"{kind}: its stats")
            for name, ref in (("mask", m1), ("err", e1), ("stats", s1)):
                if name in got:
                    g = got[name][0][slots[i]]
                    same(g[0] if name == "stats" else g, ref, f"{shape}: pair {i} ({kind}): {name}")
        if stats is not None:       # a slot no pair writes is left alone (it is not even zeroed)
            free = sorted(set(range(max(slots) + 1)) - set(slots))
            assert (got["stats"][0][free] == FILL64).all()


def test_batch_of_sixteen(eng):
    w, h = 67, 33
    pairs = [(BATCH_KINDS[i % 3], i // 3) for i in range(16)]
    for shape in SHAPES[:2]:
        mask, err, stats = _batch(eng, w, h, pairs, shape, tuple(range(16)))
        for buf, k, name in ((mask, 0, "mask"), (err, 1, "err"), (stats, 2, "stats")):
            if buf is None:
                continue
            got, clean = buf.host()
            assert clean, f"{shape}: bytes around the {name} slots were written"
            for i, (kind, seed) in enumerate(pairs):
                same(got[i][0] if name == "stats" else got[i], R.reference(kind, w, h, 0, seed)[k], f"{shape}: pair {i} ({kind}, seed {seed}): {name}")


# ---- 3. the clip call -----------------------------------------------------------------------------------------------------------

W, H, LEVELS, WIN, NF = 128, 96, 3, 9, 6


@functools.lru_cache(maxsize=None)
def _clip():
    import torch

    return torch.from_numpy(np.stack([synth.smooth_pair(W, H, 1.2 * i, -0.6 * i, seed=41)[1] for i in range(NF)])).cuda()


@functools.lru_cache(maxsize=None)
def _flows(iters, level):
    """(video_flow of the clip, video_flow of the reversed clip) as host arrays"""
    from cuda_optical_flow_2_amd import engine

    clip = _clip()
    fwd = engine.video_flow(clip, LEVELS, WIN, level=level, iters=iters).cpu().numpy()
    bwd = engine.video_flow(clip.flip(0).contiguous(), LEVELS, WIN, level=level, iters=iters).cpu().numpy()
    return fwd, bwd


@functools.lru_cache(maxsize=None)
def _clip_reference(iters, level):
    """per pair p: the referee's (mask, stats) forward, and backward (the fields swapped)"""
    fwd, bwd = _flows(iters, level)
    alpha, beta = R.tolerances(R.ITER_SCALE)[0]
    out = []
    for p in range(NF - 1):
        f, b = fwd[p], bwd[NF - 2 - p]
        mf, _, sf = R.consistency(f, b, R.ITER_SCALE, alpha, beta)
        mb, _, sb = R.consistency(b, f, R.ITER_SCALE, alpha, beta)
        out.append((mf, sf, mb, sb))
    return out


@pytest.mark.parametrize("batch", [1, 2, None])
@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("iters", [1, 3])
def test_video_consistency_equals_the_referee_on_video_flow(eng, iters, level, batch):
    import torch

    want = _clip_reference(iters, level)
    fwd, bwd = _flows(iters, level)
    mask, stats, mask_b, stats_b, ring_f, ring_b = eng.video_consistency(_clip(), LEVELS, WIN, level=level, iters=iters, batch=batch, both=True,
                                                                         return_flows=True)
    hl, wl = H >> level, W >> level
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == (NF - 1, hl, wl) and stats.dtype == torch.int64 and tuple(stats.shape) == (NF - 1, 4)
    same(ring_f.cpu().numpy(), fwd, "the forward ring vs video_flow of the clip")
    same(ring_b.cpu().numpy(), bwd, "the backward ring vs video_flow of the reversed clip")
    mask, stats, mask_b, stats_b = (t.cpu().numpy() for t in (mask, stats, mask_b, stats_b))
    for p in range(NF - 1):
        same(mask[p], want[p][0], f"pair {p}: mask"); same(stats[p], want[p][1], f"pair {p}: stats")
        same(mask_b[p], want[p][2], f"pair {p}: backward mask"); same(stats_b[p], want[p][3], f"pair {p}: backward stats")
    # without the extras: the same two
    m2, s2 = eng.video_consistency(_clip(), LEVELS, WIN, level=level, iters=iters, batch=batch)
    same(m2.cpu().numpy(), mask, "both=False: mask"); same(s2.cpu().numpy(), stats, "both=False: stats")
    print(f"iters {iters} level {level} batch {batch}: stats {stats.tolist()}")


def test_identical_frames(eng):
    """min_det > 0: all flows are exactly (0, 0) and every pixel is consistent.  min_det = 0: class 3 counts the forward vectors
    that fail step 2, and the classes add up.  (That equality needs no finite forward vector beside a NaN of bwd's: a NaN tap
    makes e NaN, which is class 3 by step 7.  On this textured clip no window is flat -- measured: 0 vectors fail step 2 in every
    pair, stats [12288, 0, 0, 0] -- so both sides are 0 here.)"""
    import torch

    clip = _clip()[:1].expand(4, H, W).contiguous()
    # min_det > 0: every flow is exactly (0, 0), every pixel consistent
    mask, stats = eng.video_consistency(clip, LEVELS, WIN, min_det=1.0)
    assert stats.cpu().numpy().tolist() == [[W * H, 0, 0, 0]] * 3 and int(mask.max()) == 0
    # min_det = 0
    mask, stats, fwd, bwd = eng.video_consistency(clip, LEVELS, WIN, return_flows=True)
    mask, stats, fwd = mask.cpu().numpy(), stats.cpu().numpy(), fwd.cpu().numpy()
    for p in range(3):
        u, v = fwd[p, ..., 0], fwd[p, ..., 1]
        with np.errstate(invalid="ignore", over="ignore"):
            px = (np.arange(W, dtype=np.float32)[None, :] + (R.ITER_SCALE * u).astype(np.float32)).astype(np.float32)
            py = (np.arange(H, dtype=np.float32)[:, None] + (R.ITER_SCALE * v).astype(np.float32)).astype(np.float32)
            fails = ~((np.abs(px) <= np.float32(1e9)) & (np.abs(py) <= np.float32(1e9)))
        print(f"pair {p}: stats {stats[p].tolist()}, forward vectors failing step 2: {int(fails.sum())}")
        assert stats[p, 3] == np.count_nonzero(fails)
        assert stats[p, 1] + stats[p, 2] + stats[p, 3] + np.count_nonzero(mask[p] == 0) == W * H and stats[p, 0] == W * H


def test_refusals(eng):
    import torch

    colour = _clip()[:3, :, :, None].expand(3, H, W, 3).contiguous()
    with pytest.raises(AssertionError, match="main_cu"):
        eng.video_consistency(colour, LEVELS, WIN, frontend="main_cu")
    with pytest.raises(AssertionError, match="at least two"):
        eng.video_consistency(_clip()[:1], LEVELS, WIN)
    # the default front end of a colour clip is "bilateral", and the reversed run sees the same images
    mask, stats, fwd, bwd = eng.video_consistency(colour, LEVELS, WIN, return_flows=True)
    want = eng.video_flow(colour.flip(0).contiguous(), LEVELS, WIN, frontend="bilateral")
    assert torch.equal(bwd.view(torch.int32), want.view(torch.int32))
    assert stats[:, 0].tolist() == [W * H, W * H]
