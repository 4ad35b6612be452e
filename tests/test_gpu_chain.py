"""GPU: the displacement chain -- ofx_displacement_chain, engine.displacement_chain, engine.chain_ring, engine.denoise_rings and
video_denoise_dense(reach=2) -- against tests/chain_ref.py, by the bits, on the inputs of tests/chain_cases.py
(tests/test_chain_ref.py shows that they reach every branch).  Fields sit 8 but not 16 bytes aligned in larger buffers whose
surroundings differ between the runs; d_dst, d_mask and d_stats sit in buffers of 0x5A, so that a tap outside a field, or a store
outside an output, shows."""
import functools

import numpy as np
import pytest

import chain_cases as K
import chain_ref as R
import temporal_cases
import temporal_ref as T
from test_gpu_interp import Guarded, same

pytestmark = pytest.mark.gpu

AROUND = [0x7FC00000, 0x7149F2CA]                          # what surrounds the fields in the two runs: a NaN, 1e30
LEVELS, WIN = 4, 9                                         # of the dense flow on the 192 x 128 clip


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cuda_optical_flow_2_amd import engine

    return engine


class Field:
    """A float32 field [h, w, 2], tightly packed, `lead` floats into a larger buffer that holds the bit pattern `around` elsewhere"""

    def __init__(self, arr, lead, around):
        import torch

        self.lead, self.n, self.around, self.shape = lead, arr.size, around, arr.shape
        host = np.full(lead + arr.size + 16, around, np.uint32)
        host[lead:lead + arr.size] = np.ascontiguousarray(arr, np.float32).reshape(-1).view(np.uint32)
        self.t = torch.from_numpy(host.view(np.int32)).cuda()
        self.ptr = self.t.data_ptr() + 4 * lead

    def host(self):
        """(the field as it is now, True when its surroundings still hold `around`)"""
        raw = self.t.cpu().numpy().view(np.uint32)
        got = raw[self.lead:self.lead + self.n].copy().view(np.float32).reshape(self.shape)
        raw[self.lead:self.lead + self.n] = self.around
        return got, bool((raw == self.around).all())


@functools.lru_cache(maxsize=None)
def expected(kind, w, h, L, seed=0):
    """the referee's (dst, mask, stats) of K.links(kind, w, h, L, seed), computed once"""
    return R.chain(K.links(kind, w, h, L, seed))


def run(eng, items, around, expect=0, reuse=None, want_keep=False):
    """one ofx_displacement_chain call on items (links, mask, want_stats, in_place): mask None, "loose" (pitch and address 4-byte
    aligned) or "odd".  Returns [(dst, mask or None, stats or None)], having checked that nothing around the outputs (pad bytes
    included) nor around an in-place field was written.  want_keep: returns (that, keep), and reuse=keep makes a later call write
    the same output buffers again."""
    import torch

    lib = eng._lib
    descs, keep = (lib.ChainDesc * len(items))(), []
    for i, (links, mask, want_stats, in_place) in enumerate(items):
        h, w, _ = links[0].shape
        d = descs[i]
        flds = [Field(f, 2 if (i + k) % 3 else 6, around) for k, f in enumerate(links)]      # 8 or 24 bytes in: never 16-byte aligned
        if reuse is not None:
            dst, msk, stats = reuse[i][1:]
        else:
            dst = None if in_place else Guarded(np.float32, 1, h, 2 * w, 2 * w, 2 + 4 * (i % 2))
            msk = None if mask is None else Guarded(np.uint8, 1, h, w, (w + 11) & ~3, 4) if mask == "loose" else Guarded(np.uint8, 1, h, w, (w + 5) | 1, 1 + i % 4)
            stats = Guarded(np.int64, 1, 1, 4, 4, 1) if want_stats else None
        keep.append((flds, dst, msk, stats))
        for k, f in enumerate(flds):
            d.d_link[k] = f.ptr
        d.n_links, d.w, d.h = len(links), w, h
        d.d_dst = flds[0].ptr if in_place else dst.ptr
        d.d_mask, d.mask_pitch = (msk.ptr, msk.pitch) if msk is not None else (None, -1)
        d.d_stats = stats.ptr if stats is not None else None
    rc = lib.load().ofx_displacement_chain(descs, len(items), eng._stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, (rc, lib.load().ofx_last_error())
    res = []
    for i, (flds, dst, msk, stats) in enumerate(keep):
        h, w, _ = items[i][0][0].shape
        if dst is None:
            got, clean = flds[0].host()
            assert clean, f"item {i}: a store outside the field written in place"
        else:
            got, clean = dst.host()
            assert clean, f"item {i}: a store outside d_dst"
            got = got[0].reshape(h, w, 2)
        m = st = None
        if msk is not None:
            m, clean = msk.host()
            assert clean, f"item {i}: a store outside the mask's rows"
            m = m[0]
        if stats is not None:
            st, clean = stats.host()
            assert clean, f"item {i}: a store outside d_stats"
            st = st[0, 0]
        res.append((got, m, st))
    return (res, keep) if want_keep else res


def check_item(got, want, what):
    (dst, mask, stats), (wdst, wmask, wstats) = got, want
    same(dst, wdst, what + ": dst")
    if mask is not None:
        same(mask, wmask, what + ": mask")
    if stats is not None:
        assert stats.tolist() == wstats.tolist(), f"{what}: stats {stats.tolist()} vs {wstats.tolist()}"


@pytest.mark.parametrize("L", [2, 3, 4])
@pytest.mark.parametrize("size", K.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_kind_of_field_and_link_count(eng, size, L):
    """each case alone with every output, the mask at a loose pitch under one surrounding and at an odd one under the other"""
    w, h = size
    for kind in K.KINDS:
        links, want = K.links(kind, w, h, L), expected(kind, w, h, L)
        for around, pitch in zip(AROUND, ("loose", "odd")):
            (got,) = run(eng, [(links, pitch, True, False)], around)
            check_item(got, want, f"{kind} {w}x{h} L={L} {pitch}")


@pytest.mark.parametrize("size", [(5, 3), (257, 40)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_outputs_absent_one_at_a_time(eng, size):
    w, h = size
    for kind in ("borders", "nonfinite"):
        links, want = K.links(kind, w, h, 3), expected(kind, w, h, 3)
        for mask, want_stats in (("odd", False), (None, True), (None, False)):
            (got,) = run(eng, [(links, mask, want_stats, False)], AROUND[0])
            assert (got[1] is None) == (mask is None) and (got[2] is None) == (not want_stats)
            check_item(got, want, f"{kind} {w}x{h} mask={mask} stats={want_stats}")


def sixteen():
    items, wants, names = [], [], []
    for i in range(16):
        w, h = K.SIZES[(3 * i + 1) % len(K.SIZES)]
        kind, L = K.KINDS[(5 * i) % len(K.KINDS)], 2 + i % 3
        items.append((K.links(kind, w, h, L, seed=i), (None, "loose", "odd")[i % 3], i % 4 != 3, i % 5 == 2))
        wants.append(expected(kind, w, h, L, seed=i))
        names.append(f"item {i}, {kind} {w}x{h} L={L}")
    return items, wants, names


def test_a_batch_of_sixteen_equals_the_single_calls(eng):
    """sixteen items of every size, kind and link count, some in place, their outputs present or absent in turn"""
    items, wants, names = sixteen()
    assert {it[0][0].shape for it in items} == {(h, w, 2) for w, h in K.SIZES} and {len(it[0]) for it in items} == {2, 3, 4}
    for around in AROUND:
        batch = run(eng, items, around)
        for item, want, name, got in zip(items, wants, names, batch):
            (one,) = run(eng, [item], around)
            check_item(got, want, name)
            check_item(got, (one[0], one[1], one[2]), name + ": the batch vs the single call")
            assert (got[1] is None) == (item[1] is None) and (got[2] is None) == (not item[2])


@pytest.mark.parametrize("L", [2, 4])
def test_in_place_on_link_0_equals_out_of_place(eng, L):
    for w, h in ((5, 3), (130, 9), (257, 40)):
        for kind in ("inverse", "borders", "edge"):
            links, want = K.links(kind, w, h, L), expected(kind, w, h, L)
            (there,) = run(eng, [(links, "odd", True, True)], AROUND[0])
            (apart,) = run(eng, [(links, "odd", True, False)], AROUND[0])
            check_item(there, want, f"in place, {kind} {w}x{h} L={L}")
            check_item(there, apart, f"in place vs out of place, {kind} {w}x{h} L={L}")


def test_a_fold_of_two_link_calls_equals_the_chain(eng):
    """the consequence the definition states, on the device: the dead vectors of one call are the next call's input"""
    w, h = 257, 40
    for kind in ("borders", "nonfinite", "overflow"):
        links = K.links(kind, w, h, 4)
        acc = links[0]
        for j in range(1, 4):
            ((acc, _, _),) = run(eng, [([acc, links[j]], None, False, False)], AROUND[1])
        same(acc, expected(kind, w, h, 4)[0], f"{kind}: the fold")


def test_the_stats_slots_carry_nothing_between_calls(eng):
    first, second = ("borders", 67, 33, 3), ("nonfinite", 67, 33, 3)
    assert expected(*first)[2].tolist() != expected(*second)[2].tolist()
    _, keep = run(eng, [(K.links(*first), "loose", True, False)], AROUND[0], want_keep=True)
    (got,) = run(eng, [(K.links(*second), "loose", True, False)], AROUND[0], reuse=keep)
    check_item(got, expected(*second), "the second call into the same buffers")


def test_the_engine_calls_on_arrays_tensors_and_rings(eng):
    import torch

    links, (wdst, wmask, wstats) = K.links("borders", 67, 33, 3), expected("borders", 67, 33, 3)
    dst, mask, stats = eng.displacement_chain(links, return_mask=True, return_stats=True)
    assert isinstance(dst, np.ndarray) and dst.dtype == np.float32 and mask.dtype == np.uint8 and stats.dtype == np.int64
    same(dst, wdst, "arrays: dst"); same(mask, wmask, "arrays: mask"); same(stats, wstats, "arrays: stats")
    dev = eng.displacement_chain([torch.from_numpy(f.copy()).cuda() for f in links])
    assert isinstance(dev, torch.Tensor) and dev.is_cuda
    same(dev.cpu().numpy(), wdst, "tensors")
    dev, stats = eng.displacement_chain([torch.from_numpy(f.copy()).cuda() for f in links[:2]], return_stats=True)
    same(stats.cpu().numpy(), R.chain(links[:2])[2], "tensors: stats")
    ring = np.stack([K.links(kind, 130, 9, 4, seed=s)[s % 4] for s, kind in enumerate(("inverse", "borders", "inverse", "nonfinite", "inverse", "edge"))])
    dev_ring = torch.from_numpy(ring).cuda()
    for span in (2, 3, 4):
        out = eng.chain_ring(dev_ring, span)
        assert tuple(out.shape) == (len(ring) - span + 1, 9, 130, 2) and out.dtype == torch.float32
        same(out.cpu().numpy(), R.chain_ring(ring, span), f"chain_ring, span {span}")
    same(dev_ring.cpu().numpy(), ring, "the ring is read, not written")


# ---- from the rings to the frames: a reach of two ------------------------------------------------------------------------------------

CLIP_N, CLIP_W, CLIP_H, SIGMA = 7, 192, 128, 10


def ratio(out, noisy, clean):
    """the error over the noisy frames' error: frames 2 to 4, border 16"""
    sl = (slice(2, 5), slice(16, -16), slice(16, -16))
    err = lambda a: float(((np.asarray(a, np.float64)[sl] - clean[sl]) ** 2).mean())
    return err(out) / err(noisy)


def neighbours(f, n):
    return int(f >= 1) + int(f + 1 < n) + int(f >= 2) + int(f + 2 < n)


@pytest.mark.parametrize("channels", [1, 3])
def test_reach_two_equals_the_referee_on_the_returned_rings_and_reduces_the_noise_further(eng, channels):
    """video_denoise_dense(reach=2) and denoise_rings(reach=2): every output frame and its stats are the referee's on the returned
    rings, the chained rings are the referee's chains of them, reach=1 is the call without the keyword.  Quality: the printed
    ratios are errors over the noisy frames' error (frames 2 to 4, border 16); reach 2 must beat the same filter with zero fields
    and reach 1, the parent's path, measured here.  It measured reach 2 0.156, reach 1 0.261, zero fields 0.838 in grey, and 0.166,
    0.269, 1.273 in colour."""
    import torch

    noisy, clean = temporal_cases.pan_clip(CLIP_N, CLIP_W, CLIP_H, channels, SIGMA)
    clip = torch.from_numpy(noisy).cuda()
    N = CLIP_N
    out, stats, fwd, bwd, fwd2, bwd2 = eng.video_denoise_dense(clip, LEVELS, WIN, float(SIGMA), median=2, return_stats=True, return_displacements=True,
                                                               reach=2)
    assert out.dtype == torch.uint8 and tuple(out.shape) == tuple(clip.shape) and tuple(stats.shape) == (N, 8)
    assert tuple(fwd.shape) == tuple(bwd.shape) == (N - 1, CLIP_H, CLIP_W, 2) and tuple(fwd2.shape) == tuple(bwd2.shape) == (N - 2, CLIP_H, CLIP_W, 2)
    h_fwd, h_bwd = fwd.cpu().numpy(), bwd.cpu().numpy()
    same(fwd2.cpu().numpy(), R.chain_ring(h_fwd, 2), "fwd2")
    same(bwd2.cpu().numpy(), R.chain_ring(h_bwd, 2), "bwd2")
    table = T.weights_for(SIGMA)
    want = R.denoise_rings(noisy, h_fwd, h_bwd, table, 2)
    out, stats = out.cpu().numpy(), stats.cpu().numpy()
    for f in range(N):
        same(out[f], want[f][0], f"frame {f}")
        assert stats[f].tolist() == want[f][1].tolist(), (f, stats[f].tolist(), want[f][1].tolist())
        assert (stats[f, 1 + neighbours(f, N):5] == 0).all(), f"frame {f} has {neighbours(f, N)} neighbours"
    assert [neighbours(f, N) for f in range(N)] == [2, 3, 4, 4, 4, 3, 2]
    # the public call on the rings gives the same frames; three frames: two neighbours each
    again, again_stats = eng.denoise_rings(clip, fwd, bwd, float(SIGMA), reach=2, return_stats=True)
    same(again.cpu().numpy(), out, "denoise_rings(reach=2) on the returned rings")
    same(again_stats.cpu().numpy(), stats, "denoise_rings(reach=2): stats")
    short, short_stats = eng.denoise_rings(clip[:3], fwd[:2], bwd[N - 3:], table, reach=2, centre_weight=200, return_stats=True)
    want3 = R.denoise_rings(noisy[:3], h_fwd[:2], h_bwd[N - 3:], table, 2, 200)
    for f in range(3):
        same(short[f].cpu().numpy(), want3[f][0], f"three frames, frame {f}")
        assert short_stats[f].cpu().numpy().tolist() == want3[f][1].tolist() and (short_stats[f, 3:5] == 0).all()
    # reach=1 is the call without the keyword, byte for byte
    plain = eng.video_denoise_dense(clip, LEVELS, WIN, float(SIGMA), median=2, return_stats=True, return_displacements=True)
    one = eng.video_denoise_dense(clip, LEVELS, WIN, float(SIGMA), median=2, return_stats=True, return_displacements=True, reach=1)
    assert len(plain) == len(one) == 4
    for a, b, what in zip(plain, one, ("frames", "stats", "fwd", "bwd")):
        same(a.cpu().numpy(), b.cpu().numpy(), "reach=1 vs no keyword: " + what)
    same(plain[2].cpu().numpy(), h_fwd, "the rings do not depend on the reach")
    same(eng.denoise_rings(clip, fwd, bwd, float(SIGMA)).cpu().numpy(), plain[0].cpu().numpy(), "denoise_rings, reach 1")
    # the quality, measured and then asserted
    zero = torch.zeros((CLIP_H, CLIP_W, 2), dtype=torch.float32, device="cuda")
    still = np.stack([eng.temporal_filter(clip[f], [clip[g] for g in (f - 1, f + 1, f - 2, f + 2) if 0 <= g < N], [zero] * neighbours(f, N),
                                          float(SIGMA)).cpu().numpy() for f in range(N)])
    r2, r1, r0 = ratio(out, noisy, clean), ratio(plain[0].cpu().numpy(), noisy, clean), ratio(still, noisy, clean)
    print(f"C = {channels}, sigma {SIGMA}: error over the noisy frames' error: reach 2 {r2:.3f}, reach 1 {r1:.3f}, zero fields (four neighbours) {r0:.3f}")
    assert r2 < r0
    assert r2 < r1
