"""GPU: the temporal noise filter -- ofx_temporal_filter, engine.temporal_filter, video_denoise and video_denoise_dense -- against
tests/temporal_ref.py, by the bits, on the inputs of tests/temporal_cases.py (tests/test_temporal_ref.py shows that they reach every
branch).  Planes sit at odd addresses, tight or loose, and fields 8 but not 16 bytes aligned, in larger buffers whose surroundings
(pad columns included) differ between the runs; d_dst and d_stats sit in buffers of 0x5A, so that a tap outside a plane or a field,
or a store outside a row, shows."""
import ctypes as C
import functools

import numpy as np
import pytest

import temporal_cases as K
import temporal_ref as T
from test_gpu_interp import Guarded, Plane

pytestmark = pytest.mark.gpu

AROUND = [(0x00, 0x7FC00000), (0xFF, 0x7149F2CA)]        # what surrounds the planes, and the fields (a NaN, 1e30), in the two runs
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

        host = np.full(lead + arr.size + 16, around, np.uint32)
        host[lead:lead + arr.size] = np.ascontiguousarray(arr, np.float32).reshape(-1).view(np.uint32)
        self.t = torch.from_numpy(host.view(np.int32)).cuda()
        self.ptr = self.t.data_ptr() + 4 * lead


@functools.lru_cache(maxsize=None)
def ladder(w, h, channels):
    """the cases of one size with the referee's answers, computed once"""
    out = []
    for name, c, planes, fields, table, wc in K.ladder(w, h, channels):
        with np.errstate(all="ignore"):
            out.append((name, c, planes, fields, table, wc) + T.temporal_filter(c, planes, fields, table, wc))
    return out


def run(eng, items, table, wc, around, expect=0, reuse=None, want_keep=False):
    """one ofx_temporal_filter call on items (centre, planes, fields, want_stats, loose); a plane that IS the centre or an earlier
    plane (the same array) is given as the same device plane.  Returns [(dst, stats or None)], having checked that nothing around
    the outputs (pad bytes included) was written.  want_keep: returns (that, keep), and reuse=keep makes a later call write the
    same destination and stats buffers again."""
    import torch

    lib = eng._lib
    descs, keep = (lib.TemporalDesc * len(items))(), []
    for i, (centre, planes, fields, want_stats, loose) in enumerate(items):
        h, w = centre.shape[:2]
        ch = 3 if centre.ndim == 3 else 1
        d = descs[i]
        made = {}

        def plane_of(a, k):
            if id(a) not in made:
                # tight pitches put the rows at every address mod 4; lead is odd or even in turn
                made[id(a)] = Plane(a.reshape(h, ch * w), ch * w + ((2 * (i + k) + 5) if loose else 0), 1 + (i + k) % 4, around[0])
            return made[id(a)]

        cen = plane_of(centre, 0)
        nbs = [plane_of(p, 1 + k) for k, p in enumerate(planes)]
        flds = [Field(f, 2 + 4 * ((i + k) % 2) if (i + k) % 3 else 4, around[1]) for k, f in enumerate(fields)]     # 8, 24 or 16 bytes in
        if reuse is None:
            dst = Guarded(np.uint8, 1, h, ch * w, ch * w + ((3 * i + 7) if loose else 0), 1 + 2 * (i % 2) + (i % 4 == 3))
            stats = Guarded(np.int64, 1, 1, 8, 8, 1) if want_stats else None
        else:
            dst, stats = reuse[i][1], reuse[i][2]
        keep.append(((cen, nbs, flds), dst, stats))
        for k, (p, f) in enumerate(zip(nbs, flds)):
            s = d.neighbour[k]
            s.d_plane, s.pitch, s.pad, s.d_field = p.ptr, p.pitch, -1, f.ptr
        d.n_neighbours, d.w, d.h, d.channels = len(planes), w, h, ch
        d.d_centre, d.centre_pitch, d.d_dst, d.dst_pitch = cen.ptr, cen.pitch, dst.ptr, dst.pitch
        d.d_stats = stats.ptr if want_stats else None
    prm = lib.TemporalParams()
    prm.weights = (C.c_uint16 * 256)(*[int(v) for v in table])
    prm.centre_weight, prm.reserved = int(wc), 0
    rc = lib.load().ofx_temporal_filter(descs, len(items), C.byref(prm), eng._stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, (rc, lib.load().ofx_last_error())
    res = []
    for i, (_, dst, stats) in enumerate(keep):
        centre = items[i][0]
        got, clean = dst.host()
        assert clean, f"item {i}: a store outside the destination's rows"
        st = None
        if stats is not None:
            st, clean = stats.host()
            assert clean, f"item {i}: a store outside d_stats"
            st = st[0, 0]
        res.append((got[0].reshape(centre.shape), st))
    return (res, keep) if want_keep else res


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)}/{got.size} differ, first at {bad[:3].tolist()}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


def check(eng, case, around, i=0, want_stats=True):
    name, c, planes, fields, table, wc, want, want_stats_ = case
    (got, stats), = run(eng, [(c, planes, fields, want_stats, i % 2 == 1)], table, wc, around)
    same(got, want, name)
    if want_stats:
        assert stats.tolist() == want_stats_.tolist(), f"{name}: stats {stats.tolist()} vs {want_stats_.tolist()}"
    return got


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("size", K.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_kind_of_field_table_and_neighbour_count(eng, size, channels):
    """each case alone, pitches tight and loose in turn, under both surroundings; stats = NULL is accepted and changes no byte"""
    for i, case in enumerate(ladder(size[0], size[1], channels)):
        a = check(eng, case, AROUND[0], i)
        b = check(eng, case, AROUND[1], i + 1, want_stats=i % 3 == 0)
        same(a, b, case[0] + ": the two runs")


@pytest.mark.parametrize("wc", [1, 37, 256])
def test_the_division_is_exact_for_every_pair_of_values(eng, wc):
    name, a, planes, fields, table, _ = K.division_case(wc)
    want, want_stats = T.temporal_filter(a, planes, fields, table, wc)
    (got, stats), = run(eng, [(a, planes, fields, True, False)], table, wc, AROUND[0])
    same(got, want, name)
    assert stats.tolist() == want_stats.tolist()


def test_the_stats_slots_carry_nothing_between_calls(eng):
    cases = ladder(67, 9, 1)
    first, second = cases[2], cases[4]
    assert first[6].shape == second[6].shape and first[7].tolist() != second[7].tolist()
    _, keep = run(eng, [(first[1], first[2], first[3], True, True)], first[4], first[5], AROUND[0], want_keep=True)
    (got, stats), = run(eng, [(second[1], second[2], second[3], True, True)], second[4], second[5], AROUND[0], reuse=keep)
    same(got, second[6], second[0])
    assert stats.tolist() == second[7].tolist()


def test_a_batch_of_sixteen_equals_the_single_calls(eng):
    """one table per launch: 16 items of every size and both channel counts, their own fields and neighbour counts"""
    table, wc = K.tables()["sigma 10"], 200
    items, names = [], []
    for i in range(16):
        w, h = K.SIZES[i % len(K.SIZES)]
        ch = 3 if (i // len(K.SIZES) + i) % 2 else 1
        name, c, planes, fields, _, _ = K.case(w, h, ch, 1 + i % 4, K.KINDS[(i * 5) % len(K.KINDS)], "sigma 10", wc, seed=60 + i, same=i % 5 == 0, own=i % 7 == 3)
        items.append((c, planes, fields, i % 4 != 3, i % 2 == 0))
        names.append(name)
    for around in AROUND:
        batch = run(eng, items, table, wc, around)
        for i, (item, name, (got, stats)) in enumerate(zip(items, names, batch)):
            (one, one_stats), = run(eng, [item], table, wc, around)
            with np.errstate(all="ignore"):
                want, want_stats = T.temporal_filter(item[0], item[1], item[2], table, wc)
            same(got, one, f"item {i}, {name}: the batch vs the single call")
            same(got, want, f"item {i}, {name}")
            assert (stats is None) == (not item[3])
            if stats is not None:
                assert stats.tolist() == one_stats.tolist() == want_stats.tolist(), (name, stats.tolist(), want_stats.tolist())


def test_the_engine_call_on_arrays_and_tensors(eng):
    import torch

    name, c, planes, fields, table, wc, want, want_stats = ladder(67, 9, 3)[12]
    got, stats = eng.temporal_filter(c, planes, fields, table, wc, return_stats=True)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and stats.dtype == np.int64
    same(got, want, name); same(stats, want_stats, name + ": stats")
    dev = eng.temporal_filter(torch.from_numpy(c).cuda(), [torch.from_numpy(p).cuda() for p in planes], [torch.from_numpy(f).cuda() for f in fields],
                              table, wc)
    assert isinstance(dev, torch.Tensor) and dev.is_cuda
    same(dev.cpu().numpy(), want, name + ": tensors")
    # a sigma for a table
    grey = ladder(67, 9, 1)[12]
    with np.errstate(all="ignore"):
        same(eng.temporal_filter(grey[1], grey[2], grey[3], 10.0), T.temporal_filter(grey[1], grey[2], grey[3], T.weights_for(10.0))[0], "sigma")


# ---- from the rings to the frames ---------------------------------------------------------------------------------------------------

CLIP_N, CLIP_W, CLIP_H, SIGMA = 5, 192, 128, 10


def mse(a, b, border=8):
    d = np.asarray(a, np.float64)[:, border:-border, border:-border] - np.asarray(b, np.float64)[:, border:-border, border:-border]
    return float((d * d).mean())


@pytest.mark.parametrize("channels", [1, 3])
def test_video_denoise_dense_equals_the_referee_on_its_rings_and_reduces_the_noise(eng, channels):
    """Every output frame is the referee applied to the returned rings: two neighbours inside, one at the ends.  Quality: the error
    against the clean frames must be below the noisy frames' and below that of the same launch with zero fields (the referee puts
    the two ends, true fields and zero fields, at 0.34 and 0.91 of the noisy error)."""
    import torch

    noisy, clean = K.pan_clip(CLIP_N, CLIP_W, CLIP_H, channels, SIGMA)
    clip = torch.from_numpy(noisy).cuda()
    out, stats, fwd, bwd = eng.video_denoise_dense(clip, LEVELS, WIN, float(SIGMA), median=2, return_stats=True, return_displacements=True)
    assert out.dtype == torch.uint8 and tuple(out.shape) == tuple(clip.shape) and tuple(stats.shape) == (CLIP_N, 8)
    assert tuple(fwd.shape) == tuple(bwd.shape) == (CLIP_N - 1, CLIP_H, CLIP_W, 2)
    out, stats, fwd, bwd = out.cpu().numpy(), stats.cpu().numpy(), fwd.cpu().numpy(), bwd.cpu().numpy()
    want = T.denoise_rings(noisy, fwd, bwd, T.weights_for(SIGMA))
    for f in range(CLIP_N):
        same(out[f], want[f][0], f"frame {f}")
        assert stats[f].tolist() == want[f][1].tolist(), (f, stats[f].tolist(), want[f][1].tolist())
    assert stats[0, 2] == 0 and stats[CLIP_N - 1, 2] == 0, "the end frames have one neighbour"
    plain = eng.video_denoise_dense(clip, LEVELS, WIN, float(SIGMA), median=2)
    assert isinstance(plain, torch.Tensor)
    same(plain.cpu().numpy(), out, "without stats and rings")
    # the quality, measured and then asserted
    zero = torch.zeros((CLIP_H, CLIP_W, 2), dtype=torch.float32, device="cuda")
    still = np.stack([eng.temporal_filter(clip[f], [clip[g] for g in (f - 1, f + 1) if 0 <= g < CLIP_N], [zero] * (1 + (0 < f < CLIP_N - 1)),
                                          float(SIGMA)).cpu().numpy() for f in range(CLIP_N)])
    base = mse(noisy, clean)
    r_flow, r_zero = mse(out, clean) / base, mse(still, clean) / base
    print(f"C = {channels}, sigma {SIGMA}: error over the noisy frames' error: video_denoise_dense(median=2) {r_flow:.3f}, zero fields {r_zero:.3f}")
    assert r_flow < 1.0
    assert r_flow < r_zero


def test_video_denoise_equals_the_referee_on_the_stream_pipelines_rings(eng):
    import torch

    noisy, _ = K.pan_clip(CLIP_N, CLIP_W, CLIP_H, 1, SIGMA, step=(1, 1))
    clip = torch.from_numpy(noisy).cuda()
    out, stats, fwd, bwd = eng.video_denoise(clip, 3, WIN, float(SIGMA), return_stats=True, return_displacements=True)
    assert out.dtype == torch.uint8 and tuple(out.shape) == tuple(clip.shape)
    out, stats, fwd, bwd = out.cpu().numpy(), stats.cpu().numpy(), fwd.cpu().numpy(), bwd.cpu().numpy()
    same(fwd, eng.video_displacement(clip, 3, WIN).cpu().numpy(), "the forward ring is video_displacement's")
    want = T.denoise_rings(noisy, fwd, bwd, T.weights_for(SIGMA))
    for f in range(CLIP_N):
        same(out[f], want[f][0], f"frame {f}")
        assert stats[f].tolist() == want[f][1].tolist(), (f, stats[f].tolist(), want[f][1].tolist())
    # a table in place of sigma, another centre weight, and a clip whose row pitch exceeds W
    wide = torch.full((CLIP_N, CLIP_H, CLIP_W + 24), 0xA5, dtype=torch.uint8, device="cuda")
    wide[:, :, 8:8 + CLIP_W] = clip
    table = K.tables()["random"]
    out2 = eng.video_denoise(wide[:, :, 8:8 + CLIP_W], 3, WIN, table, centre_weight=37).cpu().numpy()
    with pytest.raises(AssertionError, match="video_denoise: grey clips only"):
        eng.video_denoise(clip[..., None].expand(-1, -1, -1, 3).contiguous(), 3, WIN, float(SIGMA))
    want2 = T.denoise_rings(noisy, fwd, bwd, table, 37)
    for f in range(CLIP_N):
        same(out2[f], want2[f][0], f"random table, frame {f}")
