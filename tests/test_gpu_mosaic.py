"""GPU: the frame mosaic -- ofx_warp_mosaic and engine.warp_mosaic -- against tests/mosaic_ref.py, by the bits, on the inputs of
tests/mosaic_cases.py (tests/test_mosaic_ref.py shows that they reach every rule).  The sources sit at odd addresses with loose
pitches in larger buffers whose surroundings (pad columns included) differ between runs; d_dst, d_which and d_counts sit in
buffers of 0x5A, so that a tap outside a plane, or a store outside a row, shows."""
import ctypes as C

import numpy as np
import pytest

import mosaic_cases as M
import mosaic_ref as Z
import warp_persp_ref as W
from test_gpu_interp import Guarded, Plane
from test_gpu_warp_persp import run as persp_run

pytestmark = pytest.mark.gpu

OFX_E_INVALID = 1
AROUND = [0x00, 0xFF]


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cuda_optical_flow_2_amd import engine

    return engine


def run(eng, items, around, expect=0, twice=()):
    """one ofx_warp_mosaic call on items (srcs, models, (w, h), border, fill, want_which, want_counts, loose); returns
    [(dst, which or None, counts or None)], having checked that nothing around the outputs (pad bytes included) was written.
    An item whose number is in `twice` gives its source 0 as ONE plane to all its sources."""
    import torch

    lib = eng._lib
    descs, keep = (lib.MosaicDesc * len(items))(), []
    for i, (srcs, models, (w, h), border, fill, want_which, want_counts, loose) in enumerate(items):
        ch = 3 if srcs[0].ndim == 3 else 1
        d = descs[i]
        planes = []
        for k, (src, m) in enumerate(zip(srcs, models)):
            sh, sw = src.shape[:2]
            if i in twice and k:
                plane = planes[0]
            else:
                plane = Plane(src.reshape(sh, ch * sw), ch * sw + ((2 * (i + k) + 5) if loose else 0), 1 + 2 * ((i + k) % 3), around)
            planes.append(plane)
            s = d.source[k]
            s.d_src, s.src_pitch, s.sw, s.sh, s.model = plane.ptr, plane.pitch, sw, sh, (C.c_double * 9)(*m)
        dst = Guarded(np.uint8, 1, h, ch * w, ch * w + ((3 * i + 7) if loose else 0), 1 + 2 * (i % 2) + (i % 4 == 3))
        which = Guarded(np.uint8, 1, h, w, w + ((i + 3) if loose else 0), 1 + i % 4) if want_which else None
        counts = Guarded(np.int64, 1, 1, 10, 10, 1) if want_counts else None
        keep.append((planes, dst, which, counts))
        d.n_sources, d.d_dst, d.dst_pitch, d.w, d.h, d.channels, d.border, d.fill = len(srcs), dst.ptr, dst.pitch, w, h, ch, W.BORDERS[border], fill
        d.d_which, d.which_pitch = (which.ptr, which.pitch) if want_which else (None, -1)
        d.d_counts = counts.ptr if want_counts else None
    rc = lib.load().ofx_warp_mosaic(descs, len(items), eng._stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, (rc, lib.load().ofx_last_error())
    res = []
    for i, (planes, dst, which, counts) in enumerate(keep):
        (w, h), src0 = items[i][2], items[i][0][0]
        got, clean = dst.host()
        assert clean, f"item {i}: a store outside the destination's rows"
        wh = cn = None
        if which is not None:
            wh, clean = which.host()
            assert clean, f"item {i}: a store outside d_which's rows"
            wh = wh[0]
        if counts is not None:
            cn, clean = counts.host()
            assert clean, f"item {i}: a store outside d_counts"
            cn = cn[0, 0]
        res.append((got[0].reshape((h, w) + src0.shape[2:]), wh, cn))
    return res


def compare(eng, items, names, around, twice=()):
    got = run(eng, items, around, twice=twice)
    for i, ((srcs, models, size, border, fill, want_which, want_counts, loose), name, (dst, which, counts)) in enumerate(zip(items, names, got)):
        srcs = [srcs[0]] * len(srcs) if i in twice else srcs
        want, want_which_, want_counts_ = Z.mosaic(srcs, models, size, border, fill)
        bad = np.argwhere(dst != want)
        assert len(bad) == 0, f"{name}: {len(bad)}/{dst.size} differ, first at {bad[:3].tolist()}: {dst[tuple(bad[0])]} vs {want[tuple(bad[0])]}"
        assert (which is None) == (not want_which) and (counts is None) == (not want_counts)
        if want_which:
            bad = np.argwhere(which != want_which_)
            assert len(bad) == 0, f"{name}: which: {len(bad)} differ, first at {bad[:3].tolist()}: {which[tuple(bad[0])]} vs {want_which_[tuple(bad[0])]}"
        if want_counts:
            assert counts.tolist() == want_counts_.tolist(), f"{name}: counts {counts.tolist()} vs {want_counts_.tolist()}"


def in_launches(eng, cases, first_alone=True):
    """cases: (name, item); once alone, then up to 16 per launch, under both surroundings"""
    names, items = [c[0] for c in cases], [c[1] for c in cases]
    for around in AROUND:
        if first_alone:
            compare(eng, items[:1], names[:1], around)
        for i0 in range(1 if first_alone else 0, len(items), 16):
            compare(eng, items[i0:i0 + 16], names[i0:i0 + 16], around)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("shape", M.SHAPES)
def test_the_ladder_at_every_shape_border_and_source_count(eng, shape, channels):
    w, h, sw, sh = shape
    cases = []
    for S in M.LADDER_S:
        name, srcs, models, size = M.ladder(w, h, S, channels)
        for border in ("replicate", "constant"):
            k = len(cases)
            cases.append((f"{w}x{h} C={channels} {name} {border}", (srcs, models, size, border, 37 + k, True, True, k % 2 == 1)))
    in_launches(eng, cases)


@pytest.mark.parametrize("channels", [1, 3])
def test_the_shake(eng, channels):
    cases = []
    for w, h, sw, sh in M.SHAPES[2:]:
        name, srcs, models, size = M.shake(w, h, channels)
        for border in ("replicate", "constant"):
            cases.append((f"{w}x{h} C={channels} {name} {border}", (srcs, models, size, border, 200, True, True, True)))
    in_launches(eng, cases)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("shape", M.SHAPES)
def test_the_hard_models_against_a_second_source(eng, shape, channels):
    w, h, sw, sh = shape
    cases = []
    for name, srcs, models, size in M.hard_pairs(w, h, sw, sh, channels):
        for border in ("replicate", "constant"):
            k = len(cases)
            cases.append((f"{w}x{h} C={channels} {name} {border}", (srcs, models, size, border, 41 + k, True, True, k % 3 != 0)))
    in_launches(eng, cases, first_alone=False)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("shape", M.SHAPES)
def test_one_source_is_the_perspective_warp_on_the_device(eng, shape, channels):
    w, h, sw, sh = shape
    src = M.image(sw, sh, channels)
    mosaic_items, persp_items, names = [], [], []
    for k, (name, m) in enumerate(M.models_for(w, h, sw, sh)):
        for border in ("replicate", "constant"):
            mosaic_items.append(([src], [m], (w, h), border, 37 + k, True, True, k % 2 == 1))
            persp_items.append((src, (w, h), m, border, 37 + k, True, k % 2 == 0))
            names.append(f"{w}x{h} from {sw}x{sh} C={channels} {name} {border}")
    for i0 in range(0, len(names), 16):
        got = run(eng, mosaic_items[i0:i0 + 16], 0xFF)
        want = persp_run(eng, persp_items[i0:i0 + 16], 0x00)
        for name, (dst, which, counts), (pdst, outside) in zip(names[i0:], got, want):
            assert np.array_equal(dst, pdst), f"{name}: {int((dst != pdst).sum())} bytes differ from ofx_warp_perspective's"
            assert counts[9] == outside and counts[0] == w * h - outside and not counts[1:9].any(), name
            assert set(which.reshape(-1).tolist()) <= {0, 255} and int((which == 255).sum()) == outside, name


def test_one_plane_given_as_two_sources(eng):
    for channels in (1, 3):
        src = M.image(40, 30, channels, 2)
        models = [(1.0, 0.0, 3.25, 0.0, 1.0, -2.5, 0.0, 0.0, 1.0), (0.98, 0.01, -4.5, -0.01, 1.01, 6.0, 1e-4, 0.0, 1.0), (1.0, 0.0, 3.25, 0.0, 1.0, -2.5, 0.0, 0.0, 1.0)]
        items = [([src] * 3, models, (44, 33), border, 9, True, True, True) for border in ("replicate", "constant")]
        compare(eng, items, [f"C={channels} twice, {b}" for b in ("replicate", "constant")], 0x00, twice=(0, 1))
        (dst, which, counts), _ = run(eng, items, 0xFF, twice=(0, 1))
        assert counts[0] > 0 and counts[1] > 0 and counts[2] == 0 and counts[9] > 0


def test_which_and_counts_null_in_every_combination(eng):
    name, srcs, models, size = M.ladder(67, 45, 5, 3)
    items = [(srcs, models, size, ("replicate", "constant")[k % 2], 77, bool(k & 1), bool(k & 2), True) for k in range(4)]
    names = [f"which={bool(k & 1)} counts={bool(k & 2)}" for k in range(4)]
    for around in AROUND:
        compare(eng, items, names, around)
        for i in range(4):
            compare(eng, items[i:i + 1], names[i:i + 1], around)


def test_sixteen_mixed_items_in_one_launch(eng):
    items, names = [], []
    for i in range(16):
        w, h, sw, sh = M.SHAPES[(i * 5 + 1) % len(M.SHAPES)]
        channels = (1, 3)[(i // 6) % 2]
        if i % 3 == 0:
            name, srcs, models, size = M.ladder(w, h, M.LADDER_S[(i // 3) % 4], channels)
        elif i % 3 == 1:
            name, srcs, models, size = M.shake(w, h, channels)
        else:
            name, srcs, models, size = M.hard_pairs(w, h, sw, sh, channels)[i % 12]
        items.append((srcs, models, size, "constant" if i % 2 else "replicate", 11 * i, i % 4 != 2, i % 5 != 3, i % 3 == 0))
        names.append(f"item {i}: {w}x{h} C={channels} {name}")
    assert len({(it[2], it[0][0].ndim, len(it[0])) for it in items}) >= 8
    for around in AROUND:
        compare(eng, items, names, around)


def test_whole_quads_at_aligned_and_unaligned_rows(eng):
    """rows whose addresses are 0 .. 3 mod 4 within one destination and one d_which (odd pitches), widths 4 k - 1 .. 4 k + 1: the
    dword and the byte stores of both planes"""
    for channels in (1, 3):
        for w in (7, 8, 9, 12):
            srcs = [M.image(w + 2, 9, channels, w), M.image(w + 5, 12, channels, w + 1)]
            items = []
            for k in range(2):
                models = [(1.0, 0.0, 3.0 + k / 32, 0.0, 1.0, 0.5, 0.001, -0.002, 1.0), (1.0, 0.0, 1.25, 0.0, 1.0, 2.5, 0.0, 0.0, 1.0)]
                items.append((srcs, models, (w, 8), "replicate", 0, True, True, True))
            assert (channels * w + 7) % 2 == 1 or (channels * w + 10) % 2 == 1, "an odd dst_pitch in one of the items"
            assert (w + 3) % 2 == 1 or (w + 4) % 2 == 1, "an odd which_pitch in one of the items"
            compare(eng, items, [f"w={w} C={channels} item {k}" for k in range(2)], 0xFF)


def test_a_refused_call_writes_nothing(eng):
    name, srcs, models, size = M.ladder(33, 17, 2, 3)
    ok = (srcs, models, size, "replicate", 0, True, True, False)
    for k, v in ((0, 16.5), (2, float("nan")), (5, 2.0 ** 21), (6, 1.5), (7, float("inf")), (8, -16.5)):
        bad = list(W.IDENTITY)
        bad[k] = v
        assert not W.accepted(bad)
        for dst, which, counts in run(eng, [ok, (srcs, [models[0], bad], size, "constant", 5, True, True, True)], 0x00, expect=OFX_E_INVALID):
            assert (dst == 0x5A).all() and (which == 0x5A).all() and (counts == 0x5A5A5A5A5A5A5A5A).all()
    msg = eng._lib.load().ofx_last_error()
    assert b"ofx_warp_mosaic" in msg and b"item 1" in msg and b"source 1" in msg and b"model[8]" in msg, msg


def test_engine_warp_mosaic(eng):
    import torch

    for channels in (1, 3):
        name, srcs, models, size = M.ladder(67, 45, 5, channels)
        want, want_which, want_counts = Z.mosaic(srcs, models, size, "replicate", 0)
        got = eng.warp_mosaic(srcs, models, out_size=size)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want)
        got, which, counts = eng.warp_mosaic(srcs, np.array(models), out_size=size, return_which=True, return_counts=True)
        assert np.array_equal(got, want) and np.array_equal(which, want_which) and counts.dtype == np.int64 and counts.tolist() == want_counts.tolist()
        # out_size None: source 0's size; tensors in, tensors out
        want, want_which, want_counts = Z.mosaic(srcs, models, (srcs[0].shape[1], srcs[0].shape[0]), "constant", 9)
        got, counts = eng.warp_mosaic([torch.from_numpy(s).cuda() for s in srcs], models, border="constant", fill=9, return_counts=True)
        assert got.is_cuda and counts.is_cuda and np.array_equal(got.cpu().numpy(), want) and counts.cpu().tolist() == want_counts.tolist()
        got, which = eng.warp_mosaic([torch.from_numpy(s).cuda() for s in srcs], models, border="constant", fill=9, return_which=True)
        assert which.is_cuda and which.dtype == torch.uint8 and np.array_equal(which.cpu().numpy(), want_which)
        # strided views of a larger tensor are copied, not misread
        big = torch.from_numpy(M.image(90, 60, channels, 5)).cuda()
        views = [big[3:53, 7:77], big[1:40, 20:81]]
        m2 = [(1.0, 0.0, 3.25, 0.0, 1.0, -2.5, 0.0, 0.0, 1.0), (1.01, -0.02, -5.5, 0.015, 0.99, 4.0, 2e-4, -1e-4, 1.0)]
        want, want_which, _ = Z.mosaic([v.cpu().numpy() for v in views], m2, (70, 50), "replicate", 0)
        got, which = eng.warp_mosaic(views, m2, return_which=True)
        assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(which.cpu().numpy(), want_which)
        assert np.array_equal(eng.warp_mosaic([srcs[0]], [W.IDENTITY]), srcs[0])
    with pytest.raises(eng.OfxError):
        eng.warp_mosaic(srcs[:2], [W.IDENTITY, (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 1.5, 0.0, 1.0)])
