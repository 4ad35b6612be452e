"""GPU: the affine frame warp -- ofx_warp_affine and engine.warp_affine -- against tests/warp_affine_ref.py, by the bits.  The
sources sit at odd addresses in larger buffers whose surroundings (pad columns included) differ between runs, the destinations at
odd addresses in buffers of 0x5A, so that a tap outside a plane, or a store outside a row, shows."""
import ctypes as C

import numpy as np
import pytest

import warp_affine_ref as W
from test_gpu_interp import Guarded, Plane

pytestmark = pytest.mark.gpu

OFX_E_INVALID = 1
SHAPES = [(1, 1, 3, 2), (2, 3, 1, 1), (5, 4, 7, 3), (33, 17, 29, 21), (67, 45, 64, 48), (262, 74, 259, 80)]      # (w, h, sw, sh)
AROUND = [0x00, 0xFF]


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cuda_optical_flow_2_amd import engine

    return engine


def image(sw, sh, channels, seed=0):
    rng = np.random.RandomState(seed + sw + 1000 * sh + channels)
    return rng.randint(0, 256, (sh, sw) if channels == 1 else (sh, sw, 3)).astype(np.uint8)


def models_for(w, h, sw, sh):
    c, s = 1.1 * np.cos(0.3), 1.1 * np.sin(0.3)
    return [("identity", W.IDENTITY), ("whole pixels", (1.0, 0.0, 2.0, 0.0, 1.0, -1.0)), ("1/32 px", (1.0, 0.0, 3 / 32, 0.0, 1.0, 17 / 32)),
            ("-33/32 px", (1.0, 0.0, -33 / 32, 0.0, 1.0, -31 / 32)), ("rotation", (c, -s, 0.3 * sw, s, c, -0.2 * sh)),
            ("shear", (0.9, 0.35, -1.7, -0.2, 1.05, 0.6)), ("fit", ((sw - 1) / max(w - 1, 1), 0.0, 0.0, 0.0, (sh - 1) / max(h - 1, 1), 0.0)),
            ("gone right", (1.0, 0.0, 70000.0, 0.0, 1.0, 0.0)), ("gone up", (1.0, 0.0, 0.0, 0.0, 1.0, -70000.5)),
            ("limits", (16.0, -16.0, 1048576.0, -16.0, 16.0, -1048576.0)), ("limits back", (-16.0, 16.0, 0.5 * sw, 16.0, -16.0, 0.5 * sh)),
            ("steep", (16.0, 15.99, -3.0, -15.99, 16.0, 2.0 * sh))]


def run(eng, items, around, expect=0):
    """one ofx_warp_affine call on items (src, (w, h), model, border, fill, count, loose); returns [(dst, outside or None)], having
    checked that nothing around the destinations (pad bytes included) and the counts was written"""
    import torch

    lib = eng._lib
    descs, keep = (lib.WarpAffineDesc * len(items))(), []
    for i, (src, (w, h), m, border, fill, count, loose) in enumerate(items):
        ch = 3 if src.ndim == 3 else 1
        sh, sw = src.shape[:2]
        plane = Plane(src.reshape(sh, ch * sw), ch * sw + ((2 * i + 5) if loose else 0), 1 + 2 * (i % 3), around)
        dst = Guarded(np.uint8, 1, h, ch * w, ch * w + ((3 * i + 7) if loose else 0), 1 + 2 * (i % 2) + (i % 4 == 3))
        out = Guarded(np.int64, 1, 1, 1, 1, 1) if count else None
        keep.append((plane, dst, out))
        descs[i] = lib.WarpAffineDesc(plane.ptr, plane.pitch, sw, sh, dst.ptr, dst.pitch, w, h, ch, W.BORDERS[border], fill, (C.c_double * 6)(*m),
                                      out.ptr if count else None)
    rc = lib.load().ofx_warp_affine(descs, len(items), eng._stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, (rc, lib.load().ofx_last_error())
    res = []
    for i, (plane, dst, out) in enumerate(keep):
        got, clean = dst.host()
        assert clean, f"item {i}: a store outside the destination's rows"
        n = None
        if out is not None:
            cnt, clean = out.host()
            assert clean, f"item {i}: a store outside d_outside"
            n = int(cnt[0, 0, 0])
        src = items[i][0]
        res.append((got[0].reshape((items[i][1][1], items[i][1][0]) + src.shape[2:]), n))
    return res


def compare(eng, items, names, around):
    got = run(eng, items, around)
    for (src, size, m, border, fill, count, loose), name, (dst, n) in zip(items, names, got):
        want, want_n = W.warp_affine(src, m, size, border, fill)
        bad = np.argwhere(dst != want)
        assert len(bad) == 0, f"{name}: {len(bad)}/{dst.size} differ, first at {bad[:3].tolist()}: {dst[tuple(bad[0])]} vs {want[tuple(bad[0])]}"
        assert n == (want_n if count else None), f"{name}: outside {n} vs {want_n}"


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_shape_model_and_border_equals_the_referee(eng, shape, channels):
    w, h, sw, sh = shape
    src = image(sw, sh, channels)
    items, names = [], []
    for k, (name, m) in enumerate(models_for(w, h, sw, sh)):
        for border in ("replicate", "constant"):
            items.append((src, (w, h), m, border, 37 + k, (k + (border == "constant")) % 3 != 0, k % 2 == 1))
            names.append(f"{w}x{h} from {sw}x{sh} C={channels} {name} {border}")
    for around in AROUND:
        compare(eng, items[:1], names[:1], around)                         # one item
        for i0 in range(1, len(items), 16):                                 # and up to 16 in a launch
            compare(eng, items[i0:i0 + 16], names[i0:i0 + 16], around)


def test_sixteen_mixed_items_in_one_launch(eng):
    items, names = [], []
    for i in range(16):
        w, h, sw, sh = SHAPES[(i * 5 + 1) % len(SHAPES)]
        channels = (1, 3)[(i // 6) % 2]
        name, m = models_for(w, h, sw, sh)[(7 * i) % 12]
        items.append((image(sw, sh, channels, i), (w, h), m, "constant" if i % 2 else "replicate", 11 * i, i % 4 != 2, i % 3 == 0))
        names.append(f"item {i}: {w}x{h} from {sw}x{sh} C={channels} {name}")
    assert len({(it[1], it[0].ndim) for it in items}) >= 8
    for around in AROUND:
        compare(eng, items, names, around)


def test_whole_quads_at_aligned_and_unaligned_rows(eng):
    """rows whose addresses are 0 .. 3 mod 4 within one destination (an odd pitch), widths 4 k - 1 .. 4 k + 1: dword and byte stores"""
    for channels in (1, 3):
        for w in (7, 8, 9, 12):
            src = image(w + 2, 9, channels, w)
            items = [(src, (w, 8), (1.0, 0.0, 1.0 + k / 32, 0.0, 1.0, 0.5), "replicate", 0, True, bool(k)) for k in range(2)]
            compare(eng, items, [f"w={w} C={channels} item {k}" for k in range(2)], 0xFF)


def test_a_refused_call_writes_nothing(eng):
    src = image(20, 10, 3)
    ok = (src, (16, 8), W.IDENTITY, "replicate", 0, True, False)
    for bad in ((16.5, 0.0, 0.0, 0.0, 1.0, 0.0), (1.0, 0.0, float("nan"), 0.0, 1.0, 0.0), (1.0, 0.0, 0.0, 0.0, 1.0, 2.0 ** 21)):
        assert W.quantise(bad) is None
        for dst, n in run(eng, [ok, (src, (16, 8), bad, "constant", 5, True, True)], 0x00, expect=OFX_E_INVALID):
            assert (dst == 0x5A).all() and n == 0x5A5A5A5A5A5A5A5A


def test_engine_warp_affine(eng):
    import torch

    c, s = np.cos(0.1), np.sin(0.1)
    m = (c, -s, 3.25, s, c, -2.5)
    for channels in (1, 3):
        src = image(70, 50, channels, 4)
        want, want_n = W.warp_affine(src, m, None, "replicate")
        got = eng.warp_affine(src, m)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want)
        want, want_n = W.warp_affine(src, m, (33, 61), "constant", 9)
        got, n = eng.warp_affine(torch.from_numpy(src).cuda(), np.array(m), out_size=(33, 61), border="constant", fill=9, return_outside=True)
        assert got.is_cuda and n == want_n and np.array_equal(got.cpu().numpy(), want)
        assert np.array_equal(eng.warp_affine(src, W.IDENTITY), src)
        # a strided view of a larger tensor is copied, not misread
        big = torch.from_numpy(image(90, 60, channels, 5)).cuda()
        view = big[3:53, 7:77]
        assert np.array_equal(eng.warp_affine(view, m).cpu().numpy(), W.warp_affine(view.cpu().numpy(), m)[0])
    with pytest.raises(eng.OfxError):
        eng.warp_affine(src, (17.0, 0.0, 0.0, 0.0, 1.0, 0.0))
