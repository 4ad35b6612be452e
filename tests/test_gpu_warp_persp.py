"""GPU: the perspective frame warp -- ofx_warp_perspective and engine.warp_perspective -- against tests/warp_persp_ref.py, by the
bits.  The sources sit at odd addresses in larger buffers whose surroundings (pad columns included) differ between runs, the
destinations at odd addresses in buffers of 0x5A, so that a tap outside a plane, or a store outside a row, shows."""
import ctypes as C

import numpy as np
import pytest

import warp_affine_ref as A
import warp_persp_ref as W
from test_gpu_interp import Guarded, Plane
from test_warp_persp_ref import lattice_models

pytestmark = pytest.mark.gpu

OFX_E_INVALID = 1
SHAPES = [(1, 1, 3, 2), (2, 3, 1, 1), (5, 4, 7, 3), (33, 17, 29, 21), (67, 45, 64, 48), (262, 74, 259, 80)]      # (w, h, sw, sh), test_gpu_warp_affine's
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
    affine = [(f"lattice affine {k}", tuple(m) + (0.0, 0.0, 1.0)) for k, m in enumerate(lattice_models(sw, sh))]
    s = float(max(w, h, 2))                              # (|m6|, |m7| <= 1 at the 1 x 1 shape too)
    return [("identity", W.IDENTITY), ("whole pixels", (1.0, 0.0, 2.0, 0.0, 1.0, -1.0, 0.0, 0.0, 1.0)), ("scaled identity", tuple(0.75 * v for v in W.IDENTITY))] + affine + [
        ("mild", (1.02, -0.015, 0.012 * sw, 0.02, 0.99, -0.008 * sh, 0.04 / s, -0.03 / s, 1.0)),
        ("fit", ((sw - 1) / max(w - 1, 1), 0.0, 0.0, 0.0, (sh - 1) / max(h - 1, 1), 0.0, 0.1 / s, 0.2 / s, 1.1)),
        ("horizon inside", (1.0, 0.1, 0.0, 0.0, 1.0, 0.0, -0.7 / s, -1.1 / s, 1.0)),
        ("W = 0 at pixels", (1.0, 0.0, 0.5, 0.0, 1.0, 0.25, -0.5, -0.25, 1.0)),                 # at (2, 0), (0, 4), (1, 2)
        ("W < 0 everywhere", (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, -0.001, -0.001, -0.5)),
        ("W = 0 everywhere", (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0)), ("zero", (0.0,) * 9),
        ("limits", W.LIMITS), ("limits back", (-16.0, 16.0, 0.5 * sw, 16.0, -16.0, 0.5 * sh, -1.0, 1.0, 16.0)),
        ("tiny W", (1.0, 0.0, 1.0, 0.0, 1.0, 1.0, 0.0, 0.0, 2.0 ** -40)), ("far", (16.0, 16.0, 1048576.0, 0.0, 1.0, 0.0, 0.0, 0.0, 2.0 ** -14))]


def run(eng, items, around, expect=0):
    """one ofx_warp_perspective call on items (src, (w, h), model, border, fill, count, loose); returns [(dst, outside or None)],
    having checked that nothing around the destinations (pad bytes included) and the counts was written"""
    import torch

    lib = eng._lib
    descs, keep = (lib.WarpPerspDesc * len(items))(), []
    for i, (src, (w, h), m, border, fill, count, loose) in enumerate(items):
        ch = 3 if src.ndim == 3 else 1
        sh, sw = src.shape[:2]
        plane = Plane(src.reshape(sh, ch * sw), ch * sw + ((2 * i + 5) if loose else 0), 1 + 2 * (i % 3), around)
        dst = Guarded(np.uint8, 1, h, ch * w, ch * w + ((3 * i + 7) if loose else 0), 1 + 2 * (i % 2) + (i % 4 == 3))
        out = Guarded(np.int64, 1, 1, 1, 1, 1) if count else None
        keep.append((plane, dst, out))
        descs[i] = lib.WarpPerspDesc(plane.ptr, plane.pitch, sw, sh, dst.ptr, dst.pitch, w, h, ch, W.BORDERS[border], fill, (C.c_double * 9)(*m),
                                     out.ptr if count else None)
    rc = lib.load().ofx_warp_perspective(descs, len(items), eng._stream_ptr())
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
        want, want_n = W.warp_perspective(src, m, size, border, fill)
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
        assert W.accepted(m), name
        for border in ("replicate", "constant"):
            items.append((src, (w, h), m, border, 37 + k, (k + (border == "constant")) % 3 != 0, k % 2 == 1))
            names.append(f"{w}x{h} from {sw}x{sh} C={channels} {name} {border}")
    for around in AROUND:
        compare(eng, items[:1], names[:1], around)                         # one item
        for i0 in range(1, len(items), 16):                                 # and up to 16 in a launch
            compare(eng, items[i0:i0 + 16], names[i0:i0 + 16], around)


def test_the_models_reach_every_rule():
    """CPU arithmetic on the referee: the list above holds a horizon inside the frame, pixels with W exactly 0, undefined frames"""
    w, h = 67, 45
    by = dict(models_for(w, h, 64, 48))
    qx, qy, defined = W.positions(by["horizon inside"], w, h)
    assert 0 < defined.sum() < w * h
    qx, qy, defined = W.positions(by["W = 0 at pixels"], w, h)
    assert defined[0, :2].all() and not defined[0, 2] and not defined[4, 0] and not defined[2, 1]
    for name in ("W < 0 everywhere", "W = 0 everywhere", "zero", "tiny W"):
        assert not W.positions(by[name], w, h)[2].any(), name
    assert W.positions(by["mild"], w, h)[2].all() and W.positions(by["far"], w, h)[2].any()


@pytest.mark.parametrize("channels", [1, 3])
def test_lattice_affine_models_give_the_affine_warps_bytes(eng, channels):
    """a bottom row of (0, 0, 1) and entries that are multiples of 1/32: no rounding in either warp"""
    w, h, sw, sh = 67, 45, 64, 48
    src = image(sw, sh, channels, 3)
    for m6 in lattice_models(sw, sh):
        for border in ("replicate", "constant"):
            got, n = run(eng, [(src, (w, h), tuple(m6) + (0.0, 0.0, 1.0), border, 9, True, True)], 0xFF)[0]
            want, want_n = A.warp_affine(src, m6, (w, h), border, 9)
            assert np.array_equal(got, want) and n == want_n, (m6, border)
            assert np.array_equal(eng.warp_affine(src, m6, (w, h), border, 9), got), "ofx_warp_affine's bytes on the device"


def test_sixteen_mixed_items_in_one_launch(eng):
    items, names = [], []
    for i in range(16):
        w, h, sw, sh = SHAPES[(i * 5 + 1) % len(SHAPES)]
        channels = (1, 3)[(i // 6) % 2]
        models = models_for(w, h, sw, sh)
        name, m = models[(7 * i) % len(models)]
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
            items = [(src, (w, 8), (1.0, 0.0, 1.0 + k / 32, 0.0, 1.0, 0.5, 0.001, -0.002, 1.0), "replicate", 0, True, bool(k)) for k in range(2)]
            compare(eng, items, [f"w={w} C={channels} item {k}" for k in range(2)], 0xFF)


def test_a_refused_call_writes_nothing(eng):
    src = image(20, 10, 3)
    ok = (src, (16, 8), W.IDENTITY, "replicate", 0, True, False)
    for k, v in ((0, 16.5), (2, float("nan")), (5, 2.0 ** 21), (6, 1.5), (7, float("inf")), (8, -16.5)):
        bad = list(W.IDENTITY)
        bad[k] = v
        assert not W.accepted(bad)
        for dst, n in run(eng, [ok, (src, (16, 8), bad, "constant", 5, True, True)], 0x00, expect=OFX_E_INVALID):
            assert (dst == 0x5A).all() and n == 0x5A5A5A5A5A5A5A5A


def test_engine_warp_perspective(eng):
    import torch

    m = (1.01, -0.02, 3.25, 0.015, 0.99, -2.5, 2e-4, -1e-4, 1.0)
    for channels in (1, 3):
        src = image(70, 50, channels, 4)
        want, want_n = W.warp_perspective(src, m, None, "replicate")
        got = eng.warp_perspective(src, m)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want)
        want, want_n = W.warp_perspective(src, m, (33, 61), "constant", 9)
        got, n = eng.warp_perspective(torch.from_numpy(src).cuda(), np.array(m).reshape(3, 3), out_size=(33, 61), border="constant", fill=9, return_outside=True)
        assert got.is_cuda and n == want_n and np.array_equal(got.cpu().numpy(), want)
        assert np.array_equal(eng.warp_perspective(src, W.IDENTITY), src)
        # a strided view of a larger tensor is copied, not misread
        big = torch.from_numpy(image(90, 60, channels, 5)).cuda()
        view = big[3:53, 7:77]
        assert np.array_equal(eng.warp_perspective(view, m).cpu().numpy(), W.warp_perspective(view.cpu().numpy(), m)[0])
    with pytest.raises(eng.OfxError):
        eng.warp_perspective(src, (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 1.5, 0.0, 1.0))
