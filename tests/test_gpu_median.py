"""GPU: the flow median -- the launch (ofx_flow_median), flow only and fused with the warp, against tests/median_ref.py, the oracle's
warp and the chain of a flow-only launch and ofx_warp_levels; several items in one launch; the session driver
(ofx_session_run_flow_dense_median) against median_ref.dense_pair_median at every level; its refusals; and the quality of
engine.video_displacement_dense(median=2) on the device.  Every comparison is by the bits (dense_ref.same_bits).  Outputs sit in
buffers of 0x5A, inputs in larger buffers whose surroundings differ between runs, so that a tap outside an input, or a store outside
an output, shows."""
import ctypes as C
import functools

import numpy as np
import pytest

import dense_ref as D
import interp_ref as IR
import iter_hard as ih
import median_ref as M
from test_gpu_interp import AROUND_F, AROUND_P, FILL, Field, Guarded, Plane

pytestmark = pytest.mark.gpu

F32 = np.float32
OFX_E_INVALID, OFX_E_UNSUPPORTED, OFX_E_STATE = 1, 3, 4


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cuda_optical_flow_2_amd import engine

    return engine


def same(got, want, what):
    """floats by their bits (two NaNs are the same value: dense_ref.same_bits), bytes as they are"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype}{got.shape} vs {want.dtype}{want.shape}"
    ok = D.same_bits(got, want) if got.dtype == np.float32 else got == want
    if not ok.all():
        bad = np.argwhere(~ok)
        raise AssertionError(f"{what}: {len(bad)}/{got.size} differ, first at {bad[:3].tolist()}: {got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}")


def _desc(eng, field, w, h, r, out, src=None, dst=None, dst_pitch=0, scale=D.P_SCALE):
    return eng._lib.MedianDesc(field.ptr, out, w, h, r, float(scale), None if src is None else src.ptr, 0 if src is None else src.pitch, dst, dst_pitch)


def _launch(eng, descs):
    lib = eng._lib.load()
    arr = (eng._lib.MedianDesc * len(descs))(*descs)
    eng.check(lib.ofx_flow_median(arr, len(descs), eng._stream_ptr()), "ofx_flow_median")


# ---- 1. the launch, flow only -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", M.M_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_median_equals_the_referee(eng, shape):
    """(a block of the kernel covers a tile of 256 columns x 16 rows, a wave one row of it per step: 63x7 and 65x9 sit inside one
    tile, 262x74 and 263x75 cross its seams both ways -- two tiles across, the second 6 and 7 columns wide, five down, the last 10
    and 11 rows high -- with quads of every w mod 4 at the row ends)"""
    import torch

    w, h = shape
    runs = []
    for ki, kind in enumerate(M.M_KINDS):
        for r in (1, 2):
            # (source lead, destination lead) in floats: both 16-byte aligned; a merely 8-byte aligned destination; ... source
            for fl, dl in ((4, 4), (4, 2), (2, 4)):
                f = Field(M.field_case(kind, w, h), fl, AROUND_F[(ki + r + fl) % 3])
                d = Guarded(np.float32, 1, h, 2 * w, 2 * w, dl)
                _launch(eng, [_desc(eng, f, w, h, r, d.ptr)])
                runs.append((f"{kind} radius {r} leads {fl}/{dl}", f, d, M.want(kind, w, h, r)))
    torch.cuda.synchronize()
    for what, _, d, want in runs:
        got, clean = d.host()
        same(got[0].reshape(h, w, 2), want, what)
        assert clean, f"{what}: bytes around the field were written"
    assert len(runs) == 24


def test_engine_helper(eng, oracle):
    w, h = 65, 9
    f = M.field_case("salted", w, h)
    for r in (1, 2):
        same(eng.flow_median(f, r), M.want("salted", w, h, r), f"engine.flow_median radius {r}")
    src = _source(w, h)
    got_f, got_w = eng.flow_median(f, src=src)
    same(got_f, M.want("salted", w, h, 2), "engine.flow_median with src: the field")
    same(got_w, oracle.warp_bilinear_u8(src, M.want("salted", w, h, 2), eng.ITER_SCALE), "engine.flow_median with src: the warped image")


# ---- 2. fused with the warp -------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _source(w, h):
    return IR.planes(w, h, seed=3)[0].copy()       # (writable: the engine's helpers hand it to torch)


@pytest.mark.parametrize("case", [((262, 74), 2, 272), ((263, 75), 2, 263), ((263, 75), 1, 264), ((263, 75), 2, 320), ((65, 9), 1, 66),
                                  ((5, 4), 2, 5), ((1, 1), 2, 3), ((2, 3), 1, 2)],
                         ids=lambda c: f"{c[0][0]}x{c[0][1]}-r{c[1]}-pitch{c[2]}")
def test_fused_warp_equals_the_referee_the_oracle_and_the_chain(eng, oracle, case):
    import torch

    (w, h), r, dst_pitch = case
    want_f = M.want("patched", w, h, r)
    src = _source(w, h)
    want_w = oracle.warp_bilinear_u8(src, want_f, D.P_SCALE)
    if w > 100:
        # the FILTERED field is what the case says: pixels that are not warped (inside the patches of 1e30, which survive the
        # median), taps clamped at all four borders, taps in the last column and row
        cen = ih.warp_census(want_f, w, h, D.P_SCALE)
        print(f"{w}x{h} radius {r}: warp census of the filtered field {cen}")
        assert all(cen[k] > 0 for k in ih.CENSUS_KEYS), cen
    runs = []
    for i, around in enumerate(AROUND_P):
        f = Field(M.field_case("patched", w, h), 2 * (i + 1), AROUND_F[i])
        s = Plane(src, w + (0, 1, 61)[i], (0, 3, 64)[i], around)       # tightly packed, an odd pitch, a padded one
        o = Guarded(np.float32, 1, h, 2 * w, 2 * w, 2)
        d = Guarded(np.uint8, 1, h, w, dst_pitch, (4, 8, 1)[i] if dst_pitch % 4 == 0 else i)
        _launch(eng, [_desc(eng, f, w, h, r, o.ptr, s, d.ptr, dst_pitch)])
        # the chain: the flow-only launch, then ofx_warp_levels of what it wrote (a plane of the session's pitch)
        o2 = Guarded(np.float32, 1, h, 2 * w, 2 * w, 4)
        _launch(eng, [_desc(eng, f, w, h, r, o2.ptr)])
        runs.append((f"surroundings {around:#x}", f, s, o, d, o2))
    torch.cuda.synchronize()
    for what, _, _, o, d, o2 in runs:
        got_f, clean_f = o.host()
        got_w, clean_w = d.host()
        got_f2, clean_f2 = o2.host()
        same(got_f[0].reshape(h, w, 2), want_f, f"{what}: d_dst_flow")
        same(got_f2[0].reshape(h, w, 2), want_f, f"{what}: d_dst_flow of the flow-only launch")
        same(got_w[0], want_w, f"{what}: d_dst")
        assert clean_f and clean_w and clean_f2, f"{what}: bytes around an output (beyond column w - 1 of a row included) were written"
        same(eng.warp_u8(src, got_f2[0].reshape(h, w, 2).copy(), float(D.P_SCALE)), got_w[0], f"{what}: the chain (flow-only launch + ofx_warp_levels)")


# ---- 3. several items in one launch -----------------------------------------------------------------------------------------------

def test_three_items_of_different_size_and_radius_in_one_launch(eng, oracle):
    import torch

    picks = [((263, 75), "salted", 2, True), ((5, 4), "ties", 1, False), ((65, 9), "noise", 2, True)]      # the largest first, then last
    for order in (picks, picks[::-1]):
        keep, descs = [], []
        for i, ((w, h), kind, r, warp) in enumerate(order):
            f = Field(M.field_case(kind, w, h), 2 + 2 * i, AROUND_F[i])
            o = Guarded(np.float32, 1, h, 2 * w, 2 * w, 4 - 2 * (i & 1))
            s = Plane(_source(w, h), w + i, i, AROUND_P[i]) if warp else None
            d = Guarded(np.uint8, 1, h, w, w + 3, i) if warp else None
            descs.append(_desc(eng, f, w, h, r, o.ptr, s, d.ptr if warp else None, w + 3 if warp else 0))
            keep.append((f, s, o, d, (w, h), kind, r))
        _launch(eng, descs)
        torch.cuda.synchronize()
        for i, (_, _, o, d, (w, h), kind, r) in enumerate(keep):
            got, clean = o.host()
            same(got[0].reshape(h, w, 2), M.want(kind, w, h, r), f"item {i} of 3, {w}x{h} radius {r}")
            assert clean, f"item {i}: bytes around the field were written"
            if d is not None:
                got_w, clean_w = d.host()
                same(got_w[0], oracle.warp_bilinear_u8(_source(w, h), M.want(kind, w, h, r), D.P_SCALE), f"item {i}: d_dst")
                assert clean_w, f"item {i}: bytes around the image were written"


def test_sixteen_items_in_one_launch(eng):
    import torch

    shapes = [M.M_SHAPES[i % 6] for i in range(16)]
    keep, descs = [], []
    for i, (w, h) in enumerate(shapes):
        kind, r = M.M_KINDS[i % 4], 1 + (i // 2) % 2
        f = Field(M.field_case(kind, w, h), 2 + 2 * (i % 3), AROUND_F[i % 3])
        o = Guarded(np.float32, 1, h, 2 * w, 2 * w, 2 + 2 * (i & 1))
        descs.append(_desc(eng, f, w, h, r, o.ptr))
        keep.append((f, o, (w, h), kind, r))
    _launch(eng, descs)
    torch.cuda.synchronize()
    for i, (_, o, (w, h), kind, r) in enumerate(keep):
        got, clean = o.host()
        same(got[0].reshape(h, w, 2), M.want(kind, w, h, r), f"item {i} of 16, {w}x{h} {kind} radius {r}")
        assert clean, f"item {i}: bytes around the field were written"


# ---- 4. the session driver against the referee, every level -----------------------------------------------------------------------

S_SHAPES = [(192, 128, 4), (204, 108, 3)]       # the latter: an odd coarsest level (51x27), level widths 204 / 102 / 51 = 0, 2, 3 mod 4
WIN = 9


@functools.lru_cache(maxsize=None)
def _frames(kind, w, h):
    if kind == "smooth":
        from cuda_optical_flow_2_amd import synth

        return tuple(synth.smooth_pair(w, h, 2.5 * i, -1.25 * i, seed=w + WIN)[1] for i in range(2))
    seam = ih.tile_out_w(WIN >> 1)
    return tuple(ih.hard_frames(w, h, 2, seam_x=seam if seam < w else None))


def _scratch(s, lead=4):
    """the session's median scratch inside a buffer of 0x5A: (buffer, pointer, bytes)"""
    import torch

    n = C.c_size_t()
    s.L.ofx_session_dense_median_scratch_bytes(s._h, C.byref(n))
    assert n.value == sum((s.width >> k) * (s.height >> k) * 8 for k in range(s.levels))
    buf = torch.full((8 * lead + n.value + 256,), FILL, dtype=torch.uint8, device="cuda")
    return buf, buf.data_ptr() + 8 * lead, n.value


def _session_pair(eng, fr, levels, iters, min_det, r, mode="lk_float", then_plain=False):
    """(the median flow pyramid of the pair, the scratch's surroundings clean?, [run_flow_dense's pyramid afterwards])"""
    import torch

    h, w = fr[0].shape
    s = eng.Session(w, h, levels, WIN, mode, iters=iters, min_det=min_det)
    try:
        s.push_frame_host(fr[0])
        s.set_frame_host(fr[1])
        s.build_pyramid()
        buf, ptr, n = _scratch(s)
        eng.check(s.L.ofx_session_run_flow_dense_median(s._h, float(WIN), r, ptr, n, eng._stream_ptr()), "run_flow_dense_median")
        torch.cuda.synchronize()
        got = [s.flow_host(k) for k in range(levels)]
        raw = buf.cpu().numpy()
        clean = bool((raw[:ptr - buf.data_ptr()] == FILL).all() and (raw[ptr - buf.data_ptr() + n:] == FILL).all())
        plain = None
        if then_plain:
            s.run_flow_dense()
            torch.cuda.synchronize()
            plain = [s.flow_host(k) for k in range(levels)]
    finally:
        s.close()
    return got, clean, plain


@pytest.mark.parametrize("r", [1, 2])
@pytest.mark.parametrize("iters", [1, 2, 3])
@pytest.mark.parametrize("shape", S_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}-L{s[2]}")
def test_run_flow_dense_median_equals_the_referee(eng, oracle, shape, iters, r):
    """Every level of the session's dense flow with median against median_ref.dense_pair_median: both parities of the ping-pong
    between the session's flow planes and the scratch, min_det 0 and 1.0, on a smooth pair and on the hard frames of
    tests/iter_hard.py, whose flat blocks put NaN in front of the filter; the scratch's surroundings stay clean; and
    run_flow_dense on the same session afterwards is still dense_ref.dense_pair."""
    w, h, levels = shape
    nonfinite = 0
    for kind in ("hard", "smooth"):
        fr = _frames(kind, w, h)
        for min_det in (0.0, 1.0):
            then_plain = kind == "hard" and min_det == 0.0
            got, clean, plain = _session_pair(eng, fr, levels, iters, min_det, r, then_plain=then_plain)
            want = M.dense_pair_median(oracle, fr[0], fr[1], levels, WIN, iters, min_det, None, r)
            for k in range(levels - 1, -1, -1):
                same(got[k], want[k], f"{kind} iters {iters} min_det {min_det} radius {r}: level {k}")
            assert clean, "bytes around the scratch were written"
            if then_plain:
                ref = D.dense_pair(oracle, fr[0], fr[1], levels, WIN, iters, min_det)
                for k in range(levels):
                    same(plain[k], ref[k], f"run_flow_dense after the median call: level {k}")
                nonfinite += int(sum((~np.isfinite(x)).sum() for x in ref))
    assert nonfinite > 0, "the hard frames were meant to put NaN in front of the filter"


@pytest.mark.parametrize("iters", [2, 3])
def test_lk_float_fast(eng, oracle, iters):
    """lk_float_fast's solve is within 1 ulp of lk_float's, so its pyramid is compared the way test_gpu_dense.py treats the mode: by
    the score.  The median itself is exact in either mode: it is applied here to the session's own result of the top level."""
    prev, nxt, truth = D.scene("split", 41)
    got = eng.flow_pair_dense(prev, nxt, D.S_LEVELS, D.S_WIN, iters=iters, min_det=D.S_MIN_DET, mode="lk_float_fast", median=2)
    sc = D.score(IR.displacement(got[0], None, D.ITER_SCALE), truth)
    print(f"split seed 41 iters {iters}: lk_float_fast with the 5x5 median scores {sc:.3f}")
    assert sc >= 0.97, sc
    top = eng.flow_pair(prev, nxt, D.S_LEVELS, D.S_WIN, "lk_float_fast", iters=iters, min_det=D.S_MIN_DET)[D.S_LEVELS - 1]
    same(got[D.S_LEVELS - 1], M.median(top, 2), "the top level: the median of what run_flow leaves there")


def test_timing_records_the_medians_as_warps(eng):
    import torch

    w, h, levels, iters = 96, 64, 4, 3
    fr = _frames("smooth", w, h)
    s = eng.Session(w, h, levels, WIN, "lk_float", iters=iters, min_det=1.0)
    try:
        s.push_frame_host(fr[0])
        s.set_frame_host(fr[1])
        s.build_pyramid()
        s.timing(64)
        s.run_flow_dense(median=2)
        torch.cuda.synchronize()
        assert s.timing_read_kind("warp")[2] == (levels - 1) * (1 + iters) + 1, "a prolongation and iters medians per level below the top, one median above"
        assert s.timing_read_kind("lk_acc")[2] >= (levels - 1) * iters, "the accumulating launches below the top write no warped image"
        assert s.timing_read_kind("shift")[2] == 0 and s.timing_read_kind("corner")[2] == 0, "nothing is shifted"
    finally:
        s.close()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------

def _refused(eng, s, code, word, radius=2, ptr=None, n=None, max_px=9.0):
    buf, p, size = _scratch(s)
    rc = s.L.ofx_session_run_flow_dense_median(s._h, max_px, radius, p if ptr is None else ptr(p), size if n is None else n(size), eng._stream_ptr())
    msg = s.L.ofx_last_error()
    assert rc == code and msg and word in msg, (rc, msg)


def test_refusals(eng):
    import torch
    from cuda_optical_flow_2_amd.parallel import ShardPlan

    w, h, levels = 128, 64, 2
    fr = _frames("smooth", w, h)
    sessions = [(eng.Session(w, h, levels, WIN, "lk_float", shard=ShardPlan(w, h, levels, WIN, 0, 2)), OFX_E_UNSUPPORTED, b"sharded"),
                (eng.Session(w, h, levels, WIN, "compat_cpu"), OFX_E_UNSUPPORTED, b"lk_float"),
                (eng.Session(w, h, levels, WIN, "lk_float", borrow_frames=True), OFX_E_UNSUPPORTED, b"borrow_frames"),
                (eng.Session(w, h, levels, WIN, "lk_float"), OFX_E_STATE, b"frame")]
    try:
        for s, code, word in sessions:
            _refused(eng, s, code, word)
        s = sessions[-1][0]
        s.set_frame_host(fr[0])                              # a next frame alone is not a pair
        s.build_pyramid()
        _refused(eng, s, OFX_E_STATE, b"frame")
        s.swap()                                             # ... nor is a previous frame alone
        _refused(eng, s, OFX_E_STATE, b"frame")
        s.set_frame_host(fr[1])
        s.build_pyramid()
        for bad in (-1.0, float("nan"), float("inf")):
            _refused(eng, s, OFX_E_INVALID, b"max_px", max_px=bad)
        for radius in (0, 3, -1):
            _refused(eng, s, OFX_E_INVALID, b"radius", radius=radius)
        _refused(eng, s, OFX_E_INVALID, b"null", ptr=lambda p: None)
        _refused(eng, s, OFX_E_INVALID, b"aligned", ptr=lambda p: p + 4)
        _refused(eng, s, OFX_E_INVALID, b"scratch", n=lambda size: size - 1)
        _refused(eng, s, OFX_E_INVALID, b"scratch", n=lambda size: 0)
        with pytest.raises(eng.OfxError):
            s.run_flow_dense(median=3)
        s.run_flow_dense(median=1)                           # and with everything in place it runs, on the session's own scratch
        s.run_flow_dense(median=2)
        torch.cuda.synchronize()
        assert s._median_scratch is not None and s._median_scratch.numel() * 4 == sum((w >> k) * (h >> k) * 8 for k in range(levels))
    finally:
        for s, _, _ in sessions:
            s.close()


# ---- 6. quality on the device -----------------------------------------------------------------------------------------------------

def _clip(frames):
    import torch

    return torch.from_numpy(np.stack(frames)).cuda()


@pytest.mark.parametrize("seed", [41, 7])
def test_video_displacement_dense_with_median_on_two_motions(eng, oracle, seed):
    prev, nxt, truth = D.scene("split", seed)
    got = eng.video_displacement_dense(_clip([prev, nxt]), D.S_LEVELS, D.S_WIN, iters=D.S_ITERS, min_det=D.S_MIN_DET, median=2)
    assert tuple(got.shape) == (1, D.S_H, D.S_W, 2)
    got = got[0].cpu().numpy()
    want = M.dense_displacement_median(oracle, prev, nxt, D.S_LEVELS, D.S_WIN, D.S_ITERS, D.S_MIN_DET, None, 2)
    sc, cpu = D.score(got, truth), D.score(want, truth)
    print(f"split seed {seed}: score with the 5x5 median on the device {sc:.3f}, on the CPU {cpu:.3f}")
    assert abs(sc - cpu) <= 0.01, (sc, cpu)
    same(got, want, f"split, seed {seed}: level-0 displacement")
    # median = 0 is what the call did before
    plain = eng.video_displacement_dense(_clip([prev, nxt]), D.S_LEVELS, D.S_WIN, iters=D.S_ITERS, min_det=D.S_MIN_DET)[0].cpu().numpy()
    same(plain, D.dense_displacement(oracle, prev, nxt, D.S_LEVELS, D.S_WIN, D.S_ITERS, D.S_MIN_DET), "median = 0")


def test_video_interpolate_dense_with_median(eng):
    step = (2.0, 1.0)
    frames = IR.quality_clip(step)
    clip = _clip([frames[0], frames[4], frames[8]])
    kw = dict(factor=4, iters=3, min_det=D.S_MIN_DET)
    with_median, fwd, bwd = eng.video_interpolate_dense(clip, IR.Q_LEVELS, IR.Q_WIN, median=2, return_displacements=True, **kw)
    with_median = with_median.cpu().numpy()
    without = eng.video_interpolate_dense(clip, IR.Q_LEVELS, IR.Q_WIN, **kw).cpu().numpy()
    _, cfwd, cbwd = eng.video_interpolate_colour_dense(clip[..., None].expand(-1, -1, -1, 3).contiguous(), IR.Q_LEVELS, IR.Q_WIN, median=2,
                                                       return_displacements=True, **kw)

    def ratios(out):
        return [IR.sad(out[p, k - 1], frames[4 * p + k]) / IR.sad(IR.cross_fade(frames[4 * p], frames[4 * p + 4], F32(k / 4)), frames[4 * p + k])
                for p in (0, 1) for k in (1, 2, 3)]

    rm, r0 = ratios(with_median), ratios(without)
    print(f"step {step}: SAD(interp) / SAD(cross-fade) on the device: 5x5 median {min(rm):.3f} .. {max(rm):.3f}, no median {min(r0):.3f} .. {max(r0):.3f}")
    assert max(rm) < max(r0), (rm, r0)
    # a grey clip as colour: its channel average is the grey clip, so the colour call's rings are the grey call's
    same(cfwd.cpu().numpy(), fwd.cpu().numpy(), "video_interpolate_colour_dense(median=2): the forward ring")
    same(cbwd.cpu().numpy(), bwd.cpu().numpy(), "video_interpolate_colour_dense(median=2): the backward ring")
    want = eng.video_displacement_dense(clip, IR.Q_LEVELS, IR.Q_WIN, iters=3, min_det=D.S_MIN_DET, median=2)
    same(fwd.cpu().numpy(), want.cpu().numpy(), "the forward ring is video_displacement_dense(median=2)")
