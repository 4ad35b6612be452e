"""GPU: the coarse-to-fine dense flow -- the prolongation launch (ofx_flow_prolong), flow only and fused with the warp, against
tests/dense_ref.py, ofx_warp_levels and the oracle's warp; the session driver (ofx_session_run_flow_dense) against
dense_ref.dense_pair at every level; its refusals; and the quality of engine.video_displacement_dense / video_interpolate_dense on
the device.  Every comparison is by the bits (dense_ref.same_bits says what that means for a NaN).  Outputs sit in buffers of 0x5A,
inputs in larger buffers whose surroundings differ between runs, so that a tap outside an input, or a store outside an output,
shows."""
import functools

import numpy as np
import pytest

import dense_ref as D
import interp_ref as IR
import iter_hard as ih
from test_gpu_interp import AROUND_F, AROUND_P, Field, Guarded, Plane

pytestmark = pytest.mark.gpu

F32 = np.float32
OFX_E_UNSUPPORTED, OFX_E_STATE = 3, 4


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


@functools.lru_cache(maxsize=None)
def _want(kind, wc, hc, w, h, max_px):
    f = D.prolong(D.coarse_case(kind, wc, hc), w, h, D.P_SCALE, max_px)
    f.setflags(write=False)
    return f


def _desc(eng, coarse, wc, hc, fine, w, h, max_px, src=None, dst=None, dst_pitch=0):
    return eng._lib.ProlongDesc(coarse.ptr, wc, hc, fine, w, h, float(D.P_SCALE), float(max_px), None if src is None else src.ptr,
                                0 if src is None else src.pitch, dst, dst_pitch)


def _launch(eng, descs):
    lib = eng._lib.load()
    arr = (eng._lib.ProlongDesc * len(descs))(*descs)
    eng.check(lib.ofx_flow_prolong(arr, len(descs), eng._stream_ptr()), "ofx_flow_prolong")


# ---- 1. the prolongation, flow only -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", D.P_SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}")
def test_prolong_equals_the_referee(eng, shape):
    import torch

    (wc, hc), (w, h) = shape
    runs = []
    for ki, kind in enumerate(D.P_KINDS):
        for mi, max_px in enumerate((0.0, D.P_MAX_PX)):
            # (coarse lead, fine lead) in floats: both 16-byte aligned; a merely 8-byte aligned destination; a merely 8-byte aligned source
            for fl, dl in ((4, 4), (4, 2), (2, 4)):
                c = Field(D.coarse_case(kind, wc, hc), fl, AROUND_F[(ki + mi + fl) % 3])
                d = Guarded(np.float32, 1, h, 2 * w, 2 * w, dl)
                _launch(eng, [_desc(eng, c, wc, hc, d.ptr, w, h, max_px)])
                runs.append((f"{kind} max_px {max_px} leads {fl}/{dl}", c, d, _want(kind, wc, hc, w, h, max_px)))
    torch.cuda.synchronize()
    for what, _, d, want in runs:
        got, clean = d.host()
        same(got[0].reshape(h, w, 2), want, what)
        assert clean, f"{what}: bytes around the field were written"
    assert len(runs) == 18


def test_prolong_three_shapes_in_one_launch(eng):
    import torch

    picks = [(D.P_SHAPES[1], "salted", D.P_MAX_PX), (D.P_SHAPES[2], "noise", 0.0), (D.P_SHAPES[4], "salted", 0.0)]   # the largest first, then last
    for order in (picks, picks[::-1]):
        keep, descs = [], []
        for i, (((wc, hc), (w, h)), kind, max_px) in enumerate(order):
            c = Field(D.coarse_case(kind, wc, hc), 2 + 2 * i, AROUND_F[i])
            d = Guarded(np.float32, 1, h, 2 * w, 2 * w, 4 - 2 * (i & 1))
            descs.append(_desc(eng, c, wc, hc, d.ptr, w, h, max_px))
            keep.append((c, d, (w, h), _want(kind, wc, hc, w, h, max_px)))
        _launch(eng, descs)
        torch.cuda.synchronize()
        for i, (_, d, (w, h), want) in enumerate(keep):
            got, clean = d.host()
            same(got[0].reshape(h, w, 2), want, f"descriptor {i} of 3, {w}x{h}")
            assert clean, f"descriptor {i}: bytes around the field were written"


# ---- 2. fused with the warp, against the chain ------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _source(w, h):
    return IR.planes(w, h, seed=3)[0].copy()       # (writable: the engine's helpers hand it to torch)


@pytest.mark.parametrize("case", [(D.P_SHAPES[0], "salted", 0.0, 272), (D.P_SHAPES[1], "salted", 0.0, 267), (D.P_SHAPES[1], "salted", D.P_MAX_PX, 320),
                                  (D.P_SHAPES[0], "smooth", D.P_MAX_PX, 262), (D.P_SHAPES[5], "noise", 0.0, 261), (D.P_SHAPES[4], "salted", 0.0, 3),
                                  (D.P_SHAPES[2], "salted", 0.0, 12)],
                         ids=lambda c: f"{c[0][1][0]}x{c[0][1][1]}-{c[1]}-max{c[2]:g}-pitch{c[3]}")
def test_fused_warp_equals_the_chain(eng, oracle, case):
    import torch

    ((wc, hc), (w, h)), kind, max_px, dst_pitch = case
    want_f = _want(kind, wc, hc, w, h, max_px)
    src = _source(w, h)
    want_w = oracle.warp_bilinear_u8(src, want_f, D.P_SCALE)
    if kind == "salted" and w > 100 and max_px == 0.0:
        # the field is what the case says: pixels that are not warped, taps clamped at all four borders, taps in the last column and row
        cen = ih.warp_census(want_f, w, h, D.P_SCALE)
        assert all(cen[k] > 0 for k in ih.CENSUS_KEYS), cen
    same(eng.warp_u8(src, np.array(want_f), float(D.P_SCALE)), want_w, "ofx_warp_levels of the referee's flow against the oracle's warp")
    runs = []
    for i, around in enumerate(AROUND_P):
        c = Field(D.coarse_case(kind, wc, hc), 2 * (i + 1), AROUND_F[i])
        s = Plane(src, w + (0, 1, 61)[i], (0, 3, 64)[i], around)       # tightly packed, an odd pitch, a padded one
        f = Guarded(np.float32, 1, h, 2 * w, 2 * w, 2)
        d = Guarded(np.uint8, 1, h, w, dst_pitch, (4, 8, 1)[i] if dst_pitch % 4 == 0 else i)
        _launch(eng, [_desc(eng, c, wc, hc, f.ptr, w, h, max_px, s, d.ptr, dst_pitch)])
        runs.append((f"surroundings {around:#x}", c, s, f, d))
    torch.cuda.synchronize()
    for what, _, _, f, d in runs:
        got_f, clean_f = f.host()
        got_w, clean_w = d.host()
        same(got_f[0].reshape(h, w, 2), want_f, f"{what}: d_fine")
        same(got_w[0], want_w, f"{what}: d_dst")
        assert clean_f and clean_w, f"{what}: bytes around an output (beyond column w - 1 of a row included) were written"


# ---- 3. the session driver against the referee, every level -----------------------------------------------------------------------

S_SHAPES = [(264, 80, 3), (520, 72, 3), (96, 64, 4)]       # level 0 of the first two crosses a tile seam of the LK launches
MIN_DETS = (0.0, 1.0)


@functools.lru_cache(maxsize=None)
def _frames(kind, w, h, win):
    if kind == "smooth":
        from cuda_optical_flow_2_amd import synth

        return tuple(synth.smooth_pair(w, h, 2.5 * i, -1.25 * i, seed=w + win)[1] for i in range(3))
    # the flat block across the tile seam of the accumulating launch where the level has one, stripes, noise (tests/iter_hard.py)
    seam = ih.tile_out_w(win >> 1)
    return tuple(ih.hard_frames(w, h, 3, seam_x=seam if seam < w else None))


def _dense_session(eng, frames, levels, win, iters, min_det, max_px, mode="lk_float"):
    """the dense flow pyramids of the consecutive pairs of `frames` through ONE session"""
    import torch

    h, w = frames[0].shape
    s = eng.Session(w, h, levels, win, mode, iters=iters, min_det=min_det)
    out = []
    try:
        s.push_frame_host(frames[0])
        for f in frames[1:]:
            s.set_frame_host(f)
            s.build_pyramid()
            s.run_flow_dense(max_px)
            torch.cuda.synchronize()
            out.append([s.flow_host(k) for k in range(levels)])
            s.swap()
    finally:
        s.close()
    return out


@pytest.mark.parametrize("win", [5, 9, 13])
@pytest.mark.parametrize("shape", S_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}-L{s[2]}")
def test_run_flow_dense_equals_the_referee(eng, oracle, shape, win):
    """Every level of the session's dense flow against dense_ref.dense_pair (the oracle's LK and warp around the NumPy prolongation):
    iters 1, 2, 3 x min_det 0, 1.0 x max_px 0, the window, on the hard frames of tests/iter_hard.py (flat block across a tile seam,
    stripes, noise: NaN and huge vectors reach the prolongation) and on a smooth pair."""
    w, h, levels = shape
    runs = [(kind, it, md, mp) for kind in ("hard", "smooth") for it in (1, 2, 3) for md in MIN_DETS for mp in (0.0, float(win))]
    runs += [("smooth", 0, 1.0, None)]                   # (iters = 0 counts as 1; max_px None: the window)
    nonfinite = huge = 0
    for kind, iters, min_det, max_px in runs:
        fr = _frames(kind, w, h, win)[:2]
        got = _dense_session(eng, fr, levels, win, iters, min_det, max_px)[0]
        want = D.dense_pair(oracle, fr[0], fr[1], levels, win, iters, min_det, max_px)
        for k in range(levels - 1, -1, -1):
            same(got[k], want[k], f"{kind} iters {iters} min_det {min_det} max_px {max_px}: level {k}")
        if kind == "hard" and min_det == 0.0:
            coarse = np.concatenate([x.reshape(-1) for x in want[1:]])
            nonfinite += int((~np.isfinite(coarse)).sum())
            with np.errstate(invalid="ignore"):
                huge += int((np.abs(coarse) * float(D.ITER_SCALE) > win).sum())
    # (on the oracle alone: every case has NaN in a coarse level; vectors beyond max_px = the window come with the 5x5 window)
    assert nonfinite > 0 and (huge > 0 or win != 5), "the hard frames were meant to send NaN and huge vectors into the prolongation"


def test_a_second_pair_after_swap_and_run_flow_afterwards(eng, oracle):
    import torch

    w, h, levels, win, iters, min_det = 264, 80, 3, 9, 3, 0.0
    fr = _frames("hard", w, h, win)
    both = _dense_session(eng, fr, levels, win, iters, min_det, None)
    fresh = _dense_session(eng, fr[1:], levels, win, iters, min_det, None)[0]
    for k in range(levels):
        same(both[1][k], fresh[k], f"pair 2 of a session against a fresh session: level {k}")
        same(both[1][k], D.dense_pair(oracle, fr[1], fr[2], levels, win, iters, min_det)[k], f"pair 2 against the referee: level {k}")
    # run_flow on the pair the dense call has just run: its own result, as a session that never ran the dense call gives it
    s = eng.Session(w, h, levels, win, "lk_float", iters=iters, min_det=min_det)
    try:
        s.push_frame_host(fr[0])
        s.set_frame_host(fr[1])
        s.build_pyramid()
        s.run_flow_dense()
        s.run_flow()
        torch.cuda.synchronize()
        got = [s.flow_host(k) for k in range(levels)]
        s.run_flow_dense()                                   # ... and the dense call after run_flow, its own again
        torch.cuda.synchronize()
        again = [s.flow_host(k) for k in range(levels)]
    finally:
        s.close()
    want = eng.flow_pair(fr[0], fr[1], levels, win, "lk_float", iters=iters, min_det=min_det)
    for k in range(levels):
        same(got[k], want[k], f"run_flow after run_flow_dense: level {k}")
        same(again[k], both[0][k], f"run_flow_dense after run_flow: level {k}")


def test_timing_records_the_prolongation_as_a_warp(eng):
    import torch

    w, h, levels, win, iters = 96, 64, 4, 9, 3
    fr = _frames("smooth", w, h, win)
    s = eng.Session(w, h, levels, win, "lk_float", iters=iters, min_det=1.0)
    try:
        s.push_frame_host(fr[0])
        s.set_frame_host(fr[1])
        s.build_pyramid()
        s.timing(64)
        s.run_flow_dense()
        torch.cuda.synchronize()
        assert s.timing_read_kind("warp")[2] == levels - 1, "one prolongation per level below the top"
        # below the top: iters accumulating launches per level, all but the last also writing the warped image
        assert s.timing_read_kind("lk_acc_warp")[2] >= (levels - 1) * (iters - 1)
        assert s.timing_read_kind("lk_acc")[2] >= levels - 1
        assert s.timing_read_kind("shift")[2] == 0 and s.timing_read_kind("corner")[2] == 0, "nothing is shifted"
    finally:
        s.close()


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------

def _refused(eng, s, code, word):
    with pytest.raises(eng.OfxError) as e:
        s.run_flow_dense()
    assert f"(code {code})" in str(e.value) and word in str(e.value), str(e.value)


def test_refusals(eng):
    import torch
    from cuda_optical_flow_2_amd.parallel import ShardPlan

    w, h, levels, win = 128, 64, 2, 9
    fr = _frames("smooth", w, h, win)
    sessions = [(eng.Session(w, h, levels, win, "lk_float", shard=ShardPlan(w, h, levels, win, 0, 2)), OFX_E_UNSUPPORTED, "sharded"),
                (eng.Session(w, h, levels, win, "compat_cpu"), OFX_E_UNSUPPORTED, "lk_float"),
                (eng.Session(w, h, levels, win, "lk_float", borrow_frames=True), OFX_E_UNSUPPORTED, "borrow_frames"),
                (eng.Session(w, h, levels, win, "lk_float"), OFX_E_STATE, "frame")]
    try:
        for s, code, word in sessions:
            _refused(eng, s, code, word)
        s = sessions[-1][0]
        s.set_frame_host(fr[0])                              # a next frame alone is not a pair
        s.build_pyramid()
        _refused(eng, s, OFX_E_STATE, "frame")
        s.swap()                                             # ... nor is a previous frame alone
        _refused(eng, s, OFX_E_STATE, "frame")
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(eng.OfxError) as e:
                s.run_flow_dense(bad)
            assert "(code 1)" in str(e.value) and "max_px" in str(e.value)
        s.set_frame_host(fr[1])
        s.build_pyramid()
        s.run_flow_dense()                                   # and with both it runs
        torch.cuda.synchronize()
    finally:
        for s, _, _ in sessions:
            s.close()


# ---- 5. quality on the device -----------------------------------------------------------------------------------------------------

def _clip(frames):
    import torch

    return torch.from_numpy(np.stack(frames)).cuda()


@pytest.mark.parametrize("seed", [41, 7])
def test_video_displacement_dense_on_two_motions(eng, oracle, seed):
    prev, nxt, truth = D.scene("split", seed)
    got = eng.video_displacement_dense(_clip([prev, nxt]), D.S_LEVELS, D.S_WIN, iters=D.S_ITERS, min_det=D.S_MIN_DET)
    assert tuple(got.shape) == (1, D.S_H, D.S_W, 2)
    got = got[0].cpu().numpy()
    same(got, D.dense_displacement(oracle, prev, nxt, D.S_LEVELS, D.S_WIN, D.S_ITERS, D.S_MIN_DET), f"split, seed {seed}: level-0 displacement")
    sc = D.score(got, truth)
    print(f"split seed {seed}: dense score on the device {sc:.3f}")
    assert sc >= 0.85, sc
    # a coarser level, and flow_pair_dense: the same pyramid
    lvl1 = eng.video_displacement_dense(_clip([prev, nxt]), D.S_LEVELS, D.S_WIN, iters=D.S_ITERS, min_det=D.S_MIN_DET, level=1)[0].cpu().numpy()
    pyr = eng.flow_pair_dense(prev, nxt, D.S_LEVELS, D.S_WIN, iters=D.S_ITERS, min_det=D.S_MIN_DET)
    same(lvl1, IR.displacement(pyr[1], None, D.ITER_SCALE), "level 1")
    same(got, IR.displacement(pyr[0], None, D.ITER_SCALE), "level 0 of flow_pair_dense")


@pytest.mark.parametrize("seed", [41, 7])
def test_the_fast_solve_meets_the_same_bar(eng, seed):
    prev, nxt, truth = D.scene("split", seed)
    got = eng.video_displacement_dense(_clip([prev, nxt]), D.S_LEVELS, D.S_WIN, iters=D.S_ITERS, min_det=D.S_MIN_DET, mode="lk_float_fast")
    sc = D.score(got[0].cpu().numpy(), truth)
    print(f"split seed {seed}: dense score on the device, lk_float_fast {sc:.3f}")
    assert sc >= 0.85, sc


def test_video_interpolate_dense_on_a_moving_texture(eng):
    step = (2.0, 1.0)
    frames = IR.quality_clip(step)
    clip = _clip([frames[0], frames[4], frames[8]])
    dense, fwd, bwd = eng.video_interpolate_dense(clip, IR.Q_LEVELS, IR.Q_WIN, factor=4, iters=3, min_det=D.S_MIN_DET, return_displacements=True)
    exist = eng.video_interpolate(clip, IR.Q_LEVELS, IR.Q_WIN, "lk_float", factor=4, iters=3, min_det=D.S_MIN_DET)
    assert tuple(dense.shape) == tuple(exist.shape) == (2, 3, IR.Q_H, IR.Q_W)
    dense, exist = dense.cpu().numpy(), exist.cpu().numpy()

    def ratios(out):
        return [IR.sad(out[p, k - 1], frames[4 * p + k]) / IR.sad(IR.cross_fade(frames[4 * p], frames[4 * p + 4], F32(k / 4)), frames[4 * p + k])
                for p in (0, 1) for k in (1, 2, 3)]

    rd, re = ratios(dense), ratios(exist)
    print(f"step {step}: SAD(interp) / SAD(cross-fade) on the device: dense {min(rd):.2f} .. {max(rd):.2f}, existing {min(re):.2f} .. {max(re):.2f}")
    assert max(rd) < 0.25, rd
    assert max(rd) < max(re), (rd, re)
    # the frames are the definition's, from the two rings: fwd[p] is frame p -> p + 1, bwd[N - 2 - p] frame p + 1 -> p
    fwd, bwd = fwd.cpu().numpy(), bwd.cpu().numpy()
    for p in (0, 1):
        for k in (1, 2, 3):
            want = IR.interpolate(frames[4 * p], frames[4 * p + 4], fwd[p], bwd[1 - p], F32(k / 4))[0]
            same(dense[p, k - 1], want, f"pair {p}, t = {k}/4")
