"""Refinement iterations on hard frames against the CPU oracle, bit for bit, every window 3x3 .. 23x23.

The other iteration tests compare with the oracle on a smooth texture (finite, small flows; no clamped tap, no "no warp", no flat
window; widths that are multiples of 4; windows up to 9x9) and compare the hard content -- flat blocks, noise, odd widths, tile
seams, min_det, lk_float_fast -- between two GPU paths that share the march, the solve and the warp.  Here the reference is
oracle.flow_pair_iter (oracle/ofx_oracle.c, orc_lk_iter_level_guard) on the frames of tests/iter_hard.py; tests/test_iter_hard_ref.py
shows on the oracle alone that every case drives the warp into its "no warp" branch, its four clamps and the last column and row,
and has non-finite flows at the tile seam.  The shapes are the smallest with a tile seam and a ragged end."""
import numpy as np
import pytest

from cuda_optical_flow_2_amd import synth
from conftest import assert_flow_close, assert_same
import iter_hard as ih
from test_gpu_iteration_pairs import _frames, _stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cuda_optical_flow_2_amd import engine

    return engine


def _ids(cases):
    return [c.id for c in cases]


def _device_frames(case, frames):
    """the case's frames in device buffers of test_gpu_iteration_pairs._frames (a pitch of 64 bytes whatever the width)"""
    import torch

    # _frames is called for its buffers alone (the pitch handling lives in it and is taken by import, not copied): the frames it
    # synthesises and uploads are overwritten at once
    bufs = _frames(case.w, case.h, len(frames))
    for b, f in zip(bufs, frames):
        b.copy_(torch.from_numpy(np.ascontiguousarray(f)))
    return bufs


def _run(eng, monkeypatch, case, frames, mode="lk_float", iters=None, min_det=0.0):
    """{pair: flow pyramid} of a case through the path it names.  A streamed session must have run the launches the case is
    about: behind every tick with an LK stage, iterations 2 .. iters two at a time up to 9x9 (csrc/lk_body_pair.h; a left-over one
    alone), one at a time above -- the count test_iteration_pairs_equal_one_launch_per_iteration asserts.  A session that fell
    back to one launch per iteration would give the same bits and leave the fused launch untested."""
    iters = case.iters if iters is None else iters
    if case.kind == "pair":
        return {1: eng.flow_pair(frames[0], frames[1], case.levels, case.win, mode, iters=iters, min_det=min_det)}
    monkeypatch.setenv("OFX_ITER_PAIRS", "1")
    for k, v in case.env:
        monkeypatch.setenv(k, v)
    n = {}
    got = _stream(eng, _device_frames(case, frames), case.w, case.h, case.levels, case.win, mode, iters, case.B, launches=n, min_det=min_det)
    want_acc = (iters // 2 if iters >= 3 else iters - 1) if case.win <= 9 else iters - 1
    assert n["ticks"] > 0 and n["acc"] == n["ticks"] * want_acc, f"{case.id} iters {iters}: {n}, {want_acc} accumulating launches per tick expected"
    if dict(case.env).get("OFX_PAIR_WAVES"):
        # the packed plan straddles: more tile columns in a pair than waves, so some wave marches segments of several
        r, waves = case.win >> 1, int(dict(case.env)["OFX_PAIR_WAVES"])
        tiles = sum(-(-(case.w >> k) // ih.pair_out_w(r)) for k in range(case.levels))
        assert tiles > waves, f"{case.id}: {tiles} tile columns on {waves} waves do not straddle"
    return got


def _against_the_oracle(eng, oracle, monkeypatch, case, min_det=0.0):
    frames = ih.case_frames(case)
    got = _run(eng, monkeypatch, case, frames, min_det=min_det)
    assert sorted(got) == list(range(1, len(frames)))
    nonfinite = False
    for p in got:
        want = oracle.flow_pair_iter(frames[p - 1], frames[p], case.levels, case.win, case.iters, min_det=min_det)
        nonfinite |= not np.isfinite(want[0]).all()
        for k in range(case.levels):
            assert_same(got[p][k], want[k], f"{case.id} min_det {min_det}: pair {p} level {k}")
    return nonfinite


@pytest.mark.parametrize("case", ih.A_CASES, ids=_ids(ih.A_CASES))
def test_every_window_pair_at_a_time(eng, oracle, monkeypatch, case):
    """A.  Three iterations, pair at a time, windows 3x3 .. 23x23 (one instance of the accumulating launch per radius): two tiles
    of TileGeom<R>, the second one column wide, an odd width, the flat block across the seam; for the windows above 9x9 also as
    level 1 of a two-level pair."""
    assert _against_the_oracle(eng, oracle, monkeypatch, case), "the frames were meant to produce non-finite flows"


@pytest.mark.parametrize("shape", ih.B_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tiny_shapes_pair_at_a_time(eng, oracle, shape):
    """B.  Images smaller than the window, than a dword, than the lag of the march: three iterations on noise."""
    w, h, win = shape
    p, n = synth.random_pair(w, h, seed=w + win)
    got = eng.flow_pair(p, n, 1, win, "lk_float", iters=3)
    assert_same(got[0], oracle.flow_pair_iter(p, n, 1, win, 3)[0], f"{w}x{h} win {win}")


@pytest.mark.parametrize("case", ih.C_CASES, ids=_ids(ih.C_CASES))
def test_stream_pipeline_two_iterations_per_launch(eng, oracle, monkeypatch, case):
    """C.  The stream pipeline, pairs on: level-1 widths around the tile of the fused launch (TileGeomP<R>), 4 iterations (two
    fused launches less one) and 5, B = 1 and 2 with 2 B + 1 frames (full ticks and a drained partial one), one packed plan with a
    straddling wave, and windows 11 and 15 (one launch per iteration).  Every pair, both levels."""
    assert _against_the_oracle(eng, oracle, monkeypatch, case), "the frames were meant to produce non-finite flows"


@pytest.mark.parametrize("case", ih.D_CASES, ids=_ids(ih.D_CASES))
def test_determinant_guard_with_iterations(eng, oracle, monkeypatch, case):
    """D.  min_det on, against the guarded restatement: the guard after every iteration's solve.  In the three-level case pixel 0
    of levels 1 and 2 lies in a black corner: guarded it is (0, 0) and the level below is not shifted, unguarded it is NaN and the
    shift leaves the image (test_iter_hard_ref.py asserts both on the oracle), so a corner solve or a shift that ignored the
    guard would give level 0 and level 1 another next image."""
    _against_the_oracle(eng, oracle, monkeypatch, case, min_det=ih.MIN_DET)


def fast_steps_against_the_oracle(oracle, case, frames, runs):
    """The body of test_fast_solve_step_by_step: runs = {j: {pair: flow pyramid}} of lk_float_fast sessions of j = 1 .. case.iters
    iterations on `frames`.  tests/test_gpu_deep_iter.py calls it with the runs of a child process."""
    L, win = case.levels, case.win
    steps = exempt = 0
    for p in runs[1]:
        pp = oracle.gauss_pyramid(synth.to_3ch(frames[p - 1]), L)
        npyr = oracle.gauss_pyramid(synth.to_3ch(frames[p]), L)
        first = [runs[1][p][k] for k in range(L)]
        for k in range(L - 1, -1, -1):
            n3 = npyr[k] if k == L - 1 else oracle.shift_back_pyramid(npyr[k], k, L, first)
            prev1, next1 = np.ascontiguousarray(pp[k][:, :, 0]), np.ascontiguousarray(n3[:, :, 0])
            assert_flow_close(runs[1][p][k], oracle.lk_iter_level(prev1, next1, win, 1)[0], 1, f"{case.id}: F_1, pair {p} level {k}")
            for j in range(1, case.iters):
                s, e = ih.check_fast_step(oracle, prev1, next1, win, runs[j][p][k], runs[j + 1][p][k], f"{case.id}: pair {p} level {k} step {j} -> {j + 1}")
                steps += s
                exempt += e
    assert exempt <= 1e-3 * steps, f"{case.id}: {exempt} of {steps} values took the exception's bound"


@pytest.mark.parametrize("case", ih.E_CASES, ids=_ids(ih.E_CASES))
def test_fast_solve_step_by_step(eng, oracle, monkeypatch, case):
    """E.  lk_float_fast is not restated on the CPU and 1 ulp may flip a byte of the next warped image, so whole chains cannot be
    compared; single steps can.  F_j and F_{j+1} are the GPU's own (sessions of j and j + 1 iterations); the oracle makes the step
    from F_j (iter_hard.check_fast_step: 1 ulp of the step's solve, lk_solve.h's cancelling numerators by their own bound).  F_1
    against the oracle's first iteration with assert_flow_close(..., 1).  Streamed cases: level 1 is unshifted, level 0's next is
    the oracle's global shift by the GPU's own first-iteration level-1 flow."""
    frames = ih.case_frames(case)
    runs = {j: _run(eng, monkeypatch, case, frames, "lk_float_fast", iters=j) for j in range(1, case.iters + 1)}
    fast_steps_against_the_oracle(oracle, case, frames, runs)
