"""Every window instance of the stream tick, of the level kernel and of the plain iteration launches on the GPU, each against a
referee the project already has (the lists and what they are for: tests/lk_instances.py; that together they select every instance:
tests/test_lk_instances_plan.py; that the hard frames reach what they are meant to: tests/test_iter_hard_ref.py).

    T0  the plain tick (stream_kernel, WOUT 0), plain and deep fetch, lk_float / compat_cpu: the oracle's pair, by the bits;
        lk_float_fast: within one ulp of the oracle's first iteration, identical NaN and Inf
    T3  the tick that also warps (WOUT 3) and the ITER 1 launch behind it: the oracle's two iterations by the bits; lk_float_fast
        step by step
    T5  row windows of three logical ranks (WOUT 5, ITER 4, ITER 1): the ranks' rows put together are the oracle's three
        iterations by the bits; lk_float_fast: an unsharded session's, by the bits
    L   lk_level_kernel: sums and flow as test_gpu_parity.test_level_sums_and_flow compares them; lk_float_fast within one ulp

After a HIP runtime error (not a mismatch) nothing more is launched: every later case fails at once with "not run"."""
import os

import numpy as np
import pytest

from cuda_optical_flow_2_amd import synth
from conftest import assert_flow_close, assert_same
import iter_hard as ih
import lk_instances as li
from test_gpu_iter_hard import _device_frames, _run, fast_steps_against_the_oracle
from test_gpu_iteration_pairs import _stream
from test_gpu_parity import _oracle_level, _oracle_sums

pytestmark = pytest.mark.gpu

_stop = []      # why nothing more is launched
_cache = {}     # references shared between cases


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    # both are read once per process and would override what the cases ask for (Session(deep_fetch=...), the plain launches)
    assert "OFX_LK_DMA" not in os.environ and "OFX_ITER_DMA" not in os.environ, "OFX_LK_DMA and OFX_ITER_DMA must be unset for this module"
    from cuda_optical_flow_2_amd import engine

    return engine


def _launching(what, fn):
    """fn(), unless a device error came before; a HIP runtime error (OFX_E_HIP, or one torch reports) ends the module's launches"""
    from cuda_optical_flow_2_amd.lib import OfxError

    if _stop:
        pytest.fail(f"not run: {_stop[0]}")
    try:
        return fn()
    except AssertionError:
        raise
    except Exception as e:
        if not isinstance(e, OfxError) or "(code 2)" in str(e):
            _stop.append(f"{what} ended in a device error: {type(e).__name__}: {str(e)[:300]}")
        raise


def _hard_frames(c, nf=5):
    """the first frames of a streamed case (a frame does not depend on how many follow it): shared by the cases of a window"""
    key = ("frames", c.w, c.h, c.seam_x, c.level, c.block)
    if key not in _cache:
        _cache[key] = ih.hard_frames(c.w, c.h, nf, seam_x=c.seam_x, level=c.level, block=c.block, corner=c.corner)
    return _cache[key][:ih.n_frames(c)]


def _oracle_pair(oracle, c, frames, p, mode):
    key = ("pair", c.w, c.h, c.win, mode, p)
    if key not in _cache:
        _cache[key] = oracle.flow_pair(synth.to_3ch(frames[p - 1]), synth.to_3ch(frames[p]), c.levels, c.win, mode, exact_sums=True)[0]
    return _cache[key]


# ---- T0 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", li.T0_CASES, ids=[t.id for t in li.T0_CASES])
def test_plain_tick_of_every_window(eng, oracle, t):
    """stream_kernel<R, MODE, FAST, DMA, WOUT 0> through Session(deep_fetch=-1 / +1), one iteration, 2 B + 1 hard frames.

    lk_float_fast: two cases (windows 3 and 23, B = 2) are why csrc/lk_solve.h sends a numerator that cancels through the replay:
    at the right edge of the flat block Sxy Sxt - Sxx Syt is exactly 0 at 21 pixels, where the numerator-first form returned 0.0
    and the reference's operation order, which the oracle replays, its own rounding noise (<= 5.7e-14 px, 6e8 float ulps)."""
    c = t.case
    frames = _hard_frames(c)
    got = _launching(t.id, lambda: _stream(eng, _device_frames(c, frames), c.w, c.h, c.levels, c.win, t.mode, 1, c.B, deep_fetch=t.deep))
    if t.mode == "lk_float_fast":
        fast_steps_against_the_oracle(oracle, c, frames, {1: got})
        return
    nonfinite = False
    for p in got:
        want = _oracle_pair(oracle, c, frames, p, t.mode)
        nonfinite |= not np.isfinite(want[0]).all()
        for k in range(c.levels):
            assert_same(got[p][k], want[k], f"{t.id}: pair {p} level {k}")
    assert nonfinite, "the frames were meant to produce non-finite flows"


# ---- T3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", li.T3_CASES, ids=[c.id for c in li.T3_CASES])
def test_warping_tick_of_every_window(eng, oracle, monkeypatch, case):
    """stream_kernel<R, lk_float, false, false, WOUT 3> and ITER 1 behind it: two iterations, every pair, both levels"""
    frames = _hard_frames(case)
    got = _launching(case.id, lambda: _run(eng, monkeypatch, case, frames))       # (asserts acc == ticks)
    nonfinite = False
    for p in got:
        want = oracle.flow_pair_iter(frames[p - 1], frames[p], case.levels, case.win, case.iters)
        nonfinite |= not np.isfinite(want[0]).all()
        for k in range(case.levels):
            assert_same(got[p][k], want[k], f"{case.id}: pair {p} level {k}")
    assert nonfinite, "the frames were meant to produce non-finite flows"


@pytest.mark.parametrize("case", li.T3_CASES, ids=[c.id for c in li.T3_CASES])
def test_warping_tick_of_every_window_fast(eng, oracle, monkeypatch, case):
    """... in lk_float_fast: sessions of one and of two iterations, step by step (test_gpu_iter_hard.test_fast_solve_step_by_step)"""
    frames = _hard_frames(case)
    runs = _launching(case.id, lambda: {j: _run(eng, monkeypatch, case, frames, "lk_float_fast", iters=j) for j in (1, 2)})
    fast_steps_against_the_oracle(oracle, case, frames, runs)


# ---- T5 ---------------------------------------------------------------------------------------------------------------------------
def _ranks(eng, c, mode, frames):
    """({pair: flow pyramid, the ranks' rows put together}, [status of every rank]): deep_child.run_rows for a case of T5"""
    import torch

    ranks = [eng.Session(c.w, c.h, c.levels, c.win, mode, shard=pl, local_corner=True, stream_batch=c.B, iters=c.iters, strict=False)
             for pl in li.shard_plans(c)]
    got, seen = {}, 0
    for s in ranks:
        s.stream_begin()

    def snap(done):
        nonlocal seen
        if done >= 1:
            for p in range(max(seen + 1, done - c.B + 1), done + 1):
                got[p] = [torch.cat([s.flow_of(p, k)[0] for s in ranks], dim=0).cpu().numpy() for k in range(c.levels)]
            seen = done
    for f in frames:
        snap([s.stream_submit(f) for s in ranks][0])
    while True:
        d = [s.stream_drain() for s in ranks][0]
        if d == -2:
            break
        snap(d)
    torch.cuda.synchronize()
    status = [s.corner_status() for s in ranks]
    for s in ranks:
        s.close()
    assert sorted(got) == list(range(1, len(frames))), f"{c.id}: pairs {sorted(got)} came out"
    return got, status


@pytest.mark.parametrize("mode", li.T5_MODES)
@pytest.mark.parametrize("c", li.T5_CASES, ids=[c.id for c in li.T5_CASES])
def test_row_windows_of_every_window(eng, oracle, c, mode):
    """stream_kernel<..., WOUT 5>, ITER 4 and ITER 1 on the row windows of three logical ranks, three iterations, smooth frames"""
    frames = li.rows_frames(c)
    dev = _device_frames(c, frames)
    got, status = _launching(f"{c.id}-{mode}", lambda: _ranks(eng, c, mode, dev))
    assert status == [0] * c.ranks, f"{c.id} {mode}: status {[hex(x) for x in status]}"
    if mode == "lk_float":
        want = {p: oracle.flow_pair_iter(frames[p - 1], frames[p], c.levels, c.win, c.iters) for p in got}
    else:   # the choice of formula is per pixel (test_fast_solve_through_every_path): an unsharded session gives the same bits
        want = _launching(f"{c.id}-{mode} unsharded", lambda: _stream(eng, dev, c.w, c.h, c.levels, c.win, mode, c.iters, c.B))
    for p in got:
        for k in range(c.levels):
            assert got[p][k].shape == ((c.h >> k), (c.w >> k), 2)
            assert_same(got[p][k], want[p][k], f"{c.id} {mode}, {c.ranks} ranks: pair {p} level {k}")


# ---- L ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", li.L_CASES, ids=[c.id for c in li.L_CASES])
def test_level_kernel_of_every_window(eng, oracle, c):
    """lk_level_kernel<R, MODE, SUMS, FAST> on two tiles, the second one column wide, the flat block across the seam"""
    p, n = li.level_pair(c)
    got = _launching(c.id, lambda: eng.lk_level(p, n, c.win, c.mode, want_sums=c.sums))
    if c.sums:
        want = _oracle_sums(oracle, p, n, c.win, c.mode)
        if c.mode == "compat_cpu":
            assert_same(got, want.astype(np.int64).astype(np.int32), f"{c.id}: sums")
        else:  # the oracle's planes are float (rounded once); the kernel's are the exact integers
            assert_same(got.astype(np.float32), want.astype(np.float32), f"{c.id}: sums")
        return
    key = ("level", c.w, c.win, "compat_cpu" if c.mode == "compat_cpu" else "lk_float")
    if key not in _cache:
        _cache[key] = _oracle_level(oracle, p, n, c.win, key[-1])
    want = _cache[key]
    assert not np.isfinite(want).all(), "the flat block was meant to produce non-finite flows"
    if c.mode == "lk_float_fast":
        assert_flow_close(got, want, 1, f"{c.id}: flow")
    else:
        assert_same(got, want, f"{c.id}: flow")
