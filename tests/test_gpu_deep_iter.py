"""The deep-fetch form of the iteration launches (lk_iter_kernel<R, MODE, FAST, ITER, DMA = true>: a step's rows fetched two steps
ahead straight into LDS, counted waits; csrc/lk_launch.h, csrc/lk_body_buf.h) against the CPU oracle, bit for bit, at small shapes.

The form is what every 8K session runs (ofx_plan::iter_deep_fetch: a largest level of 16 Mpx or more) and what OFX_ITER_DMA=1
forces at any size.  The switch is read once per process, at the first LK launch, so each group of cases runs in a fresh child
process started with it (tests/deep_child.py, which only computes and stores); everything is compared here, on the CPU, with the
references of tests/test_gpu_iter_hard.py and tests/test_gpu_dense.py.  tests/test_deep_plan.py shows on the host that the launches
of these cases select the deep kernels.  At most two processes have the device open: this one and one child.

Every instance of the deep family -- 2 solves x ITER 1..4 x 11 radii = 88 kernels -- is run by some group: lk_float ITER 3, 2, 1 by A,
the fast ones by E (every window, step by step), ITER 4 and the ITER 1 behind it in both solves by R (the row windows of
tests/lk_instances.py's T5: lk_float against the oracle, lk_float_fast against an unsharded session run HERE, in the plain form, which
tests/test_gpu_lk_instances.py ties to the oracle); tests/test_deep_plan.py holds the census.

A child that a signal ended (or that aborted, or ran into its limit) has faulted the device or hung on it: no further child is
started after that, every later group fails at once.

The last test is in-process: the tick's deep form (stream_kernel<..., DMA = true>) is reachable through Session(deep_fetch=+1)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from cuda_optical_flow_2_amd import synth
from conftest import assert_same
import deep_child as dc
import dense_ref
import iter_hard as ih
import lk_instances as li
from test_gpu_iter_hard import _device_frames, fast_steps_against_the_oracle
from test_gpu_iteration_pairs import _stream

pytestmark = pytest.mark.gpu

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "deep_child.py")
CHILD_LIMIT = 600   # seconds: the limit of the other child-process test (test_gpu_surface.py); a group needs seconds
_stop = []          # why no further child is started


def _child(tmp_path_factory, group):
    """the arrays the child stored for `group`"""
    if _stop:
        pytest.fail(f"group {group} not started: {_stop[0]}")
    path = str(tmp_path_factory.mktemp("deep_" + group) / "out.npz")
    env = dict(os.environ, OFX_ITER_DMA="1")
    env.pop("OFX_LK_DMA", None)
    try:
        r = subprocess.run([sys.executable, CHILD, path, group], env=env, timeout=CHILD_LIMIT, capture_output=True)
    except subprocess.TimeoutExpired:
        _stop.append(f"the child of group {group} did not end within {CHILD_LIMIT} s")
        pytest.fail(_stop[0])
    out, err = r.stdout.decode(errors="replace"), r.stderr.decode(errors="replace")
    if r.returncode < 0 or r.returncode in (134, 139):
        _stop.append(f"the child of group {group} ended with status {r.returncode}: {err[-2000:]}")
        pytest.fail(_stop[0])
    if r.returncode != 0 or not out.rstrip().endswith("deep ok"):
        pytest.fail(f"the child of group {group} ended with status {r.returncode}: {out[-500:]} {err[-2000:]}")
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def _group(name):
    @pytest.fixture(scope="module", name="group_" + name)
    def fixture(tmp_path_factory):
        return _child(tmp_path_factory, name)

    return fixture


group_A, group_strips, group_C, group_D, group_E, group_dense, group_rows, group_R, group_Rstrips, group_B = \
    (_group(g) for g in ("A", "strips", "C", "D", "E", "dense", "rows", "R", "Rstrips", "B"))


def _ids(cases):
    return [c.id for c in cases]


def _pairs(got, prefix, case):
    """{pair: flow pyramid} of what the child stored under prefix"""
    return {p: [got[dc.key(prefix, f"pair{p}", f"level{k}")] for k in range(case.levels)] for p in range(1, ih.n_frames(case))}


def _against_the_oracle(oracle, got, prefix, case, min_det=0.0):
    """test_gpu_iter_hard._against_the_oracle on the child's arrays; a streamed case must have run one launch per iteration"""
    frames = ih.case_frames(case)
    if case.kind == "stream":
        ticks, acc = int(got[dc.key(prefix, "ticks")]), int(got[dc.key(prefix, "acc")])
        assert ticks > 0 and acc == ticks * (case.iters - 1), f"{case.id}: {ticks} ticks, {acc} accumulating launches: the session did not see the switch"
    nonfinite = False
    for p, pyr in _pairs(got, prefix, case).items():
        want = oracle.flow_pair_iter(frames[p - 1], frames[p], case.levels, case.win, case.iters, min_det=min_det)
        nonfinite |= not np.isfinite(want[0]).all()
        for k in range(case.levels):
            assert_same(pyr[k], want[k], f"{case.id} min_det {min_det}: pair {p} level {k}")
    return nonfinite


@pytest.mark.parametrize("case", dc.A_CASES, ids=_ids(dc.A_CASES))
def test_every_window_pair_at_a_time(oracle, group_A, case):
    """A.  ITER 3, ITER 2 and ITER 1 of every radius: the cases of test_gpu_iter_hard.py's A."""
    assert _against_the_oracle(oracle, group_A, dc.key("A", case.id), case), "the frames were meant to produce non-finite flows"


@pytest.mark.parametrize("min_strip", dc.MIN_STRIPS)
@pytest.mark.parametrize("case", dc.STRIP_CASES, ids=_ids(dc.STRIP_CASES))
def test_one_strip_per_tile_column_and_strips_of_one_row(oracle, group_strips, case, min_strip):
    """strips.  OFX_LK_MIN_STRIP=1000: a wave marches a whole tile column and refreshes its row table on the way (once at 67 rows,
    twice at 132); =1: a wave marches one row, primes more rows than it takes, and must have drained its fetches before it ends."""
    assert _against_the_oracle(oracle, group_strips, dc.key("strips", case.id, f"strip{min_strip}"), case), "the frames were meant to produce non-finite flows"


@pytest.mark.parametrize("case", dc.C_CASES, ids=_ids(dc.C_CASES))
def test_stream_pipeline_one_iteration_per_launch(oracle, group_C, case):
    """C.  Streamed: every pair, both levels; iters - 1 accumulating launches behind every tick, for every window."""
    assert _against_the_oracle(oracle, group_C, dc.key("C", case.id), case), "the frames were meant to produce non-finite flows"


@pytest.mark.parametrize("case", dc.D_CASES, ids=_ids(dc.D_CASES))
def test_determinant_guard_with_iterations(oracle, group_D, case):
    """D.  min_det on, against the guarded restatement."""
    _against_the_oracle(oracle, group_D, dc.key("D", case.id), case, min_det=ih.MIN_DET)


@pytest.mark.parametrize("case", dc.E_CASES, ids=_ids(dc.E_CASES))
def test_fast_solve_step_by_step(oracle, group_E, case):
    """E.  lk_float_fast: test_gpu_iter_hard.py's step-by-step check on the child's sessions of 1 .. iters iterations, every window."""
    runs = {j: _pairs(group_E, dc.key("E", case.id, f"iters{j}"), case) for j in range(1, case.iters + 1)}
    if case.kind == "stream":
        for j in runs:
            ticks, acc = (int(group_E[dc.key("E", case.id, f"iters{j}", x)]) for x in ("ticks", "acc"))
            assert ticks > 0 and acc == ticks * (j - 1), f"{case.id} iters {j}: {ticks} ticks, {acc} accumulating launches"
    fast_steps_against_the_oracle(oracle, case, ih.case_frames(case), runs)


@pytest.mark.parametrize("run", dc.DENSE_RUNS, ids=lambda r: dc.dense_key(r).split("/")[1])
def test_run_flow_dense_equals_the_referee(oracle, group_dense, run):
    """dense.  The single-level launches of Session.run_flow_dense (ITER 2, ITER 1) against dense_ref.dense_pair, every level."""
    from test_gpu_dense import _frames

    w, h, levels, win, kind, iters, min_det, max_px = run
    fr = _frames(kind, w, h, win)[:2]
    want = dense_ref.dense_pair(oracle, fr[0], fr[1], levels, win, iters, min_det, max_px)
    for k in range(levels - 1, -1, -1):
        got = group_dense[dc.key(dc.dense_key(run), f"level{k}")]
        assert got.shape == want[k].shape and got.dtype == np.float32
        ok = dense_ref.same_bits(got, want[k])
        assert ok.all(), f"{dc.dense_key(run)} level {k}: {int((~ok).sum())}/{ok.size} differ, first at {np.argwhere(~ok)[:3].tolist()}"


def test_row_windows_of_logical_ranks(oracle, group_rows):
    """rows.  ITER 4 (add + warp on a shard's row window): the ranks' rows put together are the oracle's pair, every level, and no
    rank reports a tap beyond its rows."""
    c = dc.ROWS
    assert group_rows["rows/status"].tolist() == [0] * c["ranks"], [hex(x) for x in group_rows["rows/status"].tolist()]
    frames = dc.rows_frames()
    for p in range(1, len(frames)):
        want = oracle.flow_pair_iter(frames[p - 1], frames[p], c["levels"], c["win"], c["iters"])
        for k in range(c["levels"]):
            got = np.concatenate([group_rows[dc.key("rows", f"rank{r}", f"pair{p}", f"level{k}")] for r in range(c["ranks"])], axis=0)
            assert_same(got, want[k], f"{c['ranks']} ranks: pair {p} level {k}")


# ---- R: the row windows of every window ------------------------------------------------------------------------------------------
_rows_want = {}     # {case id: {pair: the oracle's pyramid}}: shared by R and Rstrips, never written to again


def _oracle_rows(oracle, c, frames):
    if c.id not in _rows_want:
        _rows_want[c.id] = {p: oracle.flow_pair_iter(frames[p - 1], frames[p], c.levels, c.win, c.iters) for p in range(1, len(frames))}
    return _rows_want[c.id]


def _ranks_together(got, prefix, c, n_frames):
    """{pair: flow pyramid} of the ranks' rows under prefix, concatenated; every rank's status word must be 0 (that the ORACLE's
    flows stay inside every rank's rows on these frames: tests/test_iter_hard_ref.py, test_row_window_cases_stay_inside_their_rows)"""
    status = got[dc.key(prefix, "status")].tolist()
    assert status == [0] * c.ranks, f"{prefix}: status {[hex(x) for x in status]}"
    out = {}
    for p in range(1, n_frames):
        out[p] = [np.concatenate([got[dc.key(prefix, f"rank{r}", f"pair{p}", f"level{k}")] for r in range(c.ranks)], axis=0) for k in range(c.levels)]
        for k in range(c.levels):
            assert out[p][k].shape == (c.h >> k, c.w >> k, 2) and out[p][k].dtype == np.float32, f"{prefix}: pair {p} level {k} has shape {out[p][k].shape}"
    return out


@pytest.mark.parametrize("mode", dc.R_MODES)
@pytest.mark.parametrize("c", dc.R_CASES, ids=[c.id for c in dc.R_CASES])
def test_row_windows_of_every_window_deep(oracle, group_R, c, mode):
    """R.  lk_iter_kernel<R, lk_float, FAST, ITER 4 / ITER 1, DMA = true> on the row windows of three logical ranks behind the plain
    WOUT 5 tick.  lk_float: the oracle's three iterations, by the bits.  lk_float_fast: an unsharded lk_float_fast session of the same
    frames run in THIS process, in the plain form, by the bits of the words (the two forms differ in how rows arrive, not in
    arithmetic; the child alone would compare deep with deep)."""
    assert "OFX_ITER_DMA" not in os.environ and "OFX_LK_DMA" not in os.environ, "with OFX_ITER_DMA or OFX_LK_DMA set this process's session would be deep as well"
    frames = li.rows_frames(c)
    got = _ranks_together(group_R, dc.key("R", c.id, mode), c, len(frames))
    if mode == "lk_float":
        want = _oracle_rows(oracle, c, frames)
        for p in got:
            for k in range(c.levels):
                assert_same(got[p][k], want[p][k], f"{c.id} {mode} deep, {c.ranks} ranks: pair {p} level {k}")
        return
    import torch

    if _stop:
        pytest.fail(f"not run: {_stop[0]}")
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cuda_optical_flow_2_amd import engine as eng

    want = _stream(eng, _device_frames(c, frames), c.w, c.h, c.levels, c.win, mode, c.iters, c.B)
    for p in got:
        for k in range(c.levels):
            assert_same(got[p][k].view(np.uint32), want[p][k].view(np.uint32), f"{c.id} {mode}, deep ranks against the plain unsharded session: pair {p} level {k}")


@pytest.mark.parametrize("min_strip", dc.MIN_STRIPS)
@pytest.mark.parametrize("c", dc.R_STRIP_CASES, ids=[c.id for c in dc.R_STRIP_CASES])
def test_row_windows_one_strip_and_strips_of_one_row_deep(oracle, group_Rstrips, c, min_strip):
    """Rstrips.  OFX_LK_MIN_STRIP=1000: a wave marches a rank's whole tile column and refreshes its row table inside a buffer that
    ends within the level; =1: strips of one row, which prime more rows than they take -- next to a buffer's first and last row too."""
    frames = li.rows_frames(c)
    got = _ranks_together(group_Rstrips, dc.key("Rstrips", c.id, f"strip{min_strip}"), c, len(frames))
    want = _oracle_rows(oracle, c, frames)
    for p in got:
        for k in range(c.levels):
            assert_same(got[p][k], want[p][k], f"{c.id} OFX_LK_MIN_STRIP={min_strip}, {c.ranks} ranks: pair {p} level {k}")


# ---- the tick's deep form, in this process ----------------------------------------------------------------------------------------

def _tick_case(win, B):
    """a C case of one iteration: level-1 width one column past a tile"""
    r = win >> 1
    return ih._c(win, (ih.pair_out_w(r) if r <= 4 else ih.tile_out_w(r)) + 1, 1, B)


TICK_CASES = [(_tick_case(win, B), "lk_float") for win in (3, 9, 15, 23) for B in (1, 2)] + [(_tick_case(25, 1), "compat_cpu")]


@pytest.mark.parametrize("case,mode", TICK_CASES, ids=[f"{c.id}-{m}" for c, m in TICK_CASES])
def test_deep_tick_on_hard_frames(oracle, case, mode):
    """stream_kernel<..., DMA = true> through Session(deep_fetch=+1), one iteration (a tick that also writes warped images never
    takes the deep fetch): every pair and level against the oracle's one-iteration pyramid.  OFX_LK_DMA overrides the hint."""
    import torch

    if _stop:
        pytest.fail(f"not run: {_stop[0]}")
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cuda_optical_flow_2_amd import engine as eng

    assert os.environ.get("OFX_LK_DMA") in (None, "1"), "OFX_LK_DMA=0 keeps the tick off the deep fetch whatever the session says"
    frames = ih.case_frames(case)
    got = _stream(eng, _device_frames(case, frames), case.w, case.h, case.levels, case.win, mode, 1, case.B, deep_fetch=1)
    nonfinite = False
    for p in got:
        want = oracle.flow_pair(synth.to_3ch(frames[p - 1]), synth.to_3ch(frames[p]), case.levels, case.win, mode, exact_sums=True)[0]
        nonfinite |= not np.isfinite(want[0]).all()
        for k in range(case.levels):
            assert_same(got[p][k], want[k], f"{case.id} {mode}: pair {p} level {k}")
    assert nonfinite or mode == "compat_cpu", "the frames were meant to produce non-finite flows"


# ---- B last: the shapes likeliest to meet something new ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape", dc.B_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tiny_shapes_pair_at_a_time(oracle, group_B, shape):
    """B.  Images smaller than the window, than a dword, than the two-step lead of the fetch: three iterations on noise."""
    w, h, win = shape
    p, n = dc.b_pair(shape)
    assert_same(group_B[dc.key("B", f"{w}x{h}-win{win}", "level0")], oracle.flow_pair_iter(p, n, 1, win, dc.B_ITERS)[0], f"{w}x{h} win {win}")
