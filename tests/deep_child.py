"""The iteration launches in their deep-fetch form (lk_iter_kernel<..., DMA = true>, csrc/lk_body_buf.h) at small shapes: the child
process of tests/test_gpu_deep_iter.py.  Not a test module and not a conftest.

    OFX_ITER_DMA=1 python tests/deep_child.py OUT.npz GROUP

OFX_ITER_DMA is read once per process, at the first LK launch (csrc/lk_level.hip, lk_switches), so the deep form is reached at small
shapes only by a process that was STARTED with it.  This one refuses to start otherwise, runs the cases of GROUP on the GPU, stores
every flow array under a readable key in OUT.npz and prints "deep ok".  Together the groups reach all 88 instances of the deep
family (A: lk_float ITER 3, 2, 1; E: the fast ones; R: ITER 4 and the ITER 1 behind it, both solves; every radius each).  It compares nothing and calls no oracle: the parent does,
on the CPU.  The first exception ends it with a non-zero status.

The case lists below are read by the parent and by tests/test_deep_plan.py (which shows on the host that the launches they make
select the deep kernels); importing this module needs neither a GPU nor torch."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import iter_hard as ih   # noqa: E402
import lk_instances as li   # noqa: E402

_P9 = ih.pair_out_w(4)
_ALL = {c.id: c for c in ih.A_CASES + ih.C_CASES + ih.D_CASES}

# A: every window pair at a time, 3 iterations: ITER 3 (set + warp), ITER 2 (add + warp), ITER 1 (add) of every radius
A_CASES = list(ih.A_CASES)
# strips: one strip per tile column (the row table is refreshed once at 67 rows, twice at 132, by the deep branch's own rule) and
# strips of one row (the rows the last step issued are never taken).  OFX_LK_MIN_STRIP is read at every launch.
STRIP_CASES = [_ALL[i] for i in ("A-win3", "A-win9", "A2-win11", "A2-win23")]
MIN_STRIPS = (1000, 1)
# B: images smaller than the window, than a dword, than the two-step lead of the fetch
B_SHAPES = list(ih.B_SHAPES)
B_ITERS = 3
# C: streamed.  Under the switch a session has no two-iterations-per-launch form (session_plan.h, want_pairs): iterations 2 .. iters
# are ITER 2 launches and one ITER 1 launch over all levels of the tick's pairs, also for the windows up to 9x9.
C_CASES = [_ALL[i] for i in (f"C-win9-w{_P9 + 1}-it5-B2", f"C-win3-w{ih.pair_out_w(1) + 1}-it5-B1", f"C-win5-w{ih.pair_out_w(2) + 1}-it4-B2",
                             f"C-win11-w{ih.tile_out_w(5) + 1}-it4-B1", f"C-win15-w{ih.tile_out_w(7) + 1}-it5-B2")]
# D: the determinant guard (ih.MIN_DET)
D_CASES = [_ALL[i] for i in ("A-win9", "A-win15", f"C-win9-w{_P9 + 1}-it5-B2", "D-3level")]
# E: lk_float_fast, sessions of 1 .. iters iterations (test_fast_solve_step_by_step): every window pair at a time -- the fast ITER 3,
# 2 and 1 of every radius -- and one streamed case
E_CASES = [c for c in ih.E_CASES if c.kind == "pair"] + [_ALL[f"C-win5-w{ih.pair_out_w(2) + 1}-it4-B2"]]
# dense: Session.run_flow_dense, whose levels below the top are single-level launches: ITER 2 (add + warp), then ITER 1
# (w, h, levels, window, frames of test_gpu_dense._frames, iters, min_det, max_px)
DENSE_RUNS = [(264, 80, 3, 9, kind, iters, min_det, max_px) for kind in ("hard", "smooth") for iters in (1, 3) for min_det in (0.0, 1.0)
              for max_px in (0.0, 9.0)] + [(96, 64, 4, 13, "hard", 2, 0.0, 0.0), (96, 64, 4, 13, "smooth", 2, 1.0, 13.0)]
# rows: ITER 4 (add + warp on a shard's row window): the smallest configuration of
# test_sharded_streamed_iterations_equal_the_unsharded_path, logical ranks on one device.  Smooth frames: the huge flows of the hard
# ones leave a shard's rows and rightly set the status word.
ROWS = dict(w=640, h=480, levels=3, win=9, iters=3, ranks=3, B=2, warp_margin=8)
# R: row windows of every window, both solves: the cases of tests/test_gpu_lk_instances.py's T5 (three logical ranks, cuts at least
# R + 2 rows deep at both levels, three iterations).  Under the switch the tick (WOUT 5) stays plain; the ITER 4 and ITER 1 launches
# behind it are deep.
R_CASES = list(li.T5_CASES)
R_MODES = tuple(li.T5_MODES)
# Rstrips: a row window under the strip settings of "strips": one strip per tile column (the row table refreshed on a buffer that
# ends inside the level) and strips of one row
R_STRIP_CASES = [c for c in R_CASES if c.win in (9, 23)]

GROUPS = ("A", "strips", "B", "C", "D", "E", "dense", "rows", "R", "Rstrips")


def key(*parts):
    return "/".join(str(p) for p in parts)


def dense_key(run):
    w, h, levels, win, kind, iters, min_det, max_px = run
    return key("dense", f"{w}x{h}-L{levels}-win{win}-{kind}-it{iters}-det{min_det:g}-max{max_px:g}")


def rows_frames():
    """the frames of the sharded test (host arrays)"""
    from cuda_optical_flow_2_amd import synth

    c = ROWS
    return [synth.smooth_pair(c["w"], c["h"], 1.1 * i, 0.6 * i, seed=29)[1] for i in range(2 * c["B"] + 2)]


def b_pair(shape):
    from cuda_optical_flow_2_amd import synth

    w, h, win = shape
    return synth.random_pair(w, h, seed=w + win)


# ---- the runs (GPU) ---------------------------------------------------------------------------------------------------------------

def _put(out, prefix, got):
    """{pair: flow pyramid} under prefix/pairP/levelK"""
    for p, pyr in got.items():
        for k, f in enumerate(pyr):
            out[key(prefix, f"pair{p}", f"level{k}")] = np.ascontiguousarray(f)


def _run(eng, out, prefix, case, mode="lk_float", iters=None, min_det=0.0):
    """a case through the path it names, the way tests/test_gpu_iter_hard.py::_run does it; a streamed one also records its ticks
    and the accumulating launches behind them"""
    from test_gpu_iter_hard import _device_frames
    from test_gpu_iteration_pairs import _stream

    iters = case.iters if iters is None else iters
    frames = ih.case_frames(case)
    if case.kind == "pair":
        _put(out, prefix, {1: eng.flow_pair(frames[0], frames[1], case.levels, case.win, mode, iters=iters, min_det=min_det)})
        return
    os.environ["OFX_ITER_PAIRS"] = "1"       # (the session must drop the two-iteration form because of the switch, not for want of asking)
    n = {}
    _put(out, prefix, _stream(eng, _device_frames(case, frames), case.w, case.h, case.levels, case.win, mode, iters, case.B, launches=n, min_det=min_det))
    out[key(prefix, "ticks")], out[key(prefix, "acc")] = np.int64(n["ticks"]), np.int64(n["acc"])


def run_A(eng, out):
    for case in A_CASES:
        _run(eng, out, key("A", case.id), case)


def run_strips(eng, out):
    try:
        for case in STRIP_CASES:
            for ms in MIN_STRIPS:
                os.environ["OFX_LK_MIN_STRIP"] = str(ms)
                _run(eng, out, key("strips", case.id, f"strip{ms}"), case)
    finally:
        os.environ.pop("OFX_LK_MIN_STRIP", None)


def run_B(eng, out):
    for shape in B_SHAPES:
        w, h, win = shape
        p, n = b_pair(shape)
        out[key("B", f"{w}x{h}-win{win}", "level0")] = eng.flow_pair(p, n, 1, win, "lk_float", iters=B_ITERS)[0]


def run_C(eng, out):
    for case in C_CASES:
        _run(eng, out, key("C", case.id), case)


def run_D(eng, out):
    for case in D_CASES:
        _run(eng, out, key("D", case.id), case, min_det=ih.MIN_DET)


def run_E(eng, out):
    for case in E_CASES:
        for j in range(1, case.iters + 1):
            _run(eng, out, key("E", case.id, f"iters{j}"), case, "lk_float_fast", iters=j)


def run_dense(eng, out):
    from test_gpu_dense import _dense_session, _frames

    for run in DENSE_RUNS:
        w, h, levels, win, kind, iters, min_det, max_px = run
        got = _dense_session(eng, _frames(kind, w, h, win)[:2], levels, win, iters, min_det, max_px)[0]
        for k in range(levels):
            out[key(dense_key(run), f"level{k}")] = got[k]


def _rank_rows(eng, out, prefix, c, mode, frames):
    """the logical ranks of c (an lk_instances.Rows) on one device, the way tests/test_gpu_lk_instances.py::_ranks runs them: every
    rank's rows of every pair and level under prefix/rankR/pairP/levelK, the ranks' status words under prefix/status"""
    import torch

    L, B = c.levels, c.B
    ranks = [eng.Session(c.w, c.h, L, c.win, mode, shard=pl, local_corner=True, stream_batch=B, iters=c.iters, strict=False) for pl in li.shard_plans(c)]
    seen = 0
    for s in ranks:
        s.stream_begin()

    def snap(done):
        nonlocal seen
        if done >= 1:
            for p in range(max(seen + 1, done - B + 1), done + 1):
                for r, s in enumerate(ranks):
                    for k in range(L):
                        out[key(prefix, f"rank{r}", f"pair{p}", f"level{k}")] = s.flow_of(p, k)[0].cpu().numpy()
            seen = done
    for f in frames:
        snap([s.stream_submit(f) for s in ranks][0])
    while True:
        d = [s.stream_drain() for s in ranks][0]
        if d == -2:
            break
        snap(d)
    torch.cuda.synchronize()
    out[key(prefix, "status")] = np.array([s.corner_status() for s in ranks], np.int64)
    for s in ranks:
        s.close()
    assert seen == len(frames) - 1, f"{prefix}: {seen} pairs of {len(frames) - 1} came out"


def run_rows(eng, out):
    import torch

    _rank_rows(eng, out, "rows", li.Rows(id="rows", **ROWS), "lk_float", [torch.from_numpy(f).cuda() for f in rows_frames()])


def run_R(eng, out):
    from test_gpu_iter_hard import _device_frames

    for c in R_CASES:
        frames = _device_frames(c, li.rows_frames(c))
        for mode in R_MODES:
            _rank_rows(eng, out, key("R", c.id, mode), c, mode, frames)


def run_Rstrips(eng, out):
    from test_gpu_iter_hard import _device_frames

    try:
        for c in R_STRIP_CASES:
            frames = _device_frames(c, li.rows_frames(c))
            for ms in MIN_STRIPS:
                os.environ["OFX_LK_MIN_STRIP"] = str(ms)
                _rank_rows(eng, out, key("Rstrips", c.id, f"strip{ms}"), c, "lk_float", frames)
    finally:
        os.environ.pop("OFX_LK_MIN_STRIP", None)


def main(argv):
    if len(argv) != 3 or argv[2] not in GROUPS:
        sys.exit(f"usage: OFX_ITER_DMA=1 python {argv[0]} OUT.npz {'|'.join(GROUPS)}")
    if os.environ.get("OFX_ITER_DMA") != "1" or "OFX_LK_DMA" in os.environ:
        sys.exit("deep_child: start me with OFX_ITER_DMA=1 and without OFX_LK_DMA (both are read once per process)")
    import torch

    assert torch.cuda.is_available(), "these runs need the MI355X"
    from cuda_optical_flow_2_amd import engine

    out = {}
    globals()["run_" + argv[2]](engine, out)
    np.savez(argv[1], **out)
    print("deep ok")


if __name__ == "__main__":
    main(sys.argv)
