"""The schedule of the refinement iterations (csrc/iter_plan.h) on the host: tools/iter_plan_main.cpp is built with the host compiler
and its plans are checked, for every iteration count a session takes and every kind of session, against the rules of the schedule and
against the two loops that used to hold it -- the stream tick's and the pair-at-a-time path's -- transcribed below.  No GPU.

tests/test_gpu_iter_schedule.py counts the launches of real sessions against the same transcription."""
import os
import shutil
import subprocess
from collections import namedtuple

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Pass = namedtuple("Pass", "it count shift warp wout win wo fin fout")
KINDS = [(0, 0), (1, 0), (1, 1)]   # (fused, pairs): pairs implies fused
ITERS = range(2, 65)


def stream_loop(iters, fused, pairs):
    """The loop behind a stream tick as it stood before the schedule became an object (loop-carried alt / wcur / two / wout / wi / wo):
    the launches after iteration 1.  The warped planes itsh[b][1] / [2] are planes 0 / 1 here."""
    out = []
    alt = bool(pairs) and bool(((iters - 1) // 2) & 1)   # the flow is in flowset2: also where the tick's LK stage started
    wcur = 1
    it = 1
    while it < iters:
        two = bool(pairs) and it + 2 <= iters
        need_warp = not fused
        wout = bool(fused) and it + (2 if two else 1) < iters
        wi = wcur if fused else 1
        wo = 3 - wi
        shift = it == 1 and not fused
        fcur, fother = (1, 0) if alt else (0, 1)
        out.append(Pass(it, 2 if two else 1, shift, need_warp, wout, wi - 1, wo - 1, fcur, fother if two else fcur))
        if two:
            alt = not alt
        wcur = wo
        it += 2 if two else 1
    return out


def pair_loop(iters, fused):
    """The loop of the pair-at-a-time path as it stood (wbuf[(it - 1) & 1] / wbuf[it & 1]; unfused: sh[1], which is wbuf[0]): one
    iteration per launch, in place in the session's flow.  Its shift launch precedes iteration 1, so no pass has one; wo counts
    only where wout holds."""
    out = []
    for it in range(1, iters):
        need_warp, wout = not fused, bool(fused) and it + 1 < iters
        out.append(Pass(it, 1, None, need_warp, wout, (it - 1) & 1 if fused else 0, it & 1, 0, 0))
    return out


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("iter_plan") / "iter_plan_main")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "cuda_optical_flow_2_amd", "csrc"),
                           os.path.join(ROOT, "tools", "iter_plan_main.cpp"), "-o", exe])

    def run(iters, fused, pairs):
        lines = subprocess.check_output([exe, str(iters), str(fused), str(pairs)], text=True).split("\n")
        head = lines[0].split()
        assert head[0] == "plan"
        plan = []
        for l in lines[1:]:
            if l:
                v = list(map(int, l.split()))
                plan.append(Pass(v[0], v[1], bool(v[2]), bool(v[3]), bool(v[4]), *v[5:]))
        assert int(head[1]) == len(plan)
        return plan
    return run


@pytest.fixture(scope="module")
def plans(planner):
    return {(iters, fused, pairs): planner(iters, fused, pairs) for iters in ITERS for fused, pairs in KINDS}


def test_passes_cover_the_iterations(plans):
    for (iters, fused, pairs), plan in plans.items():
        what = f"iters {iters} fused {fused} pairs {pairs}"
        assert 1 <= len(plan) <= 63, what
        assert sum(q.count for q in plan) == iters - 1, what
        done = 1
        for q in plan:
            assert q.it == done and q.count in (1, 2), what
            done += q.count
        singles = [i for i, q in enumerate(plan) if q.count == 1]
        if pairs:   # paired from the front; a left-over one is last
            assert singles in ([], [len(plan) - 1]), what
        else:
            assert len(singles) == len(plan), what


def test_flow_sets_chain_and_end_in_set_0(plans):
    for (iters, fused, pairs), plan in plans.items():
        what = f"iters {iters} fused {fused} pairs {pairs}"
        assert plan[-1].fout == 0, what
        assert all(b.fin == a.fout for a, b in zip(plan, plan[1:])), what
        assert all(q.fin in (0, 1) and q.fout in (0, 1) and (q.fin != q.fout) == (q.count == 2) for q in plan), what


def test_warped_planes(plans):
    for (iters, fused, pairs), plan in plans.items():
        what = f"iters {iters} fused {fused} pairs {pairs}"
        assert all(q.win in (0, 1) and q.wo in (0, 1) for q in plan), what
        if fused:
            assert plan[0].win == 0, what   # the plane iteration 1 wrote
            assert all(b.win == a.wo for a, b in zip(plan, plan[1:])), what
            assert all(q.wo != q.win for q in plan if q.wout), what   # (a launch never writes the plane it reads)
            assert [q.wout for q in plan] == [True] * (len(plan) - 1) + [False], what
            assert not any(q.shift or q.warp for q in plan), what
        else:
            assert all(q.win == 0 and q.warp and not q.wout for q in plan), what
            assert [q.shift for q in plan] == [True] + [False] * (len(plan) - 1), what


def test_plan_equals_the_loops_it_replaces(plans):
    for (iters, fused, pairs), plan in plans.items():
        what = f"iters {iters} fused {fused} pairs {pairs}"
        assert plan == stream_loop(iters, fused, pairs), what
        if not pairs:   # (the pair-at-a-time path runs one iteration per launch in every session)
            want = pair_loop(iters, fused)
            assert len(plan) == len(want), what
            for q, r in zip(plan, want):
                assert q._replace(shift=None, wo=q.wo if q.wout else None) == r._replace(wo=r.wo if r.wout else None), what


@pytest.mark.parametrize("iters", [0, 1])
def test_no_iterations_no_passes(planner, iters):
    assert all(planner(iters, fused, pairs) == [] for fused, pairs in KINDS)
