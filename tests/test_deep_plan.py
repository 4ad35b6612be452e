"""The launches of tests/test_gpu_deep_iter.py on the host: every iteration launch its cases make, described to tools/lk_plan_main.cpp
(csrc/lk_plan.h), selects the deep kernel lk_iter_kernel<..., ITER, DMA = true> of the ITER its group is about when OFX_ITER_DMA=1 --
and the plain one without it, so the GPU module's child processes are what reaches the deep form; and under the switch a session
(tools/session_plan_main.cpp, csrc/session_plan.h) has no two-iterations-per-launch form.  The descriptions are derived from the case
lists of tests/deep_child.py, the way csrc/session.cpp and csrc/session_stream.cpp build the launches.

The census: under the switch the launches of all groups together select every one of the 88 instances of the deep family
(lk_instances.iter_family(deep=1): 2 solves x ITER 1..4 x 11 radii) and nothing else -- A the lk_float ITER 3, 2, 1 of every radius, E
the fast ones, R the ITER 4 and ITER 1 of both solves -- so a window that leaves dc.E_CASES or li.T5_CASES fails here, by name.  No GPU."""
import functools
import subprocess

import pytest

import deep_child as dc
import iter_hard as ih
import lk_instances as li
import lk_plan_ref as ref
from test_lk_plan import compile_tool, item, line_of, parse

LK_FLOAT, LK_FLOAT_FAST = 1, 2          # OFX_MODE_* (include/ofx.h)
SET_WARP, ADD_WARP, ADD = (0, 1), (1, 1), (1, 0)   # (accumulate, warp_out) of ITER 3, ITER 2 (ITER 4 on a row window), ITER 1


def pyramid(w, h, levels, pairs=1, k_lo=0):
    """whole levels, per pair the coarsest first (lk_all_levels, iter_passes)"""
    return [item(w >> k, h >> k) for _ in range(pairs) for k in range(levels - 1, k_lo - 1, -1)]


def session_launches(items, iters):
    """ofx_session_run_flow with iters >= 2: iteration 1 sets and warps, the last one only adds"""
    return [(items, SET_WARP, 3)] + [(items, ADD_WARP, 2)] * (iters - 2) + [(items, ADD, 1)]


def case_launches(case, iters=None):
    """[(items, (accumulate, warp_out), the ITER expected)] of a case of tests/iter_hard.py"""
    iters = case.iters if iters is None else iters
    if iters < 2:
        return []                        # (one iteration is the level kernel or the tick alone)
    if case.kind == "pair":
        return session_launches(pyramid(case.w, case.h, case.levels), iters)
    out = []
    for pairs in sorted({case.B, 1}):    # full ticks, and the drained one with a single pair; iteration 1 is the tick's
        items = pyramid(case.w, case.h, case.levels, pairs)
        out += [(items, ADD_WARP, 2)] * (iters - 2) + [(items, ADD, 1)]
    return out


def dense_launches(run):
    """ofx_session_run_flow_dense: the top level as run_flow runs it, below it iters accumulating single-level launches"""
    w, h, levels, win, _, iters, _, _ = run
    out = session_launches(pyramid(w, h, levels, k_lo=levels - 1), iters) if iters >= 2 else []
    for k in range(levels - 2, -1, -1):
        out += [([item(w >> k, h >> k)], ADD_WARP, 2)] * (iters - 1) + [([item(w >> k, h >> k)], ADD, 1)]
    return out


def rank_items(c, pl, pairs):
    """a rank's items: the planes hold its buffer rows (ShardPlan.buf); the rows written shrink from iteration to iteration towards
    its own (which rows exactly does not enter the variant: a row window does)"""
    return [item(c.w >> k, c.h >> k, out=pl.own[k], rows=pl.buf[k], flow_row0=pl.buf[k][0]) for _ in range(pairs) for k in range(c.levels - 1, -1, -1)]


def rows_launches(c):
    """the accumulating launches of every rank of c (an lk_instances.Rows), for full ticks and for the drained tick of one pair:
    ADD_WARP on a row window is ITER 4, the last iteration ITER 1"""
    out = []
    for pl in li.shard_plans(c):
        for pairs in sorted({c.B, 1}, reverse=True):
            items = rank_items(c, pl, pairs)
            assert any(a["row0"] > 0 or a["row_end"] < a["h"] for a in items)
            out += [(items, ADD_WARP, 4)] * (c.iters - 2) + [(items, ADD, 1)]
    return out


@functools.lru_cache(maxsize=None)
def launches():
    """[(group, what, mode, window, items, (accumulate, warp_out), ITER)]"""
    out = []

    def add(group, what, mode, win, ls):
        out.extend((group, what, mode, win, items, aw, it) for items, aw, it in ls)
    for case in dc.A_CASES:
        add("A", case.id, LK_FLOAT, case.win, case_launches(case))
    for case in dc.STRIP_CASES:
        add("strips", case.id, LK_FLOAT, case.win, case_launches(case))
    for w, h, win in dc.B_SHAPES:
        add("B", f"{w}x{h}", LK_FLOAT, win, session_launches(pyramid(w, h, 1), dc.B_ITERS))
    for group, cases in (("C", dc.C_CASES), ("D", dc.D_CASES)):
        for case in cases:
            add(group, case.id, LK_FLOAT, case.win, case_launches(case))
    for case in dc.E_CASES:
        for j in range(1, case.iters + 1):
            add("E", f"{case.id} iters {j}", LK_FLOAT_FAST, case.win, case_launches(case, j))
    for run in dc.DENSE_RUNS:
        add("dense", dc.dense_key(run), LK_FLOAT, run[3], dense_launches(run))
    add("rows", "ranks", LK_FLOAT, dc.ROWS["win"], rows_launches(li.Rows(id="rows", **dc.ROWS)))
    for c in dc.R_CASES:
        for mode in dc.R_MODES:
            add("R", f"{c.id}-{mode}", li.MODE_ID[mode], c.win, rows_launches(c))
    for c in dc.R_STRIP_CASES:
        add("Rstrips", c.id, LK_FLOAT, c.win, rows_launches(c))
    return out


def _line(mode, win, items, aw, dma, **words):
    items = [dict(a, accumulate=aw[0], warp_out=aw[1]) for a in items]
    return line_of("levels", items, dict(ref.ENV, OFX_ITER_DMA=dma), mode=mode, window=win, **words)


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = compile_tool(tmp_path_factory.mktemp("deep_plan"), "lk_plan_main")

    def ask(lines):
        text = subprocess.run([exe], input="".join(l + "\n" for l in lines), text=True, check=True, stdout=subprocess.PIPE).stdout
        return parse(text, len(lines))
    return ask


def test_the_groups_are_about_the_launches_the_issue_names():
    ls = launches()
    iters_of = lambda g: {it for group, *_, it in ls if group == g}
    assert iters_of("A") == iters_of("B") == iters_of("strips") == {3, 2, 1}
    assert {win for group, _, _, win, *_ in ls if group == "A"} == set(range(3, 24, 2))          # all eleven radii
    assert iters_of("C") == {2, 1} and iters_of("rows") == iters_of("R") == iters_of("Rstrips") == {4, 1} and iters_of("E") == {3, 2, 1}
    single = {it for group, _, _, _, items, _, it in ls if group == "dense" and len(items) == 1 and items[0]["w"] in (264, 132, 96, 48, 24)}
    assert single == {2, 1}
    assert {win for group, _, _, win, *_ in ls if group == "E"} == set(range(3, 24, 2))          # all eleven, in lk_float_fast
    assert {mode for group, _, mode, *_ in ls if group == "E"} == {LK_FLOAT_FAST}
    assert {(mode, win) for group, _, mode, win, *_ in ls if group == "R"} == {(m, w) for m in (LK_FLOAT, LK_FLOAT_FAST) for w in range(3, 24, 2)}
    assert {(mode, win) for group, _, mode, win, *_ in ls if group == "Rstrips"} == {(LK_FLOAT, 9), (LK_FLOAT, 23)}


def test_every_launch_selects_the_deep_kernel_under_the_switch_only(tool):
    ls = launches()
    assert len(ls) > 200
    deep = tool([_line(mode, win, items, aw, 1) for _, _, mode, win, items, aw, _ in ls])
    plain = tool([_line(mode, win, items, aw, None) for _, _, mode, win, items, aw, _ in ls])
    for (group, what, mode, win, items, aw, it), d, p in zip(ls, deep, plain):
        where = (group, what, win, aw)
        assert not isinstance(d, ref.Rejected) and not isinstance(p, ref.Rejected), (where, d, p)
        want = dict(family="iter", mode=LK_FLOAT, fast=int(mode == LK_FLOAT_FAST), sums=0, iter=it, deep=1, many=0)
        assert d["variant"] == want, (where, d["variant"])
        assert p["variant"] == dict(want, deep=0), (where, p["variant"])


def _missing(want, got, what):
    """test_lk_instances_plan._missing (that module imports this one)"""
    assert got == want, f"{what}: {len(want - got)} instances without a case: {sorted(want - got)[:12]}; {len(got - want)} unknown: {sorted(got - want)[:12]}"


def test_the_deep_iteration_family_is_reached(tool):
    """The census.  Under iter_dma=1 the launches of all groups select exactly the 88 instances of the deep family, without the switch
    the same lines select the 88 plain ones; and which group holds which instances."""
    ls = launches()
    for dma, deep in ((1, 1), (None, 0)):
        got = tool([_line(mode, win, items, aw, dma) for _, _, mode, win, items, aw, _ in ls])
        for l, g in zip(ls, got):
            assert not isinstance(g, ref.Rejected), (l[:4], g)
            assert g["variant"]["family"] == "iter" and g["variant"]["sums"] == 0 and g["variant"]["many"] == 0, (l[:4], g["variant"])
        by = lambda *names: {(v["mode"], v["fast"], v["iter"], v["deep"], win >> 1) for (group, _, _, win, *_), v in
                             zip(ls, (g["variant"] for g in got)) if not names or group in names}
        _missing(li.iter_family(deep=deep), by(), f"lk_iter_kernel, deep = {deep}")
        radii = set(li.radii("lk_float"))
        assert len(radii) == 11
        _missing({(1, 0, it, deep, r) for it in (3, 2, 1) for r in radii}, by("A"), f"A, deep = {deep}")                       # lk_float ITER 3, 2, 1
        _missing({(1, 1, it, deep, r) for it in (3, 2, 1) for r in radii}, by("E"), f"E, deep = {deep}")                       # the fast ones
        _missing({(1, f, it, deep, r) for f in (0, 1) for it in (4, 1) for r in radii}, by("R"), f"R, deep = {deep}")          # ITER 4 and the ITER 1 behind it
        _missing({(1, 0, it, deep, r) for it in (4, 1) for r in (4, 11)}, by("Rstrips"), f"Rstrips, deep = {deep}")


def test_the_strip_settings_of_the_row_windows(tool):
    """OFX_LK_MIN_STRIP of the group "Rstrips": one strip over the rows a rank's launch writes, and strips of one row; a rank's
    planes end inside the level (a true row window) in every launch"""
    capacity = ref.wave_target(256, 8, *ref.CALL_SITES["levels"], ref.ENV)
    for c in dc.R_STRIP_CASES:
        for items, aw, it in rows_launches(c):
            for ms in dc.MIN_STRIPS:
                t = tool([_line(LK_FLOAT, c.win, items, aw, 1, min_strip=ms, out_w=ih.tile_out_w(c.win >> 1), capacity=capacity)])[0]
                assert (t["variant"]["iter"], t["variant"]["deep"]) == (it, 1)
                assert t["strip_h"] == [a["out_y1"] - a["out_y0"] if ms == 1000 else 1 for a in items], (c.id, ms, t["strip_h"])
                assert min(t["tiles_x"]) == 2, (c.id, t["tiles_x"])


def test_the_strip_settings_give_one_strip_per_column_and_strips_of_one_row(tool):
    """OFX_LK_MIN_STRIP of the group "strips", at the capacity of the device's 256 CUs (4 waves per SIMD, 95 %: lk_plan.h)"""
    capacity = ref.wave_target(256, 8, *ref.CALL_SITES["levels"], ref.ENV)
    for case in dc.STRIP_CASES:
        items, aw, _ = case_launches(case)[0]
        for ms in dc.MIN_STRIPS:
            t = tool([_line(LK_FLOAT, case.win, items, aw, 1, min_strip=ms, out_w=ih.tile_out_w(case.win >> 1), capacity=capacity)])[0]
            assert t["variant"]["deep"] == 1
            assert t["strip_h"] == [a["h"] if ms == 1000 else 1 for a in items], (case.id, ms, t["strip_h"])
            assert min(t["tiles_x"]) == 2, (case.id, t["tiles_x"])         # every level crosses a tile seam


def test_the_lines_of_the_issue(tool):
    base = "launch=levels mode=1 window=9 accumulate=%d warp_out=%d items=241x67"
    for (a, b), it in ((SET_WARP, 3), (ADD_WARP, 2), (ADD, 1)):
        d, p = tool([base % (a, b) + " iter_dma=1", base % (a, b)])
        assert (d["variant"]["family"], d["variant"]["iter"], d["variant"]["deep"]) == ("iter", it, 1)
        assert (p["variant"]["family"], p["variant"]["iter"], p["variant"]["deep"]) == ("iter", it, 0)
    rows, fast = tool(["launch=levels mode=1 window=9 accumulate=1 warp_out=1 items=320x120/30:90@40:80 iter_dma=1",
                       "launch=levels mode=2 window=23 accumulate=1 warp_out=0 items=1x1 iter_dma=1"])
    assert (rows["variant"]["iter"], rows["variant"]["deep"]) == (4, 1)
    assert (fast["variant"]["fast"], fast["variant"]["deep"]) == (1, 1)


def test_the_sessions_of_the_row_windows_are_accepted_under_the_switch(tmp_path):
    """tools/session_plan_main.cpp with iter_dma=1: every sharded session of R (T5_CASES x T5_MODES, every rank) and the unsharded
    one of the same shape are sessions the library accepts, none with the two-iterations-per-launch form.  (That the oracle's flows
    stay inside every rank's rows on these frames, so that a status of 0 is what the reference expects:
    tests/test_iter_hard_ref.py::test_row_window_cases_stay_inside_their_rows, over the same li.T5_CASES.)"""
    assert dc.R_CASES == li.T5_CASES and dc.R_MODES == tuple(li.T5_MODES)       # ... the cases that test is parametrised over
    exe = compile_tool(tmp_path, "session_plan_main")
    base = "width=%d height=%d levels=%d window=%d mode=%d iters=%d stream_batch=%d"
    lines = []
    for c in dc.R_CASES:
        for mode in dc.R_MODES:
            for pl in li.shard_plans(c):
                rows = " ".join("%s=%s" % (n, ",".join(str(x[i]) for x in v)) for n, v, i in (("own_y0", pl.own, 0), ("own_y1", pl.own, 1), ("buf_y0", pl.buf, 0),
                                                                                             ("buf_y1", pl.buf, 1), ("comp_y0", pl.comp, 0), ("comp_y1", pl.comp, 1)))
                lines.append(base % (c.w, c.h, c.levels, c.win, li.MODE_ID[mode], c.iters, c.B) + " sharded=1 local_corner=1 " + rows + " iter_dma=1")
            lines.append(base % (c.w, c.h, c.levels, c.win, li.MODE_ID[mode], c.iters, c.B) + " iter_dma=1")
    text = subprocess.run([exe], input="".join(l + "\n" for l in lines), text=True, check=True, stdout=subprocess.PIPE).stdout
    plans = [l for l in text.splitlines() if l.startswith(("plan ", "error "))]
    assert len(plans) == len(lines) == len(dc.R_CASES) * len(dc.R_MODES) * 4
    for l, p in zip(lines, plans):
        assert p.startswith("plan ") and " iter_pairs=0 " in p + " ", (l, p)


def test_a_session_under_the_switch_has_no_two_iteration_form(tmp_path):
    """... also where it would have one without it (windows up to 9x9, three iterations and more): acc == ticks * (iters - 1) in the
    GPU module is what such a session shows"""
    exe = compile_tool(tmp_path, "session_plan_main")
    cases = [c for c in dc.C_CASES + dc.D_CASES + dc.E_CASES if c.kind == "stream"]
    sessions = sorted({(c.w, c.h, c.levels, c.win, j, c.B, LK_FLOAT_FAST if c in dc.E_CASES else LK_FLOAT)
                       for c in cases for j in (range(1, c.iters + 1) if c in dc.E_CASES else [c.iters])})
    words = ["width=%d height=%d levels=%d window=%d iters=%d stream_batch=%d mode=%d" % s for s in sessions]
    text = subprocess.run([exe], input="".join(w + " iter_dma=1\n" for w in words) + "".join(w + "\n" for w in words), text=True, check=True,
                          stdout=subprocess.PIPE).stdout
    pairs = [int(l.split("iter_pairs=")[1].split()[0]) for l in text.splitlines() if l.startswith("plan ")]
    assert len(pairs) == 2 * len(sessions)
    assert pairs[:len(sessions)] == [0] * len(sessions)
    assert pairs[len(sessions):] == [int(win <= 9 and iters >= 3) for _, _, _, win, iters, _, _ in sessions] and any(pairs[len(sessions):])
