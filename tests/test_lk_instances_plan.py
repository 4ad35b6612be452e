"""The census of tests/lk_instances.py on the host: every tick and every launch its cases make, described to tools/lk_plan_main.cpp
(csrc/lk_plan.h), selects a kernel instance; together they select EVERY instance of the stream family (112), of the level kernel
(57) and of the plain iteration launches (88), as the lk_inst_*.hip units and lk_inst.h define them.  A new family, a new radius or
a hint that is no longer read leaves an instance without a case and fails here, naming it.  The descriptions are built the way
csrc/session_stream.cpp and csrc/session.cpp build the launches (tests/test_deep_plan.py).  No GPU."""
import functools
import glob
import os
import re
import subprocess

import pytest

import iter_hard as ih
import lk_instances as li
import lk_plan_ref as ref
from test_deep_plan import ADD, ADD_WARP, case_launches, rank_items
from test_lk_plan import ROOT, compile_tool, item, line_of, parse

CSRC = os.path.join(ROOT, "cuda_optical_flow_2_amd", "csrc")


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = compile_tool(tmp_path_factory.mktemp("lk_instances_plan"), "lk_plan_main")

    def ask(lines):
        text = subprocess.run([exe], input="".join(l + "\n" for l in lines), text=True, check=True, stdout=subprocess.PIPE).stdout
        got = parse(text, len(lines))
        for l, g in zip(lines, got):
            assert not isinstance(g, ref.Rejected), (l, g)
        return [g["variant"] for g in got]
    return ask


# ---- the descriptions -----------------------------------------------------------------------------------------------------------
def tick_pairs(B):
    """the pairs a tick's LK stage carries in a stream of 2 B + 1 frames: B, and one in the drain (and before the first full tick)"""
    return sorted({B, 1}, reverse=True)


def tick_line(c, mode, warp_out, hint, pairs):
    return "launch=tick mode=%d window=%d warp_out=%d hint=%d pyramid=%dx%d:%d:%d" % (li.MODE_ID[mode], c.win, warp_out, hint, c.w, c.h, c.levels, pairs)


def with_flags(items, aw):
    return [dict(a, accumulate=aw[0], warp_out=aw[1]) for a in items]


@functools.lru_cache(maxsize=None)
def ticks():
    """[(list, what, radius, pairs, line)] of T0, T3 and T5"""
    out = []
    for t in li.T0_CASES:
        out += [("T0", t.id, t.case.win >> 1, n, tick_line(t.case, t.mode, 0, t.deep, n)) for n in tick_pairs(t.case.B)]
    for c in li.T3_CASES:
        for mode in li.T3_MODES:
            out += [("T3", f"{c.id}-{mode}", c.win >> 1, n, tick_line(c, mode, 1, 0, n)) for n in tick_pairs(c.B)]
    for c in li.T5_CASES:
        for mode in li.T5_MODES:
            for pl in li.shard_plans(c):
                for n in tick_pairs(c.B):
                    items = with_flags(rank_items(c, pl, n), (0, 1))
                    out.append(("T5", f"{c.id}-{mode}-rank{pl.rank}", c.win >> 1, n, line_of("tick", items, ref.ENV, mode=li.MODE_ID[mode], window=c.win, hint=0)))
    return out


@functools.lru_cache(maxsize=None)
def launches():
    """[(list, what, radius, line)] of the ofx_lk_levels launches: L; behind T3 and T5; ih.A_CASES and the fast E"""
    out = []

    def add(name, what, mode, win, ls):
        out.extend((name, what, win >> 1, line_of("levels", with_flags(items, aw), ref.ENV, mode=li.MODE_ID[mode], window=win)) for items, aw, _ in ls)
    for c in li.L_CASES:
        out.append(("L", c.id, c.win >> 1, line_of("levels", [item(c.w, c.h)], ref.ENV, mode=li.MODE_ID[c.mode], window=c.win, sums=int(c.sums))))
    for c in li.T3_CASES:
        for mode in li.T3_MODES:
            add("T3", c.id, mode, c.win, case_launches(c))
    for c in li.T5_CASES:
        for mode in li.T5_MODES:
            for pl in li.shard_plans(c):
                for n in tick_pairs(c.B):
                    add("T5", f"{c.id}-rank{pl.rank}", mode, c.win, [(rank_items(c, pl, n), ADD_WARP, 4)] * (c.iters - 2) + [(rank_items(c, pl, n), ADD, 1)])
    for c in ih.A_CASES:
        add("A", c.id, "lk_float", c.win, case_launches(c))
    for c in ih.E_CASES:
        if c.kind == "pair":
            for j in range(1, c.iters + 1):
                add("E", f"{c.id} iters {j}", "lk_float_fast", c.win, case_launches(c, j))
    return out


def _missing(want, got, what):
    assert got == want, f"{what}: {len(want - got)} instances without a case: {sorted(want - got)[:12]}; {len(got - want)} unknown: {sorted(got - want)[:12]}"


# ---- the census -----------------------------------------------------------------------------------------------------------------
def test_the_families_are_the_ones_the_sets_are_written_for():
    """seven units instantiate ofx_launch::stream, three ofx_launch::levels and eight ofx_launch::iter: a new family cannot appear
    without the products of lk_instances.py -- and with them a case list -- being extended"""
    lines = [l for f in sorted(glob.glob(os.path.join(CSRC, "*"))) if os.path.isfile(f) for l in open(f, errors="replace") if l.startswith("template int ofx_launch::")]
    count = lambda name: sum(1 for l in lines if re.match(r"template int ofx_launch::%s<" % name, l))
    assert (count("stream"), count("levels"), count("iter")) == (7, 3, 8), [l.split("(")[0] for l in lines]
    assert len(lines) == 7 + 3 + 8 + 4                           # ... and iter_pair's four (two iterations per launch: its own census)
    with open(os.path.join(CSRC, "lk_plan.h")) as f:
        assert "lk_max_radius(int mode) { return mode == OFX_MODE_COMPAT_CPU ? 12 : 11; }" in f.read()


def test_the_stream_family_is_reached(tool):
    ts = ticks()
    got = tool([t[-1] for t in ts])
    seen = set()
    for (name, what, r, pairs, _), v in zip(ts, got):
        assert v["family"] == "stream", (what, v)
        assert v["many"] == int(pairs >= 2), (what, pairs, v)       # two pairs and more: the other wave plan; the drained tick: one
        want_wout = {"T0": li.WOUT_SET, "T3": li.WOUT_WARP, "T5": li.WOUT_ROWS}[name]
        assert v["iter"] == want_wout, (what, v)
        seen.add((v["mode"], v["fast"], v["iter"], v["deep"], r))
    _missing(li.stream_family(), seen, "stream_kernel")
    # both wave plans in every list, in both fetch forms of T0
    for name in ("T0", "T3", "T5"):
        assert {(v["many"], v["deep"]) for t, v in zip(ts, got) if t[0] == name} == ({(0, 0), (1, 0), (0, 1), (1, 1)} if name == "T0" else {(0, 0), (1, 0)}), name


def test_the_tick_reads_the_hint_of_every_t0_case(tool):
    """Session(deep_fetch=+1 / -1) is what selects the deep / the plain tick at these sizes (no level has 16 Mpx)"""
    ts = [t for t in ticks() if t[0] == "T0"]
    for t, v in zip(ts, tool([t[-1] for t in ts])):
        assert v["deep"] == int("hint=1" in t[-1].split()), (t[1], v)


def test_the_levels_family_is_reached(tool):
    ls = [l for l in launches() if l[0] == "L"]
    got = tool([l[-1] for l in ls])
    assert all(v["family"] == "levels" for v in got)
    _missing(li.levels_family(), {(v["mode"], v["fast"], v["sums"], r) for (_, _, r, _), v in zip(ls, got)}, "lk_level_kernel")


def test_the_plain_iteration_family_is_reached(tool):
    ls = [l for l in launches() if l[0] != "L"]
    got = tool([l[-1] for l in ls])
    assert all(v["family"] == "iter" and v["deep"] == 0 and v["sums"] == 0 for v in got)
    by = lambda *names: {(v["mode"], v["fast"], v["iter"], v["deep"], r) for (name, _, r, _), v in zip(ls, got) if name in names}
    _missing(li.iter_family(), by("T3", "T5", "A", "E"), "lk_iter_kernel")
    radii = set(li.radii("lk_float"))
    assert by("A") == {(1, 0, it, 0, r) for it in (3, 2, 1) for r in radii}           # lk_float ITER 3, 2, 1: ih.A_CASES
    assert by("E") == {(1, 1, it, 0, r) for it in (3, 2, 1) for r in radii}           # the fast ones: the extended E
    assert by("T5") == {(1, f, it, 0, r) for f in (0, 1) for it in (4, 1) for r in radii}   # ITER 4 and the ITER 1 behind it
    assert by("T3") == {(1, f, 1, 0, r) for f in (0, 1) for r in radii}              # two iterations: the tick and one ITER 1 launch


def test_every_rank_of_t5_has_a_true_row_window():
    """... at both levels, cut at least R + 2 rows deep, in a shape the rule of lk_instances.cuts_deep_enough calls its smallest"""
    for c in li.T5_CASES:
        assert c.h % 4 == 0 and li.cuts_deep_enough(c) and not li.cuts_deep_enough(c._replace(h=c.h - 4)), c.id
        for pl in li.shard_plans(c):
            items = rank_items(c, pl, 1)
            assert all(a["row0"] > 0 or a["row_end"] < a["h"] for a in items), (c.id, pl.rank, items)
            assert all(a["row0"] == 0 or a["row0"] >= (c.win >> 1) + 2 for a in items) and all(a["row_end"] == a["h"] or a["h"] - a["row_end"] >= (c.win >> 1) + 2 for a in items)
        assert c.w == 2 * (ih.tile_out_w(c.win >> 1) + 1) and c.w <= 498 and c.h <= 392


def test_every_session_of_the_lists_is_one_the_library_accepts(tmp_path):
    """tools/session_plan_main.cpp (csrc/session_plan.h, what ofx_session_create checks): no case is refused -- T5's heights are
    the rule's, none had to move on -- and the sessions of two iterations have no two-per-launch form (acc == ticks on the GPU)"""
    exe = compile_tool(tmp_path, "session_plan_main")
    lines, two = [], []
    base = "width=%d height=%d levels=%d window=%d mode=%d iters=%d stream_batch=%d"
    for t in li.T0_CASES:
        c = t.case
        lines.append(base % (c.w, c.h, c.levels, c.win, li.MODE_ID[t.mode], 1, c.B) + " deep_fetch=%d" % t.deep)
    for c in li.T3_CASES:
        for mode in li.T3_MODES:
            for j in (1, 2):
                two.append(len(lines))
                lines.append(base % (c.w, c.h, c.levels, c.win, li.MODE_ID[mode], j, c.B))
    for c in li.T5_CASES:
        for mode in li.T5_MODES:
            for pl in li.shard_plans(c):
                rows = " ".join("%s=%s" % (n, ",".join(str(x[i]) for x in v)) for n, v, i in (("own_y0", pl.own, 0), ("own_y1", pl.own, 1), ("buf_y0", pl.buf, 0),
                                                                                             ("buf_y1", pl.buf, 1), ("comp_y0", pl.comp, 0), ("comp_y1", pl.comp, 1)))
                lines.append(base % (c.w, c.h, c.levels, c.win, li.MODE_ID[mode], c.iters, c.B) + " sharded=1 local_corner=1 " + rows)
            lines.append(base % (c.w, c.h, c.levels, c.win, li.MODE_ID[mode], c.iters, c.B))      # the unsharded session lk_float_fast is compared with
    text = subprocess.run([exe], input="".join(l + "\n" for l in lines), text=True, check=True, stdout=subprocess.PIPE).stdout
    plans = [l for l in text.splitlines() if l.startswith(("plan ", "error "))]
    assert len(plans) == len(lines)
    for l, p in zip(lines, plans):
        assert p.startswith("plan "), (l, p)
    assert all(" iter_pairs=0 " in plans[i] for i in two)
