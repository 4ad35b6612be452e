"""The planner of the fused two-iteration launch (csrc/pair_plan.h) on the host: tools/pair_plan_main.cpp is built with the host
compiler and its plans are checked -- every row of every tile column of every item exactly once, no sliver, at most two segments
per wave, no more waves than slots, and S the steps of the longest wave.  No GPU."""
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_SEGS = 2
MIN_H = 8


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("pair_plan") / "pair_plan_main")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "cuda_optical_flow_2_amd", "csrc"),
                           os.path.join(ROOT, "tools", "pair_plan_main.cpp"), "-o", exe])

    def run(out_w, overhead, capacity, items, min_h=MIN_H):
        args = [exe, str(out_w), str(overhead), str(min_h), str(capacity)] + [str(v) for it in items for v in it]
        lines = subprocess.check_output(args, text=True).split("\n")
        if lines[0] == "none":
            return None
        head = lines[0].split()
        assert head[0] == "plan"
        segs = [tuple(map(int, l.split())) for l in lines[1:] if l]
        return int(head[1]), int(head[2]), int(head[3]), segs
    return run


def pyramid(w, h, levels, pairs):
    """the items of a tick: per pair, the coarsest level first (session_stream.cpp)"""
    return [(w >> k, h >> k) for _ in range(pairs) for k in range(levels - 1, -1, -1)]


def check(plan, out_w, overhead, capacity, items, min_h=MIN_H):
    assert plan is not None, "no plan"
    waves, nsegs, S, segs = plan
    assert waves <= capacity and nsegs == len(segs)
    per_wave, cost, rows = {}, {}, {}
    for wv, item, tile, y0, y1 in segs:
        w, h = items[item]
        assert 0 <= wv < waves and 0 <= tile < -(-w // out_w) and 0 <= y0 < y1 <= h
        assert y1 - y0 >= min_h or (y0 == 0 and y1 == h), f"sliver {y0}..{y1} of {h}"
        per_wave[wv] = per_wave.get(wv, 0) + 1
        cost[wv] = cost.get(wv, 0) + (y1 - y0) + overhead
        rows.setdefault((item, tile), []).append((y0, y1))
    assert sorted(per_wave) == list(range(waves)), "an empty wave"
    assert max(per_wave.values()) <= MAX_SEGS
    assert S == max(cost.values())
    assert sorted(rows) == [(i, t) for i, (w, _) in enumerate(items) for t in range(-(-w // out_w))]
    for (item, _), spans in rows.items():   # exactly once: the spans of a column tile [0, h)
        spans.sort()
        assert spans[0][0] == 0 and spans[-1][1] == items[item][1]
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    return S


def test_4k_flagship_plan(planner):
    """4K, 5 levels, 9x9, 8 pairs in 2 048 slots.  One strip per wave marches 216 + 16 = 232 steps (plan_table_g).  On 232-column
    tiles a pair has 17 + 9 + 5 + 3 + 2 columns; were no column cut, 2 048 waves would need ceil(sum(rows + 16) / 2 048) = 199 steps,
    and every cut adds a segment's 16.  The plan may not need more than 216, the strip height of today's plan WITHOUT its 16 steps."""
    items = pyramid(3840, 2160, 5, 8)
    cols = sum(-(-w // 232) * (h + 16) for w, h in items)
    assert -(-cols // 2048) == 199
    S = check(planner(232, 16, 2048, items), 232, 16, 2048, items)
    assert 199 <= S <= 216
    S224 = check(planner(224, 16, 2048, items), 224, 16, 2048, items)   # packing alone, on the old tile
    assert S < S224 < 232


def test_1080p_plan(planner):
    """1080p, 4 levels, 7x7 (240-column tiles, 13 steps per segment), 16 pairs: one strip per wave marches 106 steps."""
    items = pyramid(1920, 1080, 4, 16)
    S = check(planner(240, 13, 2048, items), 240, 13, 2048, items)
    assert S <= 106


@pytest.mark.parametrize("size,pairs,out_w,overhead,capacity", [
    ((300, 200, 3), 2, 232, 16, 5), ((300, 200, 3), 2, 232, 16, 7), ((300, 200, 3), 1, 232, 16, 3), ((300, 200, 3), 2, 240, 13, 5),
    ((300, 200, 3), 2, 248, 7, 5), ((464, 20, 3), 2, 232, 16, 2048), ((464, 44, 3), 1, 232, 16, 2048), ((474, 40, 2), 1, 232, 16, 2048),
    ((926, 40, 2), 1, 232, 16, 2048), ((496, 40, 2), 2, 248, 7, 2048),
])
def test_tiny_plans(planner, size, pairs, out_w, overhead, capacity):
    items = pyramid(*size, pairs)
    check(planner(out_w, overhead, capacity, items), out_w, overhead, capacity, items)


def test_too_few_waves_have_no_plan(planner):
    """8 tile columns do not go into 3 waves of two segments: the launch then keeps one strip per wave"""
    assert planner(232, 16, 3, pyramid(300, 200, 3, 2)) is None


def test_random_plans(planner):
    rng = random.Random(5)
    for _ in range(40):
        levels, pairs = rng.randint(2, 5), rng.randint(1, 8)
        w, h = rng.randint(16, 2000) << (levels - 1), rng.randint(2, 600) << (levels - 1)
        R = rng.randint(1, 4)
        out_w, overhead = {1: 248, 2: 240, 3: 240, 4: 232}[R], 3 * R + 4
        items = pyramid(w, h, levels, pairs)
        capacity = rng.choice([2048, 1216, 64, 9])
        min_h = rng.choice([8, 8, 2, 16])
        plan = planner(out_w, overhead, capacity, items, min_h)
        cols = sum(-(-iw // out_w) for iw, _ in items)
        if plan is None:
            assert cols > MAX_SEGS * capacity, (w, h, levels, pairs, capacity)
            continue
        check(plan, out_w, overhead, capacity, items, min_h)
