"""What an LK launch does (csrc/lk_plan.h) on the host: tools/lk_plan_main.cpp is built with the host compiler and run ONCE over all the
descriptions below.  The strips of every case are decoded the way the kernels decode them and must march every output row of every
tile column of every item exactly once, within the capacity; every table, every wave count and every kernel variant equals the
transcription of the code that held this arithmetic before (tests/lk_plan_ref.py), every launch that code rejected is rejected with
its code and message, and every variant is one that build.SOURCES instantiates.  No GPU: the plan is arithmetic only."""
import functools
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import lk_plan_ref as ref
from cuda_optical_flow_2_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_ITEMS = 80   # OFX_MAX_LK_ITEMS
WIDTHS = [1, 3, 4, 223, 224, 225, 240, 241, 248, 256, 480, 1919, 1920, 3840]
HEIGHTS = [1, 2, 7, 8, 9, 15, 16, 17, 135, 1080, 2160]
TILE_WIDTHS = [224, 232, 240, 248]   # TileGeom<R>::OUT_W for R = 1 .. 12, TileGeomP<R>::OUT_W for R = 1 .. 4
CAPACITIES = [1, 7, 256, 1024, 2048, 4096, 8192]
MIN_HEIGHTS = [1, 8, 1000]
SWITCH_WORDS = {"OFX_LK_DMA": "lk_dma", "OFX_ITER_DMA": "iter_dma", "OFX_LK_MIN_STRIP": "min_strip", "OFX_LK_WAVES_PER_SIMD": "waves_per_simd",
                "OFX_LK_FILL": "fill", "OFX_LK_TARGET_WAVES": "target_waves"}


def item(w, h, out=None, rows=None, pitch=None, flow_row0=0):
    out, rows = out or (0, h), rows or (0, h)
    return dict(w=w, h=h, pitch=pitch or (w + 63) // 64 * 64, row0=rows[0], row_end=rows[1], out_y0=out[0], out_y1=out[1], flow_row0=flow_row0,
                accumulate=0, warp_out=0)


def item_word(a):
    return "%dx%d@%d:%d/%d:%dp%df%d" % (a["w"], a["h"], a["out_y0"], a["out_y1"], a["row0"], a["row_end"], a["pitch"], a["flow_row0"])


def line_of(launch, items, env, **words):
    words = dict(words, **{SWITCH_WORDS[k]: v for k, v in env.items() if v is not None})
    if items:
        words.update(items=",".join(item_word(a) for a in items), accumulate=items[0]["accumulate"], warp_out=items[0]["warp_out"])
    return " ".join(["launch=" + launch] + ["%s=%s" % kv for kv in words.items()])


def pyramid(w, h, levels, pairs):
    """the whole levels of a tick's pairs, per pair the coarsest first"""
    return [item(max(w >> k, 1), max(h >> k, 1)) for _ in range(pairs) for k in range(levels - 1, -1, -1)]


def row_window(w, h):
    """a shard's item: the planes hold a window of the level's rows, the launch writes fewer still (out_y0 > 0, out_y1 < h)"""
    y0, y1 = max(h // 3, 1), h - max(h // 5, 1)
    return item(w, h, out=(y0, y1), rows=(max(y0 - 5, 0), min(y1 + 5, h)), flow_row0=max(y0 - 2, 0))


@functools.lru_cache(maxsize=None)
def strip_cases():
    """[(items, out_w, capacity, min_h)]: every size x every tile width for single items and row windows, every capacity x every minimum
    on the sizes' diagonal, and pyramids of 2 .. 6 levels x 1 / 2 / 8 / 16 pairs (as many as 80 items hold) x every capacity; the
    axes not spelt out cycle, so that their values meet in changing combinations."""
    caps, mins, tiles = itertools.cycle(CAPACITIES), itertools.cycle(MIN_HEIGHTS), itertools.cycle(TILE_WIDTHS)
    out = []
    for w, h, out_w in itertools.product(WIDTHS, HEIGHTS, TILE_WIDTHS):
        out.append(([item(w, h)], out_w, next(caps), next(mins)))
        if h >= 3:
            out.append(([row_window(w, h)], out_w, next(caps), next(mins)))
    for (w, h), cap, min_h in itertools.product(zip(WIDTHS, itertools.cycle(HEIGHTS)), CAPACITIES, MIN_HEIGHTS):
        out.append(([item(w, h)], next(tiles), cap, min_h))
    sizes = itertools.cycle([(w, h) for w in WIDTHS[3:] for h in HEIGHTS[6:]])
    for levels, pairs, cap in itertools.product(range(2, 7), [1, 2, 8, 16], CAPACITIES):
        for _ in range(3):
            out.append((pyramid(*next(sizes), levels, min(pairs, MAX_ITEMS // levels)), next(tiles), cap, next(mins)))
    # a shard's tick: the row windows of two pairs' pyramids
    for (w, h), cap in itertools.product([(1920, 1080), (3840, 2160), (241, 135)], CAPACITIES):
        out.append(([row_window(max(w >> k, 1), max(h >> k, 1)) for _ in range(2) for k in (2, 1, 0)], next(tiles), cap, next(mins)))
    return out


# ---- the variants: one axis each of the issue's product -------------------------------------------------------------------------
SIZES = {"below": (4000, 3999), "at": (4000, 4000), "above": (4001, 4000)}   # the largest level against 16 Mpx
DMA = [None, 0, 1]


def variant_items(size, rowwin, fits, several, accumulate, warp_out):
    """one or two pairs of two levels, the coarse one first; !fits: the large level's planes pass 2 GB (by their pitch)"""
    w, h = SIZES[size]
    out = []
    for _ in range(2 if several else 1):
        for ww, hh in ((w // 2, h // 2), (w, h)):
            a = item(ww, hh, out=(20, hh - 20), rows=(10, hh - 10), flow_row0=15) if rowwin else item(ww, hh)
            if not fits and ww == w:
                a["pitch"] = 600000
            out.append(dict(a, accumulate=accumulate, warp_out=warp_out))
    return out


def session_launch(size, iter_dma):
    return line_of("levels", variant_items(size, 0, 1, 0, 1, 0)[1:], dict(ref.ENV, OFX_ITER_DMA=iter_dma), mode=1, sums=0)


@functools.lru_cache(maxsize=None)
def variant_cases():
    """{the tool's line: what the transcription says}: a variant dict or a Rejected.  The full product; the axes a launch does not read
    collapse into one line."""
    out = {}
    for mode, sums, acc, wout, rowwin, fits, size, iter_dma, lk_dma, hint, several in itertools.product(
            (0, 1, 2), (0, 1), (0, 1), (0, 1), (0, 1), (1, 0), SIZES, DMA, DMA, (-1, 0, 1), (0, 1)):
        items = variant_items(size, rowwin, fits, several, acc, wout)
        env = dict(ref.ENV, OFX_ITER_DMA=iter_dma, OFX_LK_DMA=lk_dma)
        try:
            want = ref.levels_variant(items, 4, mode, bool(sums), env)
        except ref.Rejected as e:
            want = e
        out.setdefault(line_of("levels", items, dict(ref.ENV, OFX_ITER_DMA=iter_dma), mode=mode, sums=sums), want)
        if not acc and not sums:   # (ofx_stream_launch takes neither)
            out.setdefault(line_of("tick", items, dict(ref.ENV, OFX_LK_DMA=lk_dma), mode=mode, hint=hint), ref.tick_variant(items, mode, hint, env))
    # windows: the last one of each mode and the first one past it, on a levels and on an iteration launch
    for mode, window, acc in itertools.product((0, 1, 2), (3, 23, 25, 27), (0, 1)):
        items = [dict(item(640, 480), accumulate=acc)]
        try:
            want = ref.levels_variant(items, window >> 1, mode, False, ref.ENV)
        except ref.Rejected as e:
            want = e
        out[line_of("levels", items, ref.ENV, mode=mode, window=window)] = want
    for size, dma in itertools.product(SIZES, (None, 1)):   # a session's level 0 in an iteration launch
        out[session_launch(size, dma)] = ref.levels_variant(variant_items(size, 0, 1, 0, 1, 0)[1:], 4, 1, False, dict(ref.ENV, OFX_ITER_DMA=dma))
    out[line_of("tick", [], ref.ENV, mode=1, lk_dma=1)] = ref.tick_variant([], 1, 0, dict(ref.ENV, OFX_LK_DMA=1))   # a tick without LK items
    return out


# the kernels of the LK families, unit by unit, as (family, MODE, FAST, SUMS, ITER / WOUT, DMA); None: both values
INSTANTIATED = {
    "lk_inst_levels_c.hip": [("levels", 0, 0, None, 0, 0)],
    "lk_inst_levels_f.hip": [("levels", 1, 0, None, 0, 0)],
    "lk_inst_levels_fast.hip": [("levels", 1, 1, 0, 0, 0)],
    "lk_inst_iter_f1.hip": [("iter", 1, 0, 0, 1, None)], "lk_inst_iter_fast1.hip": [("iter", 1, 1, 0, 1, None)],
    "lk_inst_iter_f2.hip": [("iter", 1, 0, 0, 2, None)], "lk_inst_iter_fast2.hip": [("iter", 1, 1, 0, 2, None)],
    "lk_inst_iter_f3.hip": [("iter", 1, 0, 0, 3, None)], "lk_inst_iter_fast3.hip": [("iter", 1, 1, 0, 3, None)],
    "lk_inst_iter_f4.hip": [("iter", 1, 0, 0, 4, None)], "lk_inst_iter_fast4.hip": [("iter", 1, 1, 0, 4, None)],
    "lk_inst_stream_c.hip": [("stream", 0, 0, 0, 0, None)],
    "lk_inst_stream_f.hip": [("stream", 1, 0, 0, 0, None)], "lk_inst_stream_fast.hip": [("stream", 1, 1, 0, 0, None)],
    "lk_inst_stream_fw.hip": [("stream", 1, 0, 0, 3, 0)], "lk_inst_stream_fastw.hip": [("stream", 1, 1, 0, 3, 0)],
    "lk_inst_stream_fwr.hip": [("stream", 1, 0, 0, 5, 0)], "lk_inst_stream_fastwr.hip": [("stream", 1, 1, 0, 5, 0)],
}


@functools.lru_cache(maxsize=None)
def capacity_cases():
    """[(line, the transcription's wave count)]: CUs x occupancy x the four call sites x each switch unset and set"""
    out = []
    for cus, occ, (site, (reserve, dflt, full_fill)) in itertools.product((1, 64, 256), range(1, 9), ref.CALL_SITES.items()):
        for per_simd, fill, target in itertools.product((None, 3), (None, 90), (None, 6144)):
            env = dict(ref.ENV, OFX_LK_WAVES_PER_SIMD=per_simd, OFX_LK_FILL=fill, OFX_LK_TARGET_WAVES=target)
            out.append((line_of("levels", [], env, cus=cus, occ=occ, reserve=reserve, dflt=dflt, full_fill=full_fill), ref.wave_target(cus, occ, reserve, dflt, full_fill, env)))
    return out


DESIGN_MD_TICK = "pyramid=3840x2160:5:8 out_w=240 cus=256 occ=5"   # (the stream kernel of lk_float: five blocks of four waves per CU)


@functools.lru_cache(maxsize=None)
def all_lines():
    """every description the test gives the tool"""
    strips = [line_of("tick", items, dict(ref.ENV, OFX_LK_MIN_STRIP=min_h), out_w=out_w, capacity=cap) for items, out_w, cap, min_h in strip_cases()]
    return strips + list(variant_cases()) + [l for l, _ in capacity_cases()] + [DESIGN_MD_TICK]


def parse(text, n):
    """the tool's output for n descriptions: per description a Rejected, or a dict with "variant", "capacity" and the strip table"""
    out, cur = [], {}
    for l in text.splitlines():
        word = l.split()
        if word[0] == "error":
            out.append(ref.Rejected(int(word[1]), l.split(None, 2)[2]))
        elif word[0] == "variant":
            cur["variant"] = {k: v if k == "family" else int(v) for k, v in (x.split("=") for x in word[1:])}
        elif word[0] == "capacity":
            cur["capacity"] = int(word[1])
        elif word[0] == "strips":
            cur.update(H=int(word[1][2:]), blocks=int(word[2][6:]), w=[], tiles_x=[], strip_h=[], first_block=[])
        elif word[0] == "item":
            assert int(word[1]) == len(cur["w"])
            for k, v in (x.split("=") for x in word[2:]):
                if k != "h":
                    cur[{"first": "first_block"}.get(k, k)].append(int(v))
        else:
            assert word[0] == "end"
            if "first_block" in cur:
                cur["first_block"].append(cur["blocks"])
            out.append(cur)
            cur = {}
    assert len(out) == n
    return out


def compile_tool(tmp, name):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp / name)
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "cuda_optical_flow_2_amd", "csrc"), os.path.join(ROOT, "tools", name + ".cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """{line: what the tool printed for it}, through one process"""
    exe = compile_tool(tmp_path_factory.mktemp("lk_plan"), "lk_plan_main")
    lines = all_lines()
    text = subprocess.run([exe], input="".join(l + "\n" for l in lines), text=True, check=True, stdout=subprocess.PIPE).stdout
    return dict(zip(lines, parse(text, len(lines))))


@pytest.fixture(scope="module")
def strips(results):
    cases = strip_cases()
    return [(c, results[l]) for c, l in zip(cases, all_lines())]


def wave_count(items, out_w, min_h, H):
    """waves of a plan with the common strip height H"""
    return sum(-(-a["w"] // out_w) * -(-(a["out_y1"] - a["out_y0"]) // min(max(H, min_h), a["out_y1"] - a["out_y0"])) for a in items)


def test_the_grid_covers_the_issue():
    cases = strip_cases()
    assert {(a["w"], a["h"]) for items, _, _, _ in cases if len(items) == 1 for a in items} >= set(itertools.product(WIDTHS, HEIGHTS))
    single = {(items[0]["w"], items[0]["h"], out_w) for items, out_w, _, _ in cases if len(items) == 1}
    assert single >= set(itertools.product(WIDTHS, HEIGHTS, TILE_WIDTHS))
    assert {(cap, min_h) for _, _, cap, min_h in cases} == set(itertools.product(CAPACITIES, MIN_HEIGHTS))
    pyramids = [(items, cap) for items, _, cap, _ in cases if len(items) > 1 and items[0]["out_y0"] == 0]
    assert {len(items) for items, _ in pyramids} >= {levels * min(pairs, MAX_ITEMS // levels) for levels in range(2, 7) for pairs in (1, 2, 8, 16)}
    assert max(len(items) for items, _ in pyramids) == MAX_ITEMS and {cap for _, cap in pyramids} == set(CAPACITIES)
    windows = [items for items, _, _, _ in cases if items[0]["out_y0"] > 0]
    assert len(windows) >= 500 and all(a["out_y0"] > 0 and a["out_y1"] < a["h"] for items in windows for a in items)
    assert any(len(items) > 1 for items in windows)


def test_every_row_is_marched_once(strips):
    assert len(strips) >= 1500
    for (items, out_w, cap, min_h), t in strips:
        what = (len(items), items[-1]["w"], items[-1]["h"], out_w, cap, min_h)
        n = len(items)
        first, tiles_x, strip_h = np.array(t["first_block"]), np.array(t["tiles_x"]), np.array(t["strip_h"])
        y0s, y1s = np.array([a["out_y0"] for a in items]), np.array([a["out_y1"] for a in items])
        assert first[0] == 0 and (np.diff(first) >= 0).all() and first[n] == t["blocks"], what
        assert (tiles_x == [-(-a["w"] // out_w) for a in items]).all(), what
        # every block, as lk_wave_buf decodes it
        b = np.arange(t["blocks"])
        lv = np.searchsorted(first, b, side="right") - 1   # the last item whose first_block <= b
        block = b - first[lv]
        tile, strip = block % tiles_x[lv], block // tiles_x[lv]
        ys = y0s[lv] + strip * strip_h[lv]
        ye = np.minimum(ys + strip_h[lv], y1s[lv])
        assert (ye > ys).all(), what   # no empty strip
        # A tile column's strips start strip_h apart and are at most strip_h long: distinct strips do not overlap, and (item, tile,
        # strip) is one block.  So the column is tiled exactly once when its strips' rows add up to rows_out.
        col0 = np.concatenate([[0], np.cumsum(tiles_x)])
        rows = np.bincount(col0[lv] + tile, weights=ye - ys, minlength=col0[n])
        assert (rows == np.repeat(y1s - y0s, tiles_x)).all(), what
        # one common height, the smallest within the capacity
        H = t["H"]
        assert H >= min_h and (strip_h == np.minimum(np.maximum(H, min_h), y1s - y0s)).all(), what
        assert t["blocks"] == wave_count(items, out_w, min_h, H), what
        max_rows = int((y1s - y0s).max())
        assert t["blocks"] <= cap or H == max(max_rows, min_h), what   # (past the tallest item nothing changes)
        assert H == min_h or wave_count(items, out_w, min_h, H - 1) > cap, what
        assert t["blocks"] <= max(cap, int(tiles_x.sum())), what


def test_the_wave_count_does_not_grow_with_the_height():
    """... which is what makes "the smallest height within the capacity" well defined (checked above at H - 1 only)"""
    for items, out_w, _, min_h in strip_cases()[::7]:
        top = max(a["out_y1"] - a["out_y0"] for a in items)
        counts = [wave_count(items, out_w, min_h, H) for H in sorted(set(range(min_h, top + 2, max(top // 40, 1))) | {top, top + 1})]
        assert all(a >= b for a, b in zip(counts, counts[1:])) and counts[-1] == sum(-(-a["w"] // out_w) for a in items)


def test_strips_equal_the_function_they_replace(strips):
    for (items, out_w, cap, min_h), t in strips:
        want = ref.plan_table(items, out_w, cap, dict(ref.ENV, OFX_LK_MIN_STRIP=min_h))
        for k in want:
            assert t[k] == want[k], (k, len(items), items[-1]["w"], items[-1]["h"], out_w, cap, min_h)
        assert t["variant"]["family"] == "stream" and t["w"] == [a["w"] for a in items]
    # OFX_LK_MIN_STRIP unset, 0 and negative: 8 rows
    assert ref.plan_table([item(300, 200)], 240, 4096, ref.ENV)["strip_h"] == [8] == ref.plan_table([item(300, 200)], 240, 4096, dict(OFX_LK_MIN_STRIP=-2))["strip_h"]


def test_capacity_equals_the_function_it_replaces(results):
    cases = capacity_cases()
    assert len(cases) == 3 * 8 * 4 * 8
    for line, want in cases:
        assert results[line]["capacity"] == want, line
    assert len({want for _, want in cases}) > 20   # (the grid is not degenerate)


def test_variants_equal_the_code_they_replace(results):
    cases = variant_cases()
    seen, rejected = set(), set()
    for line, want in cases.items():
        got = results[line]
        if isinstance(want, ref.Rejected):
            assert isinstance(got, ref.Rejected) and (got.code, str(got)) == (want.code, str(want)), (line, got)
            rejected.add((want.code, str(want)))
            continue
        assert not isinstance(got, ref.Rejected) and got["variant"] == want, (line, got)
        v = got["variant"]
        seen.add((v["family"], v["mode"], v["fast"], v["sums"], v["iter"], v["deep"]))
    # its three rejections
    assert rejected == {(ref.E_INVALID, "ofx_lk_levels: d_warp_out needs mode lk_float and levels below 2 GB"),
                        (ref.E_INVALID, "ofx_lk_levels: iteration 1 with d_warp_out on a row window runs in the stream tick only"),
                        (ref.E_UNSUPPORTED, "ofx_lk_level: window 25 not supported in mode 1"), (ref.E_UNSUPPORTED, "ofx_lk_level: window 27 not supported in mode 1"),
                        (ref.E_UNSUPPORTED, "ofx_lk_level: window 27 not supported in mode 0")}
    # every variant is a kernel the build has, and the product reaches every kernel of these families
    units = {s for s in build.SOURCES if s.startswith(("lk_inst_levels", "lk_inst_iter", "lk_inst_stream"))}
    assert units == set(INSTANTIATED)
    have = {tuple(c) for u in units for k in INSTANTIATED[u] for c in itertools.product(*[(0, 1) if x is None else (x,) for x in k])}
    assert seen == have
    assert {v["many"] for v in (results[l]["variant"] for l, w in cases.items() if not isinstance(w, ref.Rejected))} == {0, 1}


def test_the_session_asks_the_iteration_launch_about_the_deep_fetch(results, tmp_path):
    """A session has no two-iteration form where its iteration launches may take the deep fetch: session_plan_make asks the launch's
    rule, with the switch as a session reads it -- OFX_ITER_DMA on, or not (0 leaves the size to decide there)."""
    session = compile_tool(tmp_path, "session_plan_main")
    cases = [(w, h, dma) for (w, h), dma in itertools.product(SIZES.values(), DMA)]
    text = subprocess.run([session], input="".join("width=%d height=%d iters=3%s\n" % (w, h, "" if dma is None else " iter_dma=%d" % dma) for w, h, dma in cases),
                          text=True, check=True, stdout=subprocess.PIPE).stdout
    pairs = [int(l.split("iter_pairs=")[1].split()[0]) for l in text.splitlines() if l.startswith("plan ")]
    assert len(pairs) == len(cases) and set(pairs) == {0, 1}
    for (w, h, dma), two in zip(cases, pairs):
        size = next(k for k, v in SIZES.items() if v == (w, h))
        assert two == (not results[session_launch(size, 1 if dma else None)]["variant"]["deep"]), (w, h, dma)


def test_the_4k_tick_of_design_md(results):
    """a 4K tick of 8 pairs on 240-column tiles: strips of 90 rows, 4 096 waves"""
    t = results[DESIGN_MD_TICK]
    assert (t["capacity"], t["H"], t["blocks"]) == (4096, 90, 4096) and t["variant"] == ref.variant("stream", 1, many=True)
    want = ref.plan_table(pyramid(3840, 2160, 5, 8), 240, ref.wave_target(256, 5, *ref.CALL_SITES["tick_many"], ref.ENV), ref.ENV)
    assert all(t[k] == want[k] for k in want)
