"""What a session is and where its buffers lie (csrc/session_plan.h) on the host: tools/session_plan_main.cpp is built with the host
compiler and run ONCE over a grid of session descriptions; every field of every plan -- the levels' geometry, the counts and flags,
the byte sizes, the offset of every pointer the session holds and the arena's total -- is compared with the transcription of the
function that held this arithmetic before (tests/session_layout_ref.py), the layout's invariants are asserted on every accepted
plan, and every description the function rejected is rejected with its code and message.  No GPU: the plan is arithmetic only.

tests/test_gpu_session_layout.py compares the pointers of real sessions with the same transcription."""
import itertools
import os
import shutil
import subprocess

import pytest

import session_layout_ref as ref
from cuda_optical_flow_2_amd.parallel import ShardPlan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = 1
SIZES = [(64, 48), (250, 186), (640, 480), (1920, 1088), (3840, 2160), (7680, 4320)]
SWITCHES = {"iter_fused": "OFX_ITER_FUSED", "iter_pairs": "OFX_ITER_PAIRS", "iter_dma": "OFX_ITER_DMA", "pair_pack": "OFX_PAIR_PACK",
            "pair_waves": "OFX_PAIR_WAVES", "debug_corner_extent": "OFX_DEBUG_CORNER_EXTENT"}
ROWS = ("own_y0", "own_y1", "buf_y0", "buf_y1", "comp_y0", "comp_y1")


def max_levels(w, h):
    """Levels 1..6 the dimensions allow: every level that is downsampled is even, the coarsest is not empty."""
    n = 1
    while n < 6 and (w >> (n - 1)) % 2 == 0 and (h >> (n - 1)) % 2 == 0 and (w >> n) > 0 and (h >> n) > 0:
        n += 1
    return n


def sharded(w, h, levels, window, iters, rank, world, comp=True, **more):
    """A rank's description with rows made as parallel.ShardPlan makes them (engine.Session copies them so); comp=False: no comp rows."""
    sp = ShardPlan(w, h, levels, window, rank, world, iters=iters)
    d = dict(width=w, height=h, levels=levels, window=window, iters=iters, sharded=1, own_y0=[r[0] for r in sp.own], own_y1=[r[1] for r in sp.own],
             buf_y0=[r[0] for r in sp.buf], buf_y1=[r[1] for r in sp.buf])
    if comp:
        d.update(comp_y0=[r[0] for r in sp.comp], comp_y1=[r[1] for r in sp.comp])
    d.update(more)
    return d


def grid():
    """A few hundred descriptions: each axis of the issue's grid in full, the others cycling under it so that the values meet in
    changing combinations."""
    out = []
    windows, iters, batches = itertools.cycle([3, 9, 15, 23]), itertools.cycle([1, 2, 3, 5]), itertools.cycle([0, 1, 2, 4, 8, 16])
    modes, patches = itertools.cycle([1, 2, 0]), itertools.cycle([0, 64, 300])
    for (w, h) in SIZES:
        for levels in range(1, max_levels(w, h) + 1):
            for kind in ("plain", "borrow", "two_stage", "local_corner", "local_borrow"):
                for _ in range(2):
                    d = dict(width=w, height=h, levels=levels, window=next(windows), iters=next(iters), stream_batch=next(batches), mode=next(modes))
                    if d["mode"] == 0:
                        d["iters"] = 1   # (compat_cpu takes no iterations)
                    if d["stream_batch"] * levels > 80:
                        d["stream_batch"] = 8   # (OFX_MAX_LK_ITEMS)
                    if kind in ("borrow", "two_stage", "local_borrow"):
                        d["borrow_frames"] = 1
                    if kind == "two_stage":
                        d["stream_two_stage"] = 1
                    if kind in ("two_stage", "local_corner", "local_borrow"):
                        d["patch_size"] = next(patches)
                    if kind in ("local_corner", "local_borrow"):
                        d["local_corner"] = 1
                    out.append(d)
    # every window x iters x stream_batch at one size, where two iterations per launch, the second flow sets and the scratch planes come and go
    for window, it, b in itertools.product([3, 9, 15, 23], [1, 2, 3, 5], [0, 1, 2, 4, 8, 16]):
        out.append(dict(width=640, height=480, levels=4, window=window, iters=it, stream_batch=b, mode=1 + (b & 1)))
    # each switch off and on (and a value for the two that carry one), on sessions that the switch bears on
    base = dict(width=640, height=480, levels=3, window=9, iters=5, stream_batch=2, borrow_frames=1, stream_two_stage=1)
    for name in SWITCHES:
        for v in (0, 1, 7):
            out.append(dict(base, **{name: v}))
            out.append(dict(base, iters=1, stream_two_stage=0, local_corner=1, **{name: v}))
    out.append(dict(base, iter_pairs=1, iter_fused=0))
    out.append(dict(base, iter_pairs=1, iter_dma=1))
    # sharded: with and without comp rows, with iterations (local_corner), every rank of 2 and 3, partial frames
    for (w, h, levels), window, world in itertools.product([(640, 480, 3), (1920, 1088, 4), (3840, 2160, 5)], [3, 9, 15], [2, 3]):
        for rank in range(world):
            out.append(sharded(w, h, levels, window, 1, rank, world, comp=bool(rank & 1)))
            out.append(sharded(w, h, levels, window, 1, rank, world, comp=not (rank & 1), local_corner=1, stream_batch=4, frames_partial=rank & 1))
            out.append(sharded(w, h, levels, window, 3, rank, world, local_corner=1, borrow_frames=1, stream_batch=2, patch_size=0 if rank else 300))
            out.append(sharded(w, h, levels, window, 5, rank, world, comp=False, local_corner=1, mode=2))
    # past the 2 GB rule: a level 0 of 32768 x 16384 (and one just as wide whose flow rows alone pass it)
    out.append(dict(width=32768, height=16384, levels=3, window=9, iters=3))
    out.append(dict(width=32768, height=16384, levels=3, window=9, iters=3, stream_batch=2, borrow_frames=1, stream_two_stage=1))
    out.append(dict(width=32768, height=8192, levels=2, window=5, iters=2))
    out.append(dict(width=32768, height=8190, levels=2, window=5, iters=2))
    # a single-level session with iterations copies its frames
    out.append(dict(width=640, height=480, levels=1, window=9, iters=3, borrow_frames=1))
    out.append(dict(width=640, height=480, levels=1, window=9, iters=3, borrow_frames=1, stream_two_stage=1, stream_batch=2))
    return out


def short_rows():
    """A shard planned without its iterations: the buffers are too short for them."""
    d = sharded(640, 480, 3, 9, 1, 1, 2, local_corner=1)
    d["iters"] = 4
    return d


def bad_rows():
    d = sharded(640, 480, 3, 9, 1, 0, 2)
    d["buf_y1"] = list(d["buf_y1"])
    d["buf_y1"][1] = d["own_y1"][1] - 1
    return d


# one per OFX_REQUIRE or error exit of the function as it stood: (description, a piece of its message)
REJECTED = [
    (dict(width=0, height=48), "bad size 0x48"),
    (dict(width=64, height=48, levels=13), "levels 13 out of range"),
    (dict(width=64, height=48, levels=0), "levels 0 out of range"),
    (dict(width=64, height=48, window=8), "window must be odd and >= 3"),
    (dict(width=64, height=48, window=1), "window must be odd and >= 3"),
    (dict(width=64, height=48, mode=3), "bad mode 3"),
    (dict(width=64, height=48, min_det=-1.0), "min_det must be >= 0"),
    (dict(width=64, height=48, iters=65), "iters 65 out of range"),
    (dict(width=64, height=48, stream_batch=17), "stream_batch 17 (0 .. 16)"),
    (dict(width=1920, height=1088, levels=6, stream_batch=16), "stream_batch 16 needs levels <= 5"),
    (dict(width=64, height=48, levels=2, stream_two_stage=1), "stream_two_stage needs borrow_frames"),
    (dict(width=64, height=48, mode=0, iters=2), "refinement iterations need mode lk_float"),
    (dict(width=64, height=48, deep_fetch=2), "deep_fetch must be -1, 0 or +1 (got 2)"),
    (dict(width=64, height=48, levels=2, frames_partial=1), "frames_partial describes the frames of a sharded local_corner session"),
    (sharded(640, 480, 3, 9, 1, 0, 2, frames_partial=1), "frames_partial describes the frames of a sharded local_corner session"),
    (sharded(640, 480, 3, 9, 1, 0, 2, frames_partial=1, local_corner=1, borrow_frames=1, stream_two_stage=1), "frames_partial describes"),
    (sharded(640, 480, 3, 9, 3, 0, 2), "refinement iterations on a sharded session run through the stream pipeline, which needs local_corner"),
    (dict(width=64, height=48, levels=8), "8 levels is too many for 64x48"),
    (dict(width=250, height=186, levels=3), "level 1 is 125x93; every level that is downsampled must have even dimensions"),
    (bad_rows(), "level 1 shard rows own [0,120) buf [0,119) invalid for height 240"),
    (short_rows(), "level 2: 4 iterations need rows [40,120) in the buffers"),
    (dict(width=640, height=480, levels=4, window=23, local_corner=1, patch_size=64), "patch_size 64 leaves 8x8 at the coarsest level, the corner needs 13"),
]


def line_of(d):
    return " ".join("%s=%s" % (k, ",".join(map(str, v)) if isinstance(v, (list, tuple)) else v) for k, v in d.items())


def split(d):
    """A description as the transcription takes it: (the fields of ofx_params, the environment)."""
    return ({k: v for k, v in d.items() if k not in SWITCHES}, {SWITCHES[k]: v for k, v in d.items() if k in SWITCHES})


def parse(text, n):
    """The tool's output for n descriptions: a list of ("error", code, message) and plan dicts shaped like the transcription's."""
    out, cur = [], None
    for l in text.splitlines():
        word = l.split()
        if word[0] == "error":
            out.append(("error", int(word[1]), l.split(None, 2)[2]))
        elif word[0] == "plan":
            cur = {k: int(v) for k, v in (x.split("=") for x in word[1:])}
            cur["at"] = {}
            levels = []
        elif word[0] == "level":
            assert int(word[1]) == len(levels)
            levels.append({k: int(v) for k, v in (x.split("=") for x in word[2:])})
        elif word[0] == "at":
            key = (word[1], int(word[2]), int(word[3]), int(word[4]))
            assert key not in cur["at"]
            cur["at"][key] = int(word[5])
        else:
            assert word[0] == "end"
            cur.update({k: [lv[k] for lv in levels] for k in levels[0]})
            out.append(cur)
    assert len(out) == n
    return out


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("session_plan") / "session_plan_main")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "cuda_optical_flow_2_amd", "csrc"), os.path.join(ROOT, "tools", "session_plan_main.cpp"), "-o", exe])

    def run(descriptions, *args):
        return subprocess.run([exe, *args], input="".join(line_of(d) + "\n" for d in descriptions), text=True, check=True, stdout=subprocess.PIPE).stdout
    return run


@pytest.fixture(scope="module")
def plans(planner):
    """[(description, the tool's plan)] of the whole grid, through one process."""
    g = grid()
    assert len(g) >= 300
    return list(zip(g, parse(planner(g), len(g))))


def regions(plan):
    """[(offset, bytes, whether it is a u8 plane the fused warp may read past, key)] of a plan, each region once, by offset."""
    size = {"img": "plane_bytes", "sh": "plane_bytes", "itsh": "plane_bytes", "flowset": "flow_bytes", "flowset2": "flow_bytes",
            "pimg": "patch_bytes", "pscr": "patch_bytes", "preloc": "patch_bytes"}
    tables = {"status": ref.align_up(4 * (1 + ref.K_UV_SLOTS), 256), "uv": ref.align_up(ref.MAX_LEVELS * 2 * 4 * ref.K_UV_SLOTS, 256),
              "staging": ref.align_up(plan["w"][0] * plan["h"][0] * 3, 256)}
    out = {}
    for key, off in plan["at"].items():
        name, t, _, k = key
        if name == "flowset" and t >= 1 and off == plan["at"]["flowset", 0, 0, k]:
            continue   # (the sets a session of fewer frames per tick never writes are set 0)
        nbytes = plan[size[name]][k] if name in size else tables[name]
        assert off not in out, (key, out.get(off))
        out[off] = (off, nbytes, size.get(name) in ("plane_bytes", "patch_bytes"), key)
    return sorted(out.values())


def test_the_grid_covers_the_issue(plans):
    ds = [d for d, _ in plans]
    assert {(d["width"], d["height"]) for d in ds} >= set(SIZES)
    assert {d["levels"] for d in ds} == set(range(1, 7))
    for name, values in (("window", [3, 9, 15, 23]), ("iters", [1, 2, 3, 5]), ("stream_batch", [0, 1, 2, 4, 8, 16]), ("patch_size", [0, 64, 300]),
                         ("mode", [0, 1, 2])):
        assert {d.get(name, 0) for d in ds} >= set(values), name
    for name in ("borrow_frames", "stream_two_stage", "local_corner", "sharded", "frames_partial") + tuple(SWITCHES):
        assert {bool(d.get(name, 0)) for d in ds} == {False, True}, name
    assert any(d.get("sharded") and "comp_y1" in d for d in ds) and any(d.get("sharded") and "comp_y1" not in d for d in ds)
    assert any(d.get("sharded") and d["iters"] > 1 for d in ds)


def test_plan_equals_the_function_it_replaces(plans):
    accepted = 0
    for d, got in plans:
        what = line_of(d)
        try:
            want = ref.layout(*split(d))
        except ref.LayoutError as e:   # (a patch_size of the grid that is too small for the window)
            assert got == ("error", E_INVALID, str(e)), what
            continue
        assert not isinstance(got, tuple), (what, got)
        assert set(got) == set(want), what
        for k in want:
            assert got[k] == want[k], (what, k)
        accepted += 1
    assert accepted >= 300
    # the paths the grid must reach
    flags = [p for _, p in plans if not isinstance(p, tuple)]
    for name in ("repair", "fused_iters", "iter_pairs", "debug_extent", "pair_pack", "pair_waves"):
        assert {bool(p[name]) for p in flags} == {False, True}, name
    assert any(p["iter_pairs"] for p in flags) and any(k[0] == "flowset2" for p in flags for k in p["at"])
    assert {p["frames_per_slot"] for p in flags} == {0, 1, 2, 3}
    big = [p for d, p in plans if d["width"] == 32768]
    assert len(big) == 4 and [p["fused_iters"] for p in big] == [0, 0, 0, 1] and not any(p["iter_pairs"] for p in big)


def test_layout_invariants(plans):
    for d, plan in plans:
        if isinstance(plan, tuple):
            continue
        what = line_of(d)
        rs = regions(plan)
        assert all(off % 256 == 0 and nbytes > 0 for off, nbytes, _, _ in rs), what
        assert rs[0][0] == 0, what
        for (off, nbytes, _, key), nxt in zip(rs, rs[1:]):
            assert off + nbytes <= nxt[0], (what, key, nxt[3])   # no two regions overlap
        assert plan["total"] == rs[-1][0] + rs[-1][1], what     # total = the end of the last region
        # the fused warp reads three bytes past a plane: 64 bytes of the plane's own region lie behind its last row, inside the arena
        L = len(plan["w"])
        for off, nbytes, is_plane, (name, _, _, k) in rs:
            if is_plane:
                used = plan["ppitch"][k] * plan["ph"][k] if name in ("pimg", "pscr", "preloc") else plan["pitch"][k] * (plan["buf1"][k] - plan["buf0"][k])
                assert used + 64 <= nbytes and off + used + 64 <= plan["total"], (what, name, k)
        # every pointer a session of this kind uses is there
        assert all(("img", t, 0, k) in plan["at"] and ("flowset", b, 0, k) in plan["at"] for t in range(plan["n_sets"]) for b in range(16) for k in range(L)), what


def test_second_flow_sets_lie_behind_everything_else(planner, plans):
    """The offsets of everything but flowset2 are the same with iter_pairs on and off."""
    on = [(d, p) for d, p in plans if not isinstance(p, tuple) and p["iter_pairs"]]
    assert len(on) >= 10
    off = parse(planner([dict(d, iter_pairs=0) for d, _ in on]), len(on))
    for (d, with_), without in zip(on, off):
        assert not without["iter_pairs"] and not any(k[0] == "flowset2" for k in without["at"])
        second = {k: v for k, v in with_["at"].items() if k[0] == "flowset2"}
        assert second and {k: v for k, v in with_["at"].items() if k[0] != "flowset2"} == without["at"], line_of(d)
        assert min(second.values()) == without["total"], line_of(d)


def test_rejected_descriptions_keep_code_and_message(planner):
    got = parse(planner([d for d, _ in REJECTED]), len(REJECTED))
    for (d, piece), g in zip(REJECTED, got):
        assert isinstance(g, tuple) and g[1] == E_INVALID, (line_of(d), g)
        assert g[2].startswith("ofx_session_create: ") and piece in g[2], (line_of(d), g[2])
    # the three exits of the layout: the transcription raises the same text
    for d, g in zip([d for d, _ in REJECTED], got):
        if d.get("sharded") and "shard rows" in g[2] or "iterations need rows" in g[2] or "patch_size" in g[2]:
            with pytest.raises(ref.LayoutError) as e:
                ref.layout(*split(d))
            assert str(e.value) == g[2]


def test_summary_adds_up(planner):
    out = planner([dict(width=3840, height=2160, levels=5), dict(width=7680, height=4320, levels=6, stream_batch=4)], "--summary")
    assert "DO NOT ADD UP" not in out
    totals = [float(l.split()[1]) for l in out.splitlines() if l.startswith("arena")]
    assert [round(t) for t in totals] == [191, 2223]
