"""The plan of the fused two-iteration launch (csrc/pair_plan.h, csrc/lk_launch.h): waves of equal steps, each marching up to two
segments -- rows of a tile column of some (pair, level) item -- and the column-exact tile of csrc/lk_body_pair.h (232 columns at
9x9, 248 at 3x3).  Three sessions are compared bit for bit, every level of every pair:

    OFX_PAIR_PACK=1   the packed plan (the default)
    OFX_PAIR_PACK=0   one strip per wave (plan_table_g), on the new tile
    OFX_ITER_PAIRS=0  one launch per iteration: neither the fused tile nor either plan

All three switches are read when a session is created.  OFX_PAIR_WAVES sets the wave count of the packed plan: with a few waves the
small levels used here straddle waves as 4K levels straddle 2 048 -- a wave then holds segments of different tile columns, levels
and pairs.  As in test_gpu_iteration_pairs.py the widths that matter to the tile are those of LEVEL 1 of a frame twice as wide."""
import numpy as np
import pytest

from cuda_optical_flow_2_amd import synth
from conftest import assert_same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cuda_optical_flow_2_amd import engine

    return engine


def _frames(w, h, nf):
    """smooth texture above, noise below, and a flat block in every frame: non-finite flows and huge finite ones"""
    import torch

    out = []
    for i in range(nf):
        f = synth.random_pair(w, h, seed=w + 7 * i)[i & 1]
        sm = synth.smooth_pair(w, h, 1.5 * i, -0.9 * i, seed=w)[1]
        f[: h // 2] = sm[: h // 2]
        f[h // 3: h // 3 + 40, w // 4: w // 4 + 90] = 77
        buf = torch.zeros((h, (w + 63) // 64 * 64), dtype=torch.uint8, device="cuda")[:, :w]
        buf.copy_(torch.from_numpy(np.ascontiguousarray(f)))
        out.append(buf)
    return out


def _stream(eng, frames, w, h, L, win, mode, iters, B):
    """every pair's flow pyramid through a streamed session"""
    import torch

    s = eng.Session(w, h, L, win, mode, iters=iters, stream_batch=B)
    s.stream_begin()
    got, seen = {}, 0

    def snap(done):
        nonlocal seen
        if done >= 1:
            for p in range(max(seen + 1, done - B + 1), done + 1):
                got[p] = [s.flow_of(p, k)[0].clone() for k in range(L)]
            seen = done
    for f in frames:
        snap(s.stream_submit(f))
    while True:
        d = s.stream_drain()
        if d == -2:
            break
        snap(d)
    torch.cuda.synchronize()
    s.close()
    assert sorted(got) == list(range(1, len(frames)))
    return {p: [t.cpu().numpy() for t in v] for p, v in got.items()}


def _three_ways(eng, monkeypatch, size, win, iters, mode, B, waves=0, min_strip=0, want_nonfinite=False):
    w, h, L = size
    frames = _frames(w, h, 2 * B + 1)   # a full tick and partial ones: two launch shapes and more
    if min_strip:
        monkeypatch.setenv("OFX_LK_MIN_STRIP", str(min_strip))
    monkeypatch.setenv("OFX_ITER_PAIRS", "0")
    want = _stream(eng, frames, w, h, L, win, mode, iters, B)
    monkeypatch.setenv("OFX_ITER_PAIRS", "1")
    monkeypatch.setenv("OFX_PAIR_PACK", "0")
    strips = _stream(eng, frames, w, h, L, win, mode, iters, B)
    monkeypatch.setenv("OFX_PAIR_PACK", "1")
    if waves:
        monkeypatch.setenv("OFX_PAIR_WAVES", str(waves))
    packed = _stream(eng, frames, w, h, L, win, mode, iters, B)
    if want_nonfinite:
        assert any(not np.isfinite(want[p][0]).all() for p in want), "the flat block was meant to produce non-finite flows"
    what = f"{mode} {w}x{h} win {win} iters {iters} B {B} waves {waves}"
    for p in want:
        for k in range(L):
            assert_same(strips[p][k], want[p][k], f"{what}: one strip per wave: pair {p} level {k}")
            assert_same(packed[p][k], want[p][k], f"{what}: packed: pair {p} level {k}")


def _id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


# level-1 widths around the new tiles: 9x9 (232 columns) 231 / 232 / 233 / 463 / 465 and 237 (a last tile of 5 columns, narrower than
# the 12-column inset); 3x3 (248 columns) 247 / 248 / 249.  3, 5 and 6 iterations: one fused launch, two, two and a left-over single.
WIDTHS = [
    ((462, 40, 2), 9, 5, "lk_float", 1), ((464, 40, 2), 9, 3, "lk_float_fast", 2), ((466, 40, 2), 9, 6, "lk_float", 1),
    ((926, 40, 2), 9, 5, "lk_float_fast", 1), ((930, 40, 2), 9, 3, "lk_float", 2), ((474, 40, 2), 9, 5, "lk_float", 1),
    ((494, 40, 2), 3, 5, "lk_float", 1), ((496, 40, 2), 3, 6, "lk_float_fast", 2), ((498, 40, 2), 3, 3, "lk_float", 1),
    ((480, 264, 2), 7, 5, "lk_float", 2), ((482, 264, 2), 5, 6, "lk_float_fast", 1),
]


@pytest.mark.parametrize("size,win,iters,mode,B", WIDTHS, ids=_id)
def test_widths_around_the_column_exact_tile(eng, monkeypatch, size, win, iters, mode, B):
    """Lanes that the old inset kept out now carry output (9x9: lanes 3 and 60; 3x3: lanes 1 and 62), and the tiles' seams move."""
    _three_ways(eng, monkeypatch, size, win, iters, mode, B, want_nonfinite=size[1] >= 200)


# three levels whose coarsest is 5 / 11 / 17 / 40 rows high: below the lag R + 2, at and above a segment's priming
HEIGHTS = [((464, 20, 3), 9, 5, "lk_float", 2), ((464, 44, 3), 9, 3, "lk_float_fast", 1), ((464, 68, 3), 7, 6, "lk_float", 2),
           ((464, 160, 3), 9, 5, "lk_float", 1), ((464, 44, 3), 3, 5, "lk_float", 1), ((464, 68, 3), 5, 3, "lk_float_fast", 2)]


@pytest.mark.parametrize("size,win,iters,mode,B", HEIGHTS, ids=_id)
def test_heights_below_and_above_the_lag(eng, monkeypatch, size, win, iters, mode, B):
    _three_ways(eng, monkeypatch, size, win, iters, mode, B)


# 300x200, three levels: 4 tile columns per pair.  B = 2 with 5 and 7 waves and B = 1 with 3: every wave holds two segments, of
# different tile columns, levels and pairs (two segments per wave: 8 tile columns need 4 waves at least).  With a minimum segment of 2
# rows, 12 waves cut level 0 at row 2 and 21 waves cut it at row 198 of 200: within R + 1 rows of the level's top and bottom.
STRADDLE = [
    ((300, 200, 3), 9, 5, "lk_float", 2, 5, 0), ((300, 200, 3), 9, 6, "lk_float_fast", 2, 7, 0), ((300, 200, 3), 9, 3, "lk_float", 1, 3, 0),
    ((300, 200, 3), 7, 5, "lk_float_fast", 2, 5, 0), ((300, 200, 3), 5, 3, "lk_float", 2, 7, 0), ((300, 200, 3), 3, 6, "lk_float", 2, 5, 0),
    ((300, 200, 3), 9, 5, "lk_float", 2, 12, 2), ((300, 200, 3), 9, 5, "lk_float_fast", 2, 21, 2),
]


@pytest.mark.parametrize("size,win,iters,mode,B,waves,min_strip", STRADDLE, ids=_id)
def test_segments_that_straddle_waves(eng, monkeypatch, size, win, iters, mode, B, waves, min_strip):
    _three_ways(eng, monkeypatch, size, win, iters, mode, B, waves=waves, min_strip=min_strip, want_nonfinite=True)


@pytest.mark.parametrize("win", [3, 5, 7, 9])
def test_packed_plan_matches_the_oracle(eng, oracle, monkeypatch, win):
    """One packed configuration per window, forced to straddle, against the restatement."""
    import torch

    w, h, L, iters = 300, 200, 3, 5
    p, n = synth.smooth_pair(w, h, 1.2, -0.8)
    monkeypatch.setenv("OFX_ITER_PAIRS", "1")
    monkeypatch.setenv("OFX_PAIR_PACK", "1")
    monkeypatch.setenv("OFX_PAIR_WAVES", "3")
    got = _stream(eng, [torch.from_numpy(p).cuda(), torch.from_numpy(n).cuda()], w, h, L, win, "lk_float", iters, 1)
    want = oracle.flow_pair_iter(p, n, L, win, iters)
    for k in range(L):
        assert_same(got[1][k], want[k], f"win {win}: level {k}")
