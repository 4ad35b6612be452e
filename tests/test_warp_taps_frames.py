"""What the frames and the wave counts of test_gpu_warp_taps.py are there for, checked without a GPU (warp_taps_cases.py):

  * with the oracle: in every case the pair of flat-block frames has pixels whose flow is not finite BEFORE an iteration that warps
    (iterations 1 .. iters - 1: the taps of such a pixel are the "no warp" taps), on both levels, and the pair of noise frames has
    finite flows whose taps are clamped at the left, the right, the top and the bottom border of level 1;
  * with the planner (tools/pair_plan_main.cpp, minimum piece 1): with the case's OFX_PAIR_WAVES every wave carries two segments or
    shares a tile column with another wave, and over all cases cuts fall within two rows of a column's top and of its bottom.

One oracle run per distinct (window, level-1 size); the restatement takes a few milliseconds at these sizes."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import warp_taps_cases as wt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _flows_before_each_warp(orc, prev, nxt, win, upto, levels):
    """{level: the flows after 1 .. upto iterations}, i.e. what the warps of iterations 2 .. upto + 1 start from, for `levels`
    (a subset of the pyramid's, the coarsest included: a level is shifted by the first iteration's flow of the one above)"""
    L = wt.LEVELS
    pp = orc.gauss_pyramid(np.repeat(prev[:, :, None], 3, 2), L)
    npyr = orc.gauss_pyramid(np.repeat(nxt[:, :, None], 3, 2), L)
    h, w = prev.shape
    first = [np.zeros((h >> k, w >> k, 2), np.float32) for k in range(L)]
    out = {}
    for k in sorted(levels, reverse=True):
        nxt3 = npyr[k] if k == L - 1 else orc.shift_back_pyramid(npyr[k], k, L, first)
        res = [orc.lk_iter_level(pp[k][:, :, 0], nxt3[:, :, 0], win, j) for j in range(1, upto + 1)]
        out[k], first[k] = [r[0] for r in res], res[0][1]
    return out


def _clamped_borders(flow, scale):
    """which borders (left, right, top, bottom) finite flows send a tap coordinate across"""
    h, w, _ = flow.shape
    fin = np.isfinite(flow).all(axis=-1) & (np.abs(flow) <= 1e9).all(axis=-1)
    sx = np.arange(w, dtype=np.float32)[None, :] + scale * flow[:, :, 0]
    sy = np.arange(h, dtype=np.float32)[:, None] + scale * flow[:, :, 1]
    with np.errstate(invalid="ignore"):
        return [bool((fin & c).any()) for c in (sx < 0, sx > w - 1, sy < 0, sy > h - 1)]


def test_frames_give_no_warp_taps_and_clamped_taps(oracle):
    seen = set()
    for win, iters, lw, lh, B, waves in wt.cases():
        if (win, lw, lh) in seen:
            continue
        seen.add((win, lw, lh))
        fr = wt.frames(lw, lh, wt.seed(win, lw, lh))
        # (a flow that is not finite after iteration 1 stays so: every later iteration adds to it)
        flat = _flows_before_each_warp(oracle, fr[2], fr[3], win, 1, (0, 1))
        for k in range(wt.LEVELS):
            assert not np.isfinite(flat[k][0]).all(), f"win {win} {lw}x{lh}: flat blocks, level {k}: every flow is finite"
        noise = _flows_before_each_warp(oracle, fr[4], fr[5], win, 4, (1,))
        for j, f in enumerate(noise[1]):
            assert all(_clamped_borders(f, oracle.ITER_SCALE)), f"win {win} {lw}x{lh}: noise, after iteration {j + 1}: borders {_clamped_borders(f, oracle.ITER_SCALE)}"


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("warp_taps_plan") / "pair_plan_main")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "cuda_optical_flow_2_amd", "csrc"),
                           os.path.join(ROOT, "tools", "pair_plan_main.cpp"), "-o", exe])

    def run(out_w, overhead, capacity, items):
        args = [exe, str(out_w), str(overhead), "1", str(capacity)] + [str(v) for it in items for v in it]
        lines = subprocess.check_output(args, text=True).split("\n")
        assert lines[0].startswith("plan"), lines[0]
        return [tuple(map(int, l.split())) for l in lines[1:] if l]   # (wave, item, tile, y0, y1)
    return run


def test_wave_counts_cut_inside_tile_columns(planner):
    near_top = near_bottom = 0
    for win, iters, lw, lh, B, waves in wt.cases():
        its = wt.items(lw, lh, B)
        segs = planner(wt.TILE[win], 3 * (win // 2) + 4, waves, its)
        per_wave = {}
        for wv, item, tile, y0, y1 in segs:
            per_wave[wv] = per_wave.get(wv, 0) + 1
        cuts = [(y0, its[item][1]) for wv, item, tile, y0, y1 in segs if y0 > 0]
        assert max(per_wave.values()) == 2, f"win {win} {lw}x{lh} B {B} waves {waves}: no wave carries two segments"
        assert cuts, f"win {win} {lw}x{lh} B {B} waves {waves}: no tile column is cut"
        near_top += any(y <= 2 for y, h in cuts)
        near_bottom += any(h - y <= 2 for y, h in cuts)
    print(f"cases with a cut within two rows of a column's top: {near_top}, of its bottom: {near_bottom}")
    assert near_top >= 4 and near_bottom >= 4
