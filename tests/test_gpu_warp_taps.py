"""The paths of the fused iteration march that were restructured so that the warp's tap loads stay in flight (csrc/lk_body_pair.h
`landed`): the steps that emit nothing, the second march's priming and the first one's drain wait for their own loads, so that the
joins behind them no longer wait for everything -- and a wait that is missing there would show as a row unpacked before it
arrived, i.e. as wrong flows at the top of a strip, behind a cut, or where a short level ends.  The tick's LK stage (iteration 1 plus
the warp) runs in front of every fused launch here and is compared with them.

Every case streams six frames (two of smooth texture, two with flat blocks, two of uniform noise: warp_taps_cases.py, whose sizes,
heights and wave counts are explained there; test_warp_taps_frames.py checks on the CPU what they provoke) through a session with
one launch per iteration (OFX_ITER_PAIRS=0) and through one with the fused launches, OFX_PAIR_WAVES so small that waves carry two
segments and OFX_LK_MIN_STRIP=1 so that cuts may fall next to a level's top and bottom, and compares every pair and level bit for bit,
NaN equal to NaN.  One configuration per window is compared with the oracle's lk_iter_level as well.

The issue behind this file gives the heights as "at level 0"; a level that is downsampled must have even dimensions, so 11, 17 and 33
can only be heights of level 1, like the widths (231 is level 1 of a frame 462 wide), and that is what the cases use: level 0 has
twice the rows and runs through the same launches."""
import numpy as np
import pytest

import warp_taps_cases as wt
from conftest import assert_same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cuda_optical_flow_2_amd import engine

    return engine


def _device_frames(host):
    import torch

    out = []
    for f in host:
        h, w = f.shape
        buf = torch.zeros((h, (w + 63) // 64 * 64), dtype=torch.uint8, device="cuda")[:, :w]   # (a frame's pitch is a multiple of 4)
        buf.copy_(torch.from_numpy(f))
        out.append(buf)
    return out


def _stream(eng, frames, w, h, L, win, iters, B):
    """every pair's flow pyramid through a streamed session"""
    import torch

    s = eng.Session(w, h, L, win, "lk_float", iters=iters, stream_batch=B)
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


def _id(c):
    win, iters, lw, lh, B, waves = c
    return f"win{win}-it{iters}-{lw}x{lh}-B{B}-waves{waves}"


@pytest.mark.parametrize("case", wt.cases(), ids=_id)
def test_fused_launches_equal_one_launch_per_iteration(eng, monkeypatch, case):
    win, iters, lw, lh, B, waves = case
    w, h, L = lw << (wt.LEVELS - 1), lh << (wt.LEVELS - 1), wt.LEVELS
    frames = _device_frames(wt.frames(lw, lh, wt.seed(win, lw, lh)))
    monkeypatch.setenv("OFX_ITER_PAIRS", "0")
    want = _stream(eng, frames, w, h, L, win, iters, B)
    monkeypatch.setenv("OFX_ITER_PAIRS", "1")
    monkeypatch.setenv("OFX_PAIR_WAVES", str(waves))
    monkeypatch.setenv("OFX_LK_MIN_STRIP", "1")
    got = _stream(eng, frames, w, h, L, win, iters, B)
    assert not np.isfinite(want[3][1]).all(), "the flat blocks were meant to give non-finite flows"
    for p in want:
        for k in range(L):
            assert_same(got[p][k], want[p][k], f"{_id(case)}: pair {p} level {k}")


# per window the case with 5 iterations (both fused forms) and the tile-wide level; the heights differ (33, 12, 70, 17)
ORACLE = [c for c in wt.cases() if c[1] == 5 and c[2] == wt.TILE[c[0]]]


@pytest.mark.parametrize("case", ORACLE, ids=_id)
def test_fused_launches_match_the_oracle(eng, oracle, monkeypatch, case):
    win, iters, lw, lh, B, waves = case
    w, h, L = lw << (wt.LEVELS - 1), lh << (wt.LEVELS - 1), wt.LEVELS
    host = wt.frames(lw, lh, wt.seed(win, lw, lh))
    monkeypatch.setenv("OFX_ITER_PAIRS", "1")
    monkeypatch.setenv("OFX_PAIR_WAVES", str(waves))
    monkeypatch.setenv("OFX_LK_MIN_STRIP", "1")
    got = _stream(eng, _device_frames(host), w, h, L, win, iters, B)
    for p in (1, 3, 5):   # the smooth, the flat-block and the noise pair
        want = oracle.flow_pair_iter(host[p - 1], host[p], L, win, iters)
        for k in range(L):
            assert_same(got[p][k], want[k], f"{_id(case)}: pair {p} level {k}")
