"""The fused two-iteration launch hands 1/det from its first march to its second (csrc/lk_body_pair.h, csrc/lk_solve.h): march B
emits an output row R + 2 joint steps after march A did, and takes the reciprocal of the row's determinants out of a register delay
line instead of computing it again.  The delay line is made of slots that rotate with the three-fold unrolled body (a delay of 3 or
6 steps) and, where R + 2 is no multiple of 3, a shift chain behind them: 3x3 -> 3 + 0, 5x5 -> 3 + 1, 7x7 -> 3 + 2, 9x9 -> 6 + 0.

Every case compares a stream session with OFX_ITER_PAIRS=1 against OFX_ITER_PAIRS=0 (one launch per iteration: no delay line), every
pair, every level, bit for bit, NaN equal to NaN.  test_gpu_iteration_pairs.py and test_gpu_pair_packing.py make the same comparison
at the sizes that matter to the tile and the plan; the sizes here are chosen for the delay line:

  * level heights below, at and just above the lag and its multiples (5, 6, 7, 11, 12, 13, 18) and one of 40 rows;
  * singular windows (det == 0: 1/det = +-Inf, NaN flows) in runs of more rows than the line is deep, so that every stage of it
    holds one at the same time;
  * waves that march two segments of different items, the second of which must not see the first one's line;
  * both solves, 3 / 4 / 5 iterations (fused launches with and without the warped image of the next iteration).

As in those files the stream pipeline halves even sizes, so a level-1 width of 231 is level 1 of a frame 462 wide."""
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
    """The frames of test_gpu_iteration_pairs.py (smooth texture above, noise below, a flat block of 40 x 90 from a third of the
    height down: non-finite flows in runs of many rows), and on top of them flat 16 x 16 blocks -- one across the 232-column tile
    seam, one in the top right corner -- and a single flat row and column."""
    import torch

    out = []
    for i in range(nf):
        f = synth.random_pair(w, h, seed=w + 7 * i)[i & 1]
        sm = synth.smooth_pair(w, h, 1.5 * i, -0.9 * i, seed=w)[1]
        f[: h // 2] = sm[: h // 2]
        f[h // 3: h // 3 + 40, w // 4: w // 4 + 90] = 77
        y0 = max(0, (h - 16) // 2)
        f[y0: y0 + 16, 224: 240] = 140
        f[:16, w - 16:] = 30
        f[h // 2, :] = 200
        f[:, w // 2 + 40] = 9
        buf = torch.zeros((h, (w + 63) // 64 * 64), dtype=torch.uint8, device="cuda")[:, :w]   # (a frame's pitch is a multiple of 4)
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


def _longest_nonfinite_run(flow):
    """the longest run of consecutive rows, in one column, whose flow is not finite"""
    bad = ~np.isfinite(flow).all(axis=-1)
    best = run = np.zeros(bad.shape[1], dtype=np.int64)
    for row in bad:
        run = np.where(row, run + 1, 0)
        best = np.maximum(best, run)
    return int(best.max())


def _pairs_on_and_off(eng, monkeypatch, size, win, iters, mode, B, waves=0, singular_rows=0):
    w, h, L = size
    frames = _frames(w, h, 2 * B + 1)   # a full tick and a partial one
    monkeypatch.setenv("OFX_ITER_PAIRS", "0")
    want = _stream(eng, frames, w, h, L, win, mode, iters, B)
    monkeypatch.setenv("OFX_ITER_PAIRS", "1")
    if waves:
        monkeypatch.setenv("OFX_PAIR_WAVES", str(waves))
    got = _stream(eng, frames, w, h, L, win, mode, iters, B)
    if singular_rows:
        runs = [_longest_nonfinite_run(want[p][0]) for p in want]
        print(f"longest run of non-finite rows per pair, level 0: {runs}")
        assert max(runs) >= singular_rows, f"the flat blocks were meant to give {singular_rows} singular rows in a column: {runs}"
    what = f"{mode} {w}x{h} win {win} iters {iters} B {B} waves {waves}"
    for p in want:
        for k in range(L):
            assert_same(got[p][k], want[p][k], f"{what}: pair {p} level {k}")


def _id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


# level heights: 20 / 10 / 5, 28 / 14 / 7, 44 / 22 / 11, 24 / 12 / 6, 52 / 26 / 13, 36 / 18, 40 / 20.  A segment of r rows emits in
# r steps after 3R + 4 of priming and lag, so a height below R + 2 is over before the delay line has gone round once, one of 6 or 7
# at 9x9 just as it does, 12 / 13 / 18 after two and three trips, 40 after many.
# level widths: 9x9 (232-column tile) 231 / 232 / 233, 470 (two tiles and six columns) and 480, whose middle tile is an interior one
# (no column masks); 7x7 and 5x5 (240 columns) 239 / 240 / 241 and 496 (interior); 3x3 (248 columns) 247 / 248 / 249 and 500.
SHAPES = [
    ((464, 20, 3), 9, 5, "lk_float", 1), ((464, 28, 3), 9, 3, "lk_float_fast", 2), ((464, 44, 3), 9, 4, "lk_float", 1),
    ((464, 24, 3), 9, 5, "lk_float_fast", 1), ((464, 52, 3), 9, 3, "lk_float", 2), ((462, 36, 2), 9, 5, "lk_float", 1),
    ((466, 40, 2), 9, 4, "lk_float_fast", 1), ((470, 40, 2), 9, 5, "lk_float_fast", 1), ((480, 26, 2), 9, 5, "lk_float", 1),
    ((480, 28, 3), 7, 5, "lk_float", 1), ((478, 24, 2), 7, 3, "lk_float_fast", 1), ((482, 36, 2), 7, 4, "lk_float", 2),
    ((496, 20, 3), 7, 5, "lk_float_fast", 1), ((480, 28, 3), 5, 5, "lk_float", 1), ((496, 24, 3), 5, 3, "lk_float_fast", 1),
    ((494, 20, 2), 3, 5, "lk_float", 1), ((496, 28, 3), 3, 3, "lk_float_fast", 2), ((498, 24, 2), 3, 4, "lk_float", 1),
    ((500, 20, 3), 3, 5, "lk_float_fast", 1),
]


@pytest.mark.parametrize("size,win,iters,mode,B", SHAPES, ids=_id)
def test_heights_and_widths_around_the_delay_line(eng, monkeypatch, size, win, iters, mode, B):
    _pairs_on_and_off(eng, monkeypatch, size, win, iters, mode, B)


# 464 x 40: the 40 x 90 block covers rows 13 .. 39 of level 0, so a 9x9 window (11 rows with its derivatives) is flat on some 17
# rows of a column: more than the 6 steps of the line and the fresh value together (7 rows).
@pytest.mark.parametrize("iters", [3, 4, 5])
@pytest.mark.parametrize("mode", ["lk_float", "lk_float_fast"])
def test_singular_pixels_through_every_stage(eng, monkeypatch, mode, iters):
    """Three iterations: one fused launch with the warped image of none; four: one with it and a single launch; five: both."""
    _pairs_on_and_off(eng, monkeypatch, (464, 40, 2), 9, iters, mode, 1, singular_rows=7)


# 300 x 64, three levels: 2 + 1 + 1 tile columns per pair.  B = 2 with 5 waves and B = 1 with 3: every wave marches two segments, of
# different tile columns, levels and pairs, so the second segment's first rows follow another item's last ones in the same registers.
STRADDLE = [
    ((300, 64, 3), 9, 5, "lk_float", 2, 5), ((300, 64, 3), 9, 4, "lk_float_fast", 1, 3), ((300, 64, 3), 7, 5, "lk_float_fast", 2, 5),
    ((300, 64, 3), 5, 3, "lk_float", 1, 3), ((300, 64, 3), 3, 5, "lk_float", 2, 5),
]


@pytest.mark.parametrize("size,win,iters,mode,B,waves", STRADDLE, ids=_id)
def test_a_segment_does_not_see_the_line_of_the_one_before(eng, monkeypatch, size, win, iters, mode, B, waves):
    _pairs_on_and_off(eng, monkeypatch, size, win, iters, mode, B, waves=waves, singular_rows=7)


def test_shared_reciprocal_matches_the_oracle(eng, oracle, monkeypatch):
    """9x9 at 96 x 64, three levels, five iterations (two fused launches), against the restatement."""
    import torch

    w, h, L, iters = 96, 64, 3, 5
    p, n = synth.smooth_pair(w, h, 1.2, -0.8)
    monkeypatch.setenv("OFX_ITER_PAIRS", "1")
    got = _stream(eng, [torch.from_numpy(p).cuda(), torch.from_numpy(n).cuda()], w, h, L, 9, "lk_float", iters, 1)
    want = oracle.flow_pair_iter(p, n, L, 9, iters)
    for k in range(L):
        assert_same(got[1][k], want[k], f"level {k}: ")
