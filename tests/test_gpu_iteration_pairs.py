"""Refinement iterations two per launch in the stream pipeline (csrc/lk_body_pair.h): a wave carries iteration j and iteration
j + 1, the second trailing the first by R + 2 rows; the flow and the warped image between them stay in LDS.  OFX_ITER_PAIRS=0
(read when a session is created) keeps one launch per iteration: everything here is compared with that, or with the oracle, bit
for bit.

The stream pipeline takes pyramids of two levels and more whose downsampled levels have even dimensions, so the level sizes
that matter to the fused tile (232 output columns at 9x9, 240 at 7x7 and 5x5, 248 at 3x3) are those of LEVEL 1 of a frame twice
as large; level 0 runs through the same launch and is compared too."""
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
    """Frames as in test_fused_warp_of_the_next_iteration_equals_the_warp_launch: smooth texture above, noise below, and a flat
    block in every frame -- non-finite flows ("no warp"), huge finite ones (taps clamped to every border)."""
    import torch

    out = []
    for i in range(nf):
        f = synth.random_pair(w, h, seed=w + 7 * i)[i & 1]
        sm = synth.smooth_pair(w, h, 1.5 * i, -0.9 * i, seed=w)[1]
        f[: h // 2] = sm[: h // 2]
        f[h // 3: h // 3 + 40, w // 4: w // 4 + 90] = 77
        buf = torch.zeros((h, (w + 63) // 64 * 64), dtype=torch.uint8, device="cuda")[:, :w]   # (a frame's pitch is a multiple of 4)
        buf.copy_(torch.from_numpy(np.ascontiguousarray(f)))
        out.append(buf)
    return out


def _stream(eng, frames, w, h, L, win, mode, iters, B, ptrs=None, launches=None, **kw):
    """every pair's flow pyramid through a streamed session, read through flow_of; ptrs (a dict) receives the device pointers,
    launches (a dict) the number of ticks with an LK stage and of accumulating launches behind them"""
    import torch

    s = eng.Session(w, h, L, win, mode, iters=iters, stream_batch=B, **kw)
    if launches is not None:
        s.timing(512)
    s.stream_begin()
    got, seen = {}, 0

    def snap(done):
        nonlocal seen
        if done >= 1:
            for p in range(max(seen + 1, done - B + 1), done + 1):
                views = [s.flow_of(p, k)[0] for k in range(L)]
                got[p] = [v.clone() for v in views]
                if ptrs is not None:
                    ptrs[p] = [v.data_ptr() for v in views]
            seen = done
    for f in frames:
        snap(s.stream_submit(f))
    while True:
        d = s.stream_drain()
        if d == -2:
            break
        snap(d)
    torch.cuda.synchronize()
    if launches is not None:
        launches["ticks"] = s.timing_read_kind("stream")[2]
        launches["acc"] = s.timing_read_kind("lk_acc")[2] + s.timing_read_kind("lk_acc_warp")[2]
    s.close()
    assert sorted(got) == list(range(1, len(frames)))
    return {p: [t.cpu().numpy() for t in v] for p, v in got.items()}


# level-1 widths 223 / 224 / 225 (inside the 232 columns of the 9x9 tile; around the 224 it had once), 449, 517 (odd, a ragged last
# chunk), 100 (less than one tile; with level 2 at 100x5); level-1 heights 130, 259, 8 and -- three levels -- 10 and 5 (around and below the lag R + 2)
S223, S224, S225, S449, S517, S100 = (446, 260, 2), (448, 518, 2), (450, 16, 2), (898, 260, 2), (1034, 518, 2), (400, 20, 3)
CASES = [
    (S223, 9, 5, "lk_float", 1), (S223, 3, 3, "lk_float_fast", 2), (S224, 9, 4, "lk_float_fast", 2), (S224, 5, 6, "lk_float", 1),
    (S225, 9, 5, "lk_float", 8), (S225, 7, 3, "lk_float_fast", 1), (S449, 7, 5, "lk_float", 2), (S449, 9, 2, "lk_float", 1),
    (S517, 9, 6, "lk_float_fast", 1), (S517, 5, 3, "lk_float", 8), (S100, 9, 5, "lk_float_fast", 2), (S100, 3, 4, "lk_float", 8),
    (S100, 9, 6, "lk_float", 1), (S223, 11, 5, "lk_float", 2), (S449, 11, 3, "lk_float_fast", 1),
]


@pytest.mark.parametrize("size,win,iters,mode,B", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_iteration_pairs_equal_one_launch_per_iteration(eng, monkeypatch, size, win, iters, mode, B):
    """Pairs on against OFX_ITER_PAIRS=0: every pair, every level.  Windows 3..9 take the fused launch (iterations 2 and 3, 4 and 5;
    a left-over one alone), window 11 keeps today's launches; 2..6 iterations cover both parities of the flow set the tick starts
    in and the cases with and without a left-over iteration; 2 B + 3 frames leave a partial tick to the drain."""
    w, h, L = size
    frames = _frames(w, h, 2 * B + 3)
    monkeypatch.setenv("OFX_ITER_PAIRS", "0")
    want = _stream(eng, frames, w, h, L, win, mode, iters, B)
    monkeypatch.setenv("OFX_ITER_PAIRS", "1")
    n = {}
    got = _stream(eng, frames, w, h, L, win, mode, iters, B, launches=n)
    assert any(not np.isfinite(want[p][0]).all() for p in want), "the flat block was meant to produce non-finite flows"
    # the launches behind a tick: iterations 2 .. iters two at a time up to 9x9, one at a time above
    assert n["ticks"] > 0 and n["acc"] == n["ticks"] * (iters // 2 if win <= 9 else iters - 1), n
    for p in want:
        for k in range(L):
            assert_same(got[p][k], want[p][k], f"{mode} {w}x{h} win {win} iters {iters} B {B}: pair {p} level {k}")


@pytest.mark.parametrize("win", [3, 5, 7, 9])
def test_iteration_pairs_match_the_oracle(eng, oracle, monkeypatch, win):
    """One streamed configuration per window, 3 levels, 5 iterations (the tick, then two fused launches), against the restatement."""
    import torch

    w, h, L, iters = 232, 136, 3, 5
    p, n = synth.smooth_pair(w, h, 1.2, -0.8)
    monkeypatch.setenv("OFX_ITER_PAIRS", "1")
    got = _stream(eng, [torch.from_numpy(p).cuda(), torch.from_numpy(n).cuda()], w, h, L, win, "lk_float", iters, 1)   # (232 = 4 * 58)
    want = oracle.flow_pair_iter(p, n, L, win, iters)
    for k in range(L):
        assert_same(got[1][k], want[k], f"win {win}: level {k}")


def test_iteration_pairs_with_the_determinant_guard(eng, monkeypatch):
    """min_det on through the fused launches, against the same session with pairs off."""
    w, h, L = S224
    frames = _frames(w, h, 5)
    monkeypatch.setenv("OFX_ITER_PAIRS", "0")
    want = _stream(eng, frames, w, h, L, 9, "lk_float", 5, 2, min_det=5e9)
    monkeypatch.setenv("OFX_ITER_PAIRS", "1")
    got = _stream(eng, frames, w, h, L, 9, "lk_float", 5, 2, min_det=5e9)
    assert any((want[p][0] == 0).all(axis=-1).any() for p in want), "the guard was meant to zero some pixels"
    for p in want:
        for k in range(L):
            assert_same(got[p][k], want[p][k], f"guard on: pair {p} level {k}")


@pytest.mark.parametrize("iters", [3, 5])
def test_flow_of_points_at_the_same_set_with_pairs_on_and_off(eng, monkeypatch, iters):
    """A pair slot's result lies in the same flow set whether its iterations ran two per launch or one (with an odd number of
    fused launches the tick starts in the slot's second set): flow_of gives the same address, relative to the first pair's level 0,
    in both sessions and for every pair of a slot, and the result is what is read through it."""
    w, h, L, B = 448, 260, 2, 2
    frames = _frames(w, h, 2 * B + 3)
    pon, poff = {}, {}
    monkeypatch.setenv("OFX_ITER_PAIRS", "0")
    want = _stream(eng, frames, w, h, L, 9, "lk_float", iters, B, ptrs=poff)
    monkeypatch.setenv("OFX_ITER_PAIRS", "1")
    got = _stream(eng, frames, w, h, L, 9, "lk_float", iters, B, ptrs=pon)
    for p in want:
        for k in range(L):
            assert pon[p][k] - pon[1][0] == poff[p][k] - poff[1][0], f"pair {p} level {k}: another flow set"
            if p + B in pon:
                assert pon[p][k] == pon[p + B][k], f"pair {p} level {k}: the slot moved"
            assert_same(got[p][k], want[p][k], f"iters {iters}: pair {p} level {k}")
