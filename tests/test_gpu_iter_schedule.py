"""A launch census of the stream pipeline's refinement iterations: the launches a session puts behind every tick are those of its
schedule (csrc/iter_plan.h), counted by kind through the session's timing events and compared with the transcription of the old
loops in tests/test_iter_plan.py; and whatever the schedule -- iterations two per launch, one per launch, or warp launches in
between -- every pair carries the bits of the pair-at-a-time path with the same number of iterations.

448x64 frames, 2 levels, window 9: level 1 is 224x32, one fused tile wide."""
import numpy as np
import pytest

from cuda_optical_flow_2_amd import synth
from conftest import assert_same
from test_iter_plan import stream_loop

pytestmark = pytest.mark.gpu

W, H, L, WIN, MODE = 448, 64, 2, 9, "lk_float"
ITERS = range(1, 7)
NF = 2 * 2 + 3   # 2 B + 3 frames for the larger B; B = 1 streams the first five
# (OFX_ITER_PAIRS, OFX_ITER_FUSED) as a session reads them when it is created; None: unset
ENVS = {"default": (None, None), "pairs0": ("0", None), "fused0": (None, "0")}


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cuda_optical_flow_2_amd import engine

    return engine


@pytest.fixture(scope="module")
def frames():
    import torch

    return [torch.from_numpy(synth.smooth_pair(W, H, 1.1 * i, -0.7 * i, seed=23)[1]).cuda() for i in range(NF)]


@pytest.fixture(scope="module")
def plain(eng, frames):
    """every pair of the frames through a pair-at-a-time session (run_flow), per iteration count: {iters: {pair: [level 0, level 1]}}"""
    import torch

    want = {}
    for iters in ITERS:
        s = eng.Session(W, H, L, WIN, MODE, iters=iters)
        s.set_frame_device(frames[0]); s.build_pyramid(); s.swap()
        want[iters] = {}
        for i in range(1, NF):
            s.set_frame_device(frames[i]); s.build_pyramid(); s.run_flow()
            torch.cuda.synchronize()
            want[iters][i] = [s.flow_host(k) for k in range(L)]
            s.swap()
        s.close()
    return want


def predicted(iters, fused, pairs, ticks):
    """launches by kind behind `ticks` ticks that have an LK stage"""
    plan = stream_loop(iters, fused, pairs)
    per_tick = {
        "stream": 1,
        # fused: one launch makes the shifted images before the tick; otherwise the first pass has it
        "shift": (1 if fused and iters > 1 else 0) + sum(q.shift for q in plan),
        "warp": sum(q.warp for q in plan),
        "lk_acc": sum(not q.wout for q in plan),
        "lk_acc_warp": sum(q.wout for q in plan),
    }
    return {k: v * ticks for k, v in per_tick.items()}


@pytest.mark.parametrize("env", list(ENVS))
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("iters", list(ITERS))
def test_launches_of_a_tick_are_the_schedule(eng, frames, plain, monkeypatch, iters, B, env):
    import torch

    for name, val in zip(("OFX_ITER_PAIRS", "OFX_ITER_FUSED"), ENVS[env]):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)
    # what ofx_session_create makes of it: fused unless switched off, two per launch from three iterations on (9x9, unsharded, fused)
    # (the rule itself: want_pairs and fused_iters in ofx_session_create, csrc/session.cpp)
    fused = iters > 1 and env != "fused0"
    pairs = fused and iters >= 3 and env != "pairs0"
    nf = 2 * B + 3
    s = eng.Session(W, H, L, WIN, MODE, iters=iters, stream_batch=B)
    s.timing(512)
    s.stream_begin()
    got, seen = {}, 0

    def snap(done):
        nonlocal seen
        if done >= 1:
            for p in range(max(seen + 1, done - B + 1), done + 1):
                got[p] = [s.flow_of(p, k)[0].cpu().numpy() for k in range(L)]
            seen = done
    for f in frames[:nf]:
        snap(s.stream_submit(f))
    while True:
        d = s.stream_drain()
        if d == -2:
            break
        snap(d)
    torch.cuda.synchronize()
    count = {kind: s.timing_read_kind(kind)[2] for kind in ("stream", "shift", "warp", "lk_acc", "lk_acc_warp")}
    s.close()
    ticks = len({p // B for p in range(1, nf)})   # pair p's LK stage runs in the tick of the pairs p // B * B ..
    print(f"iters {iters} B {B} {env}: {count}")
    assert count == predicted(iters, fused, pairs, ticks)
    assert sorted(got) == list(range(1, nf))
    for p in got:
        for k in range(L):
            assert_same(got[p][k], plain[iters][p][k], f"iters {iters} B {B} {env}: pair {p} level {k}")


@pytest.mark.parametrize("env", ["default", "fused0"])
def test_borrowed_pitch_is_required_before_the_tick(eng, frames, monkeypatch, env):
    """with iterations, borrowed frames of another pitch than the session's are refused by the call whose tick would run their LK stage,
    fused or not, and nothing of that tick is reported"""
    import torch
    from cuda_optical_flow_2_amd.lib import OfxError

    if ENVS[env][1] is not None:
        monkeypatch.setenv("OFX_ITER_FUSED", ENVS[env][1])
    wide = [torch.zeros((H, W + 64), dtype=torch.uint8, device="cuda") for _ in range(4)]
    for t, f in zip(wide, frames):
        t[:, :W] = f
    s = eng.Session(W, H, L, WIN, MODE, iters=2, borrow_frames=True)
    s.timing(64)
    s.stream_begin()
    assert [s.stream_submit(t[:, :W]) for t in wide[:3]] == [-1, -1, -1]   # (pyramid, corner: no LK stage yet)
    with pytest.raises(OfxError, match=f"need a row pitch of {W} bytes"):
        s.stream_submit(wide[3][:, :W])
    # (only a tick with an LK stage is timed: neither it nor the shift launch in front of it was enqueued)
    assert [s.timing_read_kind(kind)[2] for kind in ("stream", "shift", "warp", "lk_acc", "lk_acc_warp")] == [0] * 5
    s.close()
