"""GPU: the arena of real sessions lies where the function that used to lay it out put it.  Sessions of every kind of layout are
created at 64x48, 3 levels, window 5 -- the smallest shape at which every part exists: the patch is clipped to the frame, leaves
16x12 at the coarsest level, and the repair's room rule holds -- and the pointers the ABI hands out (ofx_session_plane,
ofx_session_flow, ofx_session_flow_of for every pair slot, the shift vectors) are compared, by their differences, with the offsets
of the transcription in tests/session_layout_ref.py; then B + 3 frames through the session give the bits of the pair-at-a-time
sequence.  What these accessors do not show (the second flow sets, the patch planes, the status words) is left to
tests/test_session_plan.py."""
import numpy as np
import pytest

import session_layout_ref as ref
from conftest import assert_same
from cuda_optical_flow_2_amd import synth
from stream_helpers import plain_sequence, stream_all_pairs

pytestmark = pytest.mark.gpu

W, H, L, WIN = 64, 48, 3, 5

# (name, what engine.Session gets, ranks of a sharded session (0: unsharded), the environment)
CASES = [("plain", dict(), 0, {}),
         ("three_stages_batch4", dict(stream_batch=4), 0, {}),
         ("two_stage_batch2", dict(stream_batch=2, borrow_frames=True, two_stage=True), 0, {}),
         ("sharded_local_corner_iters3", dict(local_corner=True, iters=3), 2, {}),
         ("iters5_two_per_launch", dict(iters=5, stream_batch=2), 0, {}),
         ("iters5_one_per_launch", dict(iters=5, stream_batch=2), 0, {"OFX_ITER_PAIRS": 0})]


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cuda_optical_flow_2_amd import engine

    return engine


@pytest.fixture(scope="module")
def sequences(eng):
    """Seven frames (B + 3 for the largest B here) and the pair-at-a-time flows of their pairs per iteration count, made once."""
    import torch

    frames = [torch.from_numpy(synth.smooth_pair(W, H, 0.5 * i, -0.25 * i, seed=5)[1]).cuda() for i in range(7)]
    return frames, {iters: plain_sequence(eng, frames, W, H, L, WIN, iters=iters) for iters in (1, 3, 5)}


def params_of(kw, shard):
    """The ofx_params engine.Session makes of its arguments, as the transcription takes them."""
    p = dict(width=W, height=H, levels=L, window=WIN, mode=ref.MODE_LK_FLOAT, iters=kw.get("iters", 1), stream_batch=kw.get("stream_batch", 1),
             borrow_frames=int(kw.get("borrow_frames", False)), stream_two_stage=int(kw.get("two_stage", False)),
             local_corner=int(kw.get("local_corner", False)))
    if shard is not None:
        p.update(sharded=1, own_y0=[r[0] for r in shard.own], own_y1=[r[1] for r in shard.own], buf_y0=[r[0] for r in shard.buf],
                 buf_y1=[r[1] for r in shard.buf], comp_y0=[r[0] for r in shard.comp], comp_y1=[r[1] for r in shard.comp])
    return p


@pytest.mark.parametrize("name,kw,ranks,env", CASES, ids=[c[0] for c in CASES])
def test_pointers_lie_at_the_transcribed_offsets_and_the_stream_keeps_its_bits(eng, sequences, monkeypatch, name, kw, ranks, env):
    from cuda_optical_flow_2_amd.parallel import ShardPlan

    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    frames, plain = sequences
    iters, B = kw.get("iters", 1), kw.get("stream_batch", 1)
    frames = frames[:B + 3]
    got = []
    for r in range(max(ranks, 1)):
        shard = ShardPlan(W, H, L, WIN, r, ranks, iters=iters) if ranks else None
        want = ref.layout(params_of(kw, shard), env)
        s = eng.Session(W, H, L, WIN, "lk_float", shard=shard, **kw)
        # a fresh session: plane 0 / 1 / 2 are image sets 0 and 1 and the first shifted set, its flow is flow set 0, its shift vectors slot 0
        seen = {}   # what the ABI hands out -> (device address, byte offset in the transcription)
        for k in range(L):
            own = (want["own0"][k] - want["fl0"][k]) * want["w"][k] * 2 * 4   # bytes from a flow set's first row to the own rows
            for which, (set_name, t) in enumerate([("img", 0), ("img", 1), ("sh", 0)]):
                view, g = s.plane(which, k)
                assert (g.w, g.h, g.pitch, g.row0, g.rows) == (want["w"][k], want["h"][k], want["pitch"][k], want["buf0"][k], want["buf1"][k] - want["buf0"][k])
                seen["plane", which, k] = (view.data_ptr(), want["at"][set_name, t, 0, k])
            view, row0 = s.flow(k)
            assert (row0, view.shape[0]) == (want["own0"][k], want["own1"][k] - want["own0"][k])
            seen["flow", 0, k] = (view.data_ptr(), want["at"]["flowset", 0, 0, k] + own)
        seen["uv", 0, 0] = (s.uv(0).data_ptr(), want["at"]["uv", 0, 0, 0])
        ptrs = {}
        got.append(stream_all_pairs(s, frames, L, B, ptrs))
        assert s.corner_status() == 0
        assert {p % B for p, _ in ptrs} == set(range(B))   # every pair slot
        for (p, k), ptr in ptrs.items():
            own = (want["own0"][k] - want["fl0"][k]) * want["w"][k] * 2 * 4
            seen["flow_of", p, k] = (ptr, want["at"]["flowset", p % B, 0, k] + own)
        s.close()
        base_ptr, base_off = seen["plane", 0, 0]
        assert base_off == 0
        for what, (ptr, off) in seen.items():   # (differences to one pointer: every pairwise difference follows)
            assert ptr - base_ptr == off - base_off, (name, r, what)
    for p in range(1, len(frames)):
        for k in range(L):
            full = np.concatenate([g[p][k] for g in got], axis=0)
            assert_same(full, plain[iters][p][k], f"{name}: pair {p} level {k}")
