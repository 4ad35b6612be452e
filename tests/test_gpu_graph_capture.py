"""GPU: the sixth clause of the stream contract (include/ofx.h, Conventions: "a device entry point may be called while its stream is
capturing") on the recipes of tests/call_order_cases.py and the capture schedule of tests/call_order.py.  Every stateless call is
recorded into a graph on a side stream (torch.cuda.graph, capture_error_mode="global"; one stream, a linear chain), between the copy
of its staged inputs and the copy of its outputs into snapshots; the host arrays it was given are overwritten as soon as it returns.
The replays are then compared with the referees by the bits, guard bytes included: with the inputs of the capture, with other device
data behind the same host arguments (call_order_cases.variant), and with the first inputs again on work and stats buffers that
nobody has touched in between -- a table uploaded at every replay, a zeroing that is no node of the graph, or a first-use copy or
query that the runtime refuses while a capture is open shows in one of them.  At the end: one pair of a session, recorded whole."""
import ctypes as C

import numpy as np
import pytest

import call_order as CO
import call_order_cases as CC
import dense_ref as D

pytestmark = pytest.mark.gpu

OFX_E_INVALID = 1


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    CC.L.load()
    return torch


@pytest.fixture(scope="module")
def lane(torch):
    """the side stream of this file: every capture, replay and live call runs on it"""
    return CO.Lane(torch)


def capture_one(torch, lane, name):
    """the recipe staged and poisoned, its variant's inputs on the device, one call recorded: nothing has run"""
    r, v = CC.recipe(name), CC.variant(name)
    CO.stage(torch, [r])
    r.stage_variant(torch, v)
    torch.cuda.synchronize()
    cap = CO.Captured(torch, [r], lane)
    assert CO.untouched(r), f"{name}: an output was written while the call was being recorded"
    assert not any(bool(s.any()) for s in cap.snaps[0].values()), f"{name}: a snapshot was written while the call was being recorded"
    return r, v, cap


# ---- a. every call can be captured, and a replay is the call -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", CC.NAMES)
def test_a_captured_call_replays_as_the_call(torch, lane, name):
    r, v, cap = capture_one(torch, lane, name)
    r.check(cap.replay()[0], f"{name}, replay 1")
    # other device data behind the same host arguments; the outputs poisoned again, 0xA5 in the work buffers
    r.check(cap.replay(before=lambda: (CO.poison(r), r.load_variant()))[0], f"{name}, replay 2 (the variant's inputs)", want=v.want)
    # the first inputs again; outputs, work and stats buffers as replay 2 left them: what is not zeroed by a node accumulates
    # (where the call leaves part of an output alone -- the feature points beyond the count -- that part keeps replay 2's)
    r.check(cap.replay(before=lambda: r.load_variant(False))[0], f"{name}, replay 3 (buffers as replay 2 left them)", want=r.want_over(v))


# ---- b. the harness discriminates ------------------------------------------------------------------------------------------------------
def test_a_replay_that_reads_nothing_anew_or_does_nothing_is_seen(torch, lane):
    r, v, cap = capture_one(torch, lane, "warp-affine")
    r.check(cap.replay()[0], "replay 1")
    got = r.read(cap.replay(before=lambda: CO.poison(r))[0])            # (the variant's inputs are NOT loaded)
    assert any(got[k].tobytes() != v.want[k].tobytes() for k in v.want), "a replay on the old inputs passed for the variant's: test a. proves nothing"
    assert not any((got[k].view(np.uint8) == CO.FILL).all() for k in got), "a replay left an output at 0x5A"
    for k, w in r.want.items():
        CC.same(got[k], w, f"replay 2 on the old inputs: {k}")
    with pytest.raises(AssertionError):
        r.check(cap.snaps[0], want=v.want)


# ---- c. chains in one graph ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CC.CHAINS))
def test_a_chain_on_shared_buffers_in_one_graph(torch, lane, name):
    """two to four calls that share their work, stats, counter or in-place buffers, recorded into ONE graph and replayed twice, the
    second time on the buffers as the first replay left them: every call of every replay equals its own referee"""
    chain = CC.chain(name)
    CO.stage(torch, chain)
    cap = CO.Captured(torch, chain, lane)
    assert all(CO.untouched(r) for r in chain)

    def clear():
        for snap in cap.snaps:
            for t in snap.values():
                t.zero_()

    for replay in (1, 2):
        snaps = cap.replay(before=clear)
        for r, snap in zip(chain, snaps):
            r.check(snap, f"{r.name}, replay {replay}")


# ---- d. capture does not disturb live work ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CC.NAMES)
def test_live_calls_after_a_capture_and_its_replays(torch, lane, name):
    """the thread's tables and argument blocks are not left in a captured state: the same call live on the same stream, then a call
    of another entry point"""
    r, v, cap = capture_one(torch, lane, name)
    r.check(cap.replay()[0], f"{name}, replay 1")
    r.check(cap.replay(before=lambda: (CO.poison(r), r.load_variant()))[0], f"{name}, replay 2", want=v.want)
    with torch.cuda.stream(lane.stream):
        CO.poison(r)
        r.load_variant(False)
    snap = CO.enqueue(torch, r, lane, rounds=0)
    names = CC.NAMES[CC.NAMES.index(name) + 1:] + CC.NAMES[:CC.NAMES.index(name)]
    o = CC.recipe(next(n for n in names if CC.recipe(n).entry != r.entry))
    torch.cuda.synchronize()
    r.check(snap, f"{name}, live after the replays")
    CO.stage(torch, [o])
    snap = CO.enqueue(torch, o, lane, rounds=0)
    torch.cuda.synchronize()
    o.check(snap, f"{o.name}, live after {name}'s capture")
    r.check(cap.replay(before=lambda: CO.poison(r))[0], f"{name}, replay 3 after the live calls")


# ---- e. a refused call inside a capture ------------------------------------------------------------------------------------------------
def test_a_refused_call_inside_a_capture_records_nothing(torch, lane):
    """ofx_warp_affine with a descriptor whose d_src is NULL returns OFX_E_INVALID "before anything is enqueued": the capture goes on,
    ends with the valid call that follows, and replays as that call"""
    lib = CC.L.load()
    r = CC.recipe("warp-affine")
    CO.stage(torch, [r])
    seen = []

    def refused():
        Desc = CC.L.WarpAffineDesc
        good = r.outs["dst0"]
        descs = (Desc * 1)(Desc(None, 64, 64, 48, good.ptr, good.pitch, 67, 45, 3, 0, 0, (C.c_double * 6)(1, 0, 0, 0, 1, 0), r.outs["outside"].slot(0)))
        seen.append((lib.ofx_warp_affine(descs, 1, lane.ptr), lib.ofx_last_error()))
        CC.wipe(descs)

    cap = CO.Captured(torch, [r], lane, also=refused)
    assert seen[0][0] == OFX_E_INVALID and b"ofx_warp_affine" in seen[0][1], seen
    assert CO.untouched(r)
    r.check(cap.replay()[0], "replay 1")
    r.check(cap.replay(before=lambda: CO.poison(r))[0], "replay 2")


# ---- a session's pair in one graph -----------------------------------------------------------------------------------------------------
SESSION = (136, 72, 3, 9)


def _pair(s, a, b, stream):
    s.set_frame_device(a, stream=stream)
    s.build_pyramid(stream=stream)
    s.swap()
    s.set_frame_device(b, stream=stream)
    s.build_pyramid(stream=stream)
    s.run_flow(stream=stream)


@pytest.mark.parametrize("iters", [1, 3])
def test_a_sessions_pair_in_one_graph(torch, lane, iters):
    """set_frame_device, build_pyramid, swap, set_frame_device, build_pyramid, run_flow on the plain single-stream path, recorded
    after one live pair (a session builds the packed plan of a shape with a blocking copy at its first use) and replayed on two other
    pairs written into the caller's two buffers: every level's flow equals a never-captured session's, by the bits"""
    from cuda_optical_flow_2_amd import engine, synth

    W, H, Lv, win = SESSION
    frames = [torch.from_numpy(np.ascontiguousarray(synth.smooth_pair(W, H, 1.5 * i, -0.75 * i)[1])).cuda() for i in range(6)]
    s, ref = (engine.Session(W, H, Lv, win, "lk_float", iters=iters) for _ in (0, 1))
    try:
        with torch.cuda.stream(lane.stream):
            _pair(s, frames[0], frames[1], lane.stream)
        torch.cuda.synchronize()
        views = [s.flow(k)[0] for k in range(Lv)]
        fa, fb = torch.zeros_like(frames[0]), torch.zeros_like(frames[0])
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=lane.stream, capture_error_mode="global"):
            _pair(s, fa, fb, lane.stream)
        torch.cuda.synchronize()
        want = []
        for a, b in ((2, 3), (5, 4)):
            _pair(ref, frames[a], frames[b], None)
            torch.cuda.synchronize()
            want.append([ref.flow(k)[0].cpu().numpy().copy() for k in range(Lv)])
        assert any(not np.array_equal(x, y) for x, y in zip(*want)), "the two pairs have the same flow"
        for (a, b), flows in zip(((2, 3), (5, 4)), want):
            with torch.cuda.stream(lane.stream):
                for v in views:
                    v.fill_(float("nan"))
                fa.copy_(frames[a])
                fb.copy_(frames[b])
                graph.replay()
            torch.cuda.synchronize()
            for k in range(Lv):
                got = views[k].cpu().numpy()
                ok = D.same_bits(got, flows[k])
                assert ok.all(), f"iters={iters}, frames {a} -> {b}, level {k}: {int((~ok).sum())}/{ok.size} values differ from the live session's"
    finally:
        s.close()
        ref.close()
