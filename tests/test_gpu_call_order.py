"""GPU: the stream contract of the stateless calls (include/ofx.h: "Device entry points only enqueue work; they never synchronise or
allocate"; host arrays are read before the call returns; a work, stats or scratch buffer needs nothing and keeps nothing), on the
recipes of tests/call_order_cases.py and the schedules of tests/call_order.py.  Every call runs on a side stream behind several
milliseconds of other work, reads inputs that hold poison before and after their window, gets descriptors that are overwritten as
soon as it returns, and is compared with its referee by the bits after one synchronisation at the very end."""
import threading

import numpy as np
import pytest

import call_order as CO
import call_order_cases as CC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    CC.L.load()
    return torch


@pytest.fixture(scope="module")
def lanes(torch):
    """the two side streams of this file"""
    return CO.Lane(torch), CO.Lane(torch)


# ---- a. in order on a caller's stream -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CC.NAMES)
def test_a_call_runs_in_order_on_the_callers_stream(torch, lanes, name):
    """every launch and memset of the call goes to `stream`: one on the null stream would read poison or be overtaken by the refill"""
    r = CC.recipe(name)
    CO.stage(torch, [r])
    snap = CO.enqueue(torch, r, lanes[0])
    torch.cuda.synchronize()
    r.check(snap)


def test_the_engine_denoises_in_order_on_the_callers_stream(torch, lanes):
    """engine.denoise_rings(reach=2) inside torch.cuda.stream(side stream), on the inputs of the row "denoise-reach2" and the schedule
    of a.: the engine takes its stream from torch's current one, enqueues two chain calls and the filter on their outputs without a
    synchronisation, and frees fwd2 and bwd2 while the filter is still pending.  Frames and stats are the recipe's, by the bits."""
    from cuda_optical_flow_2_amd import engine

    r, lane = CC.recipe("denoise-reach2"), lanes[0]
    N, w, h, sigma = CC.DENOISE
    clean = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (r.frames, r.fwd, r.bwd)]
    bufs = [torch.empty_like(c) for c in clean]

    def poison():
        bufs[0].fill_(0xEE)
        for b in bufs[1:]:
            b.fill_(CC.NAN)

    poison()
    torch.cuda.synchronize()
    with torch.cuda.stream(lane.stream):
        lane.a = CO.busy(torch, lane.a, CO.BUSY_ROUNDS)
        for b, c in zip(bufs, clean):
            b.copy_(c)
        out, stats = engine.denoise_rings(bufs[0], bufs[1], bufs[2], float(sigma), reach=2, return_stats=True)
        poison()
        got = out.clone(), stats.clone()
        del out, stats
    torch.cuda.synchronize()
    CC.same(got[0].cpu().numpy().reshape(N, h, w), r.want["frames"], "engine.denoise_rings(reach=2) on a side stream: frames")
    CC.same(got[1].cpu().numpy().reshape(N, 1, 8), r.want["stats"], "engine.denoise_rings(reach=2) on a side stream: stats")


# ---- b. the harness sees a misplaced launch -------------------------------------------------------------------------------------------
def test_a_call_on_the_null_stream_is_seen(torch, lanes):
    """the schedule of a., the call handed the null stream while its producer sits on the side stream: torch's side streams are not
    ordered against the null stream and the busy work outlasts the call, so the warp reads poison"""
    r = CC.recipe("warp-affine")
    CO.stage(torch, [r])
    snap = CO.enqueue(torch, r, lanes[0], call_stream=None, rounds=4 * CO.BUSY_ROUNDS)      # (a margin for a slow host)
    torch.cuda.synchronize()
    got = r.read(snap)
    assert any(got[k].tobytes() != r.want[k].tobytes() for k in r.want), "a call on the wrong stream went unnoticed: test a. proves nothing"


# ---- c. buffers reused ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CC.CHAINS))
def test_calls_back_to_back_on_shared_buffers(torch, lanes, name):
    """two to four calls with different parameters that share their work, stats, counter or in-place buffers, enqueued without a
    synchronisation between them: each equals its own referee (tests/test_call_order_cases.py: the referees' answers differ)"""
    chain = CC.chain(name)
    CO.stage(torch, chain)
    snaps = [CO.enqueue(torch, r, lanes[0], rounds=CO.BUSY_ROUNDS if r is chain[0] else 0) for r in chain]
    torch.cuda.synchronize()
    for r, snap in zip(chain, snaps):
        r.check(snap)


# ---- d. two calls in flight -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CC.OTHERS))
def test_two_calls_in_flight_on_two_streams(torch, lanes, name):
    a, b = CC.recipe(name), CC.other(name)
    CO.stage(torch, [a])
    CO.stage(torch, [b])
    snap_a = CO.enqueue(torch, a, lanes[0])
    snap_b = CO.enqueue(torch, b, lanes[1])
    torch.cuda.synchronize()
    a.check(snap_a)
    b.check(snap_b)


def test_two_host_threads_each_on_its_own_stream(torch, lanes):
    """a fit on one thread and a warp on the other, started together: both equal their referees, and each thread's ofx_last_error is
    its own refusal's"""
    lib = CC.L.load()
    jobs = [(CC.recipe("fit-affine"), lambda: lib.ofx_fit_motion(None, 0, None, None), b"ofx_fit_motion"),
            (CC.recipe("warp-affine"), lambda: lib.ofx_warp_affine(None, 0, None), b"ofx_warp_affine")]
    for r, _, _ in jobs:
        CO.stage(torch, [r])
    gate = threading.Barrier(2)
    out = [None, None]

    def run(i):
        r, refuse, _ = jobs[i]
        try:
            rc = refuse()
            gate.wait(timeout=60)
            snap = CO.enqueue(torch, r, lanes[i])
            gate.wait(timeout=60)
            out[i] = (rc, snap, lib.ofx_last_error())
        except BaseException as e:      # noqa: BLE001 -- reported by the main thread
            out[i] = e
            gate.abort()

    threads = [threading.Thread(target=run, args=(i,)) for i in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    torch.cuda.synchronize()
    for (r, _, word), res in zip(jobs, out):
        assert not isinstance(res, BaseException), res
        rc, snap, msg = res
        assert rc == 1 and word in msg, (r.name, rc, msg)
        r.check(snap)


# ---- e. never synchronises ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CC.NAMES)
def test_a_call_never_waits_for_its_stream(torch, lanes, name):
    """an event behind busy work that lasts at least 50 times the call's host time (both measured here) is still pending when the call
    returns"""
    r = CC.recipe(name)
    CO.stage(torch, [r])
    call, dur, rounds = CO.busy_for(torch, r, lanes[0])
    print(f"{name}: the call takes {call * 1e6:.1f} us on the host, {rounds} rounds of busy work last {dur * 1e3:.2f} ms")
    assert dur >= CO.BUSY_FACTOR * call
    before, after = CO.event_around_call(torch, r, lanes[0], rounds)
    assert not before, "busy work too short: the event had completed before the call"
    assert not after, f"{r.entry} returned only after the work in front of it on the stream had completed"


# ---- f. never allocates ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CC.NAMES)
def test_a_call_never_allocates(torch, lanes, name):
    """free device memory before and after three calls on buffers staged beforehand (one call made before the first reading); the LK
    calls among them: plans are cached by sessions, not by the stateless launches"""
    r = CC.recipe(name)
    CO.stage(torch, [r])
    with torch.cuda.stream(lanes[0].stream):
        for i in r.ins + r.loads:
            i.load()
    assert r.launch(lanes[0].ptr) == 0
    torch.cuda.synchronize()
    free = torch.cuda.mem_get_info()[0]
    for _ in range(3):
        assert r.launch(lanes[0].ptr) == 0
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free, f"{r.entry} changed the free device memory"
