"""The schedules of tests/test_gpu_call_order.py: a recipe of tests/call_order_cases.py on a caller's stream behind several
milliseconds of other work, its inputs valid only between the harness's copy and its refill, with no host synchronisation anywhere;
and the schedule of tests/test_gpu_graph_capture.py (Captured): the same copy, call and snapshot recorded into a graph and replayed.
Run as a program it measures, per recipe, the call's host time and the busy work the never-synchronises test puts in front of it:
    python tests/call_order.py [output file, default profiles/call_order_times.txt]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:          # (run as a program: pytest's conftest has done this)
    sys.path.insert(0, ROOT)

import call_order_cases as CC  # noqa: E402

FILL = CC.FILL
BUSY_ROUNDS = 24       # four times tests/test_gpu_ordering.py's: about 4 ms on an MI355X
BUSY_FACTOR = 50       # the busy work in front of a call that must not wait lasts at least this many times the call's host time


def busy(torch, a, rounds=BUSY_ROUNDS):
    """`rounds` matrix products of work on the current stream (tests/test_gpu_ordering.py's _busy)"""
    for _ in range(rounds):
        a = a @ a
        a = a / a.abs().max()
    return a


class Lane:
    """a side stream and the matrix its busy work runs on"""

    def __init__(self, torch):
        self.stream = torch.cuda.Stream()
        self.a = torch.rand((2048, 2048), device="cuda")

    @property
    def ptr(self):
        return self.stream.cuda_stream


def poison(r):
    """step 1: poison in the inputs, 0x5A in the outputs, 0xA5 in the work buffers"""
    for i in r.ins:
        i.fill()
    for g in r.outs.values():
        g.flat.fill_(FILL)
    for w in r.works:
        w.fill_(CC.WORK_FILL)


def stage(torch, recipes):
    """stage the recipes, each after the first on the first one's shared buffers, and poison everything"""
    for r in recipes:
        r.stage(torch, share=None if r is recipes[0] else recipes[0])
    for r in recipes:
        poison(r)
    torch.cuda.synchronize()


def enqueue(torch, r, lane, call_stream="lane", rounds=BUSY_ROUNDS):
    """steps 2 to 6 on the lane's stream, nothing waited for: busy work, the copy of the clean inputs, the call, the refill of the
    inputs with poison, clones of the outputs.  call_stream: the stream handed to the call (default: the lane's).  Returns the clones."""
    with torch.cuda.stream(lane.stream):
        if rounds:
            lane.a = busy(torch, lane.a, rounds)
        for i in r.ins + r.loads:
            i.load()
        rc = r.launch(lane.ptr if call_stream == "lane" else call_stream)
        assert rc == 0, (r.name, rc, r.lib().ofx_last_error())
        for i in r.ins:
            i.fill()
        return {k: t.clone() for k, t in r.outputs().items()}


# ---- the capture schedule of tests/test_gpu_graph_capture.py ------------------------------------------------------------------------------
class Captured:
    """A graph of one single-stream chain on the lane's stream: per recipe the load() copies of its staged clean inputs, its call on
    lane.ptr, and the copies of its outputs into the snapshot tensors `snaps`, which are allocated here, before the capture.  Nothing
    else is recorded, nothing runs while it is; `also` (a function of no arguments) is called inside the capture, before the first
    recipe.  rcs: what the calls returned."""

    def __init__(self, torch, recipes, lane, also=None):
        self.torch, self.recipes, self.lane = torch, list(recipes), lane
        self.snaps = [{k: torch.zeros_like(t) for k, t in r.outputs().items()} for r in self.recipes]
        self.graph = torch.cuda.CUDAGraph()
        self.rcs, self.errors = [], []
        torch.cuda.synchronize()
        try:
            with torch.cuda.graph(self.graph, stream=lane.stream, capture_error_mode="global"):
                if also is not None:
                    also()
                for r, snap in zip(self.recipes, self.snaps):
                    for i in r.ins + r.loads:
                        i.load()
                    rc = r.launch(lane.ptr)
                    self.rcs.append(rc)
                    self.errors.append(r.lib().ofx_last_error() if rc else b"")
                    for k, t in r.outputs().items():
                        snap[k].copy_(t)
        except RuntimeError as e:
            raise AssertionError(f"{[r.name for r in self.recipes]}: the capture failed ({e}); the calls returned {self.rcs} {self.errors}") from e
        torch.cuda.synchronize()
        assert self.rcs == [0] * len(self.recipes), (self.rcs, self.errors)

    def replay(self, before=None):
        """`before` (live work on the lane's stream), the replay behind it, one synchronisation; returns the snapshots"""
        with self.torch.cuda.stream(self.lane.stream):
            if before is not None:
                before()
            self.graph.replay()
        self.torch.cuda.synchronize()
        return self.snaps


def untouched(r):
    """whether every output of r still holds 0x5A in every byte"""
    return all(bool((g.flat == FILL).all()) for g in r.outs.values())


def call_host_time(torch, r, lane, repeats=5):
    """the median host time of the call on an idle stream, in seconds"""
    with torch.cuda.stream(lane.stream):
        for i in r.ins + r.loads:
            i.load()
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        rc = r.launch(lane.ptr)
        times.append(time.perf_counter() - t)
        assert rc == 0, (r.name, rc, r.lib().ofx_last_error())
    torch.cuda.synchronize()
    return statistics.median(times)


def busy_time(torch, lane, rounds):
    """the duration of `rounds` of busy work on the lane's idle stream, in seconds"""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(lane.stream):
        e0.record()
        lane.a = busy(torch, lane.a, rounds)
        e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3


def busy_for(torch, r, lane):
    """(call seconds, busy seconds, rounds): busy work measured to last at least BUSY_FACTOR times the call's host time"""
    call = call_host_time(torch, r, lane)
    rounds = 4 * BUSY_ROUNDS                                         # (a margin for a slow host: the factor is a minimum)
    busy_time(torch, lane, rounds)                                   # (the first products pay for the library's start)
    while True:
        dur = busy_time(torch, lane, rounds)
        if dur >= BUSY_FACTOR * call:
            return call, dur, rounds
        assert rounds < 1 << 16, f"{r.name}: {rounds} rounds of busy work last {dur} s, the call takes {call} s"
        rounds = int(rounds * max(1.5, 1.25 * BUSY_FACTOR * call / dur)) + 1


def event_around_call(torch, r, lane, rounds):
    """(done before, done after): whether an event behind `rounds` of busy work had completed before the call and when it returned"""
    torch.cuda.synchronize()
    with torch.cuda.stream(lane.stream):
        lane.a = busy(torch, lane.a, rounds)
        ev = torch.cuda.Event()
        ev.record()
        before = ev.query()
        rc = r.launch(lane.ptr)
        after = ev.query()
    torch.cuda.synchronize()
    assert rc == 0, (r.name, rc, r.lib().ofx_last_error())
    return before, after


def main(path):
    import torch

    lane = Lane(torch)
    lines = ["# per recipe of tests/call_order_cases.py: the call's host time on an idle stream (median of five), and the busy work that",
             "# tests/test_gpu_call_order.py enqueues in front of it in test_a_call_never_waits_for_its_stream (at least 50 times the call)",
             f"# device: {torch.cuda.get_device_name(0)}",
             f"{'recipe':<22} {'entry point':<34} {'call us':>9} {'busy ms':>9} {'rounds':>7} {'done before':>12} {'done after':>11}"]
    for name in CC.NAMES:
        r = CC.recipe(name)
        stage(torch, [r])
        call, dur, rounds = busy_for(torch, r, lane)
        before, after = event_around_call(torch, r, lane, rounds)
        lines.append(f"{name:<22} {r.entry:<34} {call * 1e6:>9.1f} {dur * 1e3:>9.2f} {rounds:>7d} {str(before):>12} {str(after):>11}")
        print(lines[-1], flush=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "call_order_times.txt"))
