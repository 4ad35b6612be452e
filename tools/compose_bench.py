#!/usr/bin/env python3
"""The stream pipeline's output stage (ofx_session_stream_compose), measured on its own terms.

  python tools/compose_bench.py [--steps K] [--warmup W] [--only 4k|1080p] [--trace]

1. The batched compose launch (one per completing call; HIP events of the session, timing kind "compose") against the route it
   replaces, B launches of ofx_compose_flow on the ofx_session_flow_of pointers between ticks (torch events around the B
   launches), at 4K with B = 8 and at 1080p with B = 16.  Both read flow sets the tick has just written; the frames come from a
   ring of distinct buffers larger than the Infinity Cache, as in bench.py, and one tick's flow sets plus the slots it writes
   (4K: 0.71 + 0.53 GB, 1080p: 0.36 + 0.27 GB) already exceed that cache.  Printed as us per launch and as a fraction of
   8 TB/s on the separate launch's byte floor: 8 B/px level 0 read + 8 B/px x (1/4 + 1/16 + ...) coarse levels + 8 B/px
   written (18.7 B/px at 5 levels).
2. The tick with and without the ring (wall time per tick, torch events around K ticks) at iters 1 and 5.
--trace: one short stream without and one with the ring at 1080p, printing the calls that completed pairs (for a
rocprofv3 --kernel-trace --stats run: the compose kernel must appear exactly that many times, and only in the second).
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_GBS = 8000.0
CONFIGS = {"4k": (3840, 2160, 5, 9, 8), "1080p": (1920, 1080, 4, 7, 16)}   # w, h, levels, window, B (bench.py's workloads)


def floor_bytes_per_px(levels):
    return 8 + 8 * sum(4.0 ** -k for k in range(1, levels)) + 8


def frame_ring(w, h, min_bytes=320e6):
    """distinct device frames (a texture rolled by i pixels), together larger than the 256 MB Infinity Cache"""
    import torch
    from cuda_optical_flow_2_amd import synth

    base = torch.from_numpy(synth.smooth_pair(w, h, 0.0, 0.0, seed=5)[0]).cuda()
    n = max(24, int(min_bytes // (w * h)) + 1)
    return [torch.roll(base, shifts=(i % 7, 3 * i), dims=(0, 1)).contiguous() for i in range(n)]


def run(cfg, iters, ring_on, baseline, steps, warmup, frames):
    """K ticks of the stream pipeline; returns a dict of per-tick wall us and, where measured, the compose launch us"""
    import torch
    from cuda_optical_flow_2_amd import engine, lib

    w, h, L, win, B = cfg
    s = engine.Session(w, h, L, win, "lk_float", iters=iters, stream_batch=B, borrow_frames=True, two_stage=True)
    ring = None
    if ring_on:
        ring = torch.empty((B, h, w, 2), dtype=torch.float32, device="cuda")
        s.stream_compose(ring, 0)
    s.stream_begin()
    L_ = lib.load()
    n = len(frames)
    groups = [engine.FrameGroup([frames[(j * B + k) % n] for k in range(B)]) for j in range(n)]
    base_ev = []
    dst = torch.empty((h, w, 2), dtype=torch.float32, device="cuda") if baseline else None
    ptrs = (C.c_void_p * lib.OFX_MAX_LEVELS)()

    def tick(j, timed):
        done = s.stream_submit_frames(groups[j % len(groups)])
        if baseline and done >= 1 and timed:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for p in range(done - B + 1, done + 1):
                for k in range(L):
                    ptrs[k] = s.flow_of(p, k)[0].data_ptr()
                lib.check(L_.ofx_compose_flow(ptrs, w, h, L, 0, dst.data_ptr(), engine._stream_ptr()), "ofx_compose_flow")
            e1.record()
            base_ev.append((e0, e1))

    for j in range(warmup):
        tick(j, False)
    s.timing(steps * (2 * iters + 4))
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for j in range(warmup, warmup + steps):
        tick(j, True)
    b.record()
    torch.cuda.synchronize()
    out = {"tick_us": a.elapsed_time(b) * 1e3 / steps}
    avg, mn, cnt = s.timing_read_kind("compose")
    if cnt:
        out.update(compose_us=avg, compose_min_us=mn, compose_launches=cnt)
    if base_ev:
        us = [e0.elapsed_time(e1) * 1e3 for e0, e1 in base_ev]
        out.update(baseline_us=sum(us) / len(us), baseline_min_us=min(us))
    s.close()
    return out


def trace(steps):
    import torch
    from cuda_optical_flow_2_amd import engine

    w, h, L, win, B = CONFIGS["1080p"]
    frames = frame_ring(w, h, 0)[:24]
    for ring_on in (False, True):
        s = engine.Session(w, h, L, win, "lk_float", stream_batch=B, borrow_frames=True, two_stage=True)
        ring = torch.empty((B, h, w, 2), dtype=torch.float32, device="cuda")
        if ring_on:
            s.stream_compose(ring, 0)
        s.stream_begin()
        calls = 0
        for i in range(steps):
            calls += s.stream_submit(frames[i % len(frames)]) >= 1
        while True:
            d = s.stream_drain()
            if d == -2:
                break
            calls += d >= 1
        torch.cuda.synchronize()
        s.close()
        print(json.dumps({"trace": "1080p B=16", "frames": steps, "ring": ring_on, "calls_completing_pairs": calls,
                          "compose_launches_expected": calls if ring_on else 0}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--only", choices=sorted(CONFIGS))
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available()
    if args.trace:
        trace(80)
        return
    for name, cfg in CONFIGS.items():
        if args.only and name != args.only:
            continue
        w, h, L, win, B = cfg
        frames = frame_ring(w, h)
        floor = floor_bytes_per_px(L)
        px = w * h * B
        ideal_us = px * floor / (HBM_GBS * 1e3)
        res = {"workload": name, "w": w, "h": h, "levels": L, "window": win, "B": B, "floor_B_per_px": round(floor, 2),
               "floor_us_at_8TBs": round(ideal_us, 1)}
        # 1. the batched launch (in a ring-on run) and the B x ofx_compose_flow route (in a ring-off run), iters 1
        on = run(cfg, 1, True, False, args.steps, args.warmup, frames)
        off = run(cfg, 1, False, True, args.steps, args.warmup, frames)
        res["batched_us"] = round(on["compose_us"], 1)
        res["batched_min_us"] = round(on["compose_min_us"], 1)
        res["batched_frac_of_8TBs"] = round(ideal_us / on["compose_us"], 3)
        res["batched_launches"] = on["compose_launches"]
        res["baseline_B_x_compose_flow_us"] = round(off["baseline_us"], 1)
        res["baseline_frac_of_8TBs"] = round(ideal_us / off["baseline_us"], 3)
        res["speedup_vs_baseline"] = round(off["baseline_us"] / on["compose_us"], 2)
        print(json.dumps(res), flush=True)
        # 2. the tick with and without the ring
        for iters in (1, 5):
            t_off = run(cfg, iters, False, False, args.steps, args.warmup, frames)
            t_on = run(cfg, iters, True, False, args.steps, args.warmup, frames)
            print(json.dumps({"workload": name, "B": B, "iters": iters, "tick_us_ring_off": round(t_off["tick_us"], 1),
                              "tick_us_ring_on": round(t_on["tick_us"], 1),
                              "overhead_us": round(t_on["tick_us"] - t_off["tick_us"], 1),
                              "overhead_frac": round(t_on["tick_us"] / t_off["tick_us"] - 1, 3),
                              "compose_us_in_tick": round(t_on["compose_us"], 1)}), flush=True)


if __name__ == "__main__":
    main()
