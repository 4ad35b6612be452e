#!/usr/bin/env python3
"""The forward-backward check's batched launch (ofx_flow_consistency_batch), measured on its own terms at 4K level 0.

  python tools/consistency_bench.py [--rounds R] [--warmup W] [--size WxH]

One launch checks eight pairs.  Every pair has its own fwd and bwd field (66 MB each at 4K: 1.06 GB per launch, four times the
256 MiB Infinity Cache, so by the time a launch comes back to a field nothing of it is cached) and its own outputs.  The fields
are a translation of a few pixels plus noise and its inverse plus noise, in OFX_ITER_SCALE units, so the taps have the locality
and the classes the mix of a real pair.  Three arms take turns R times in one process, each between two HIP events:
  mask + stats        17 B/px algorithmic (8 fwd + 8 bwd read once + 1 written)
  mask + err + stats  21 B/px
  compose             eight ofx_compose_flow launches of a 5-level pyramid into eight fields: what making ONE of the two fields a
                      pair's check reads costs (18.7 B/px)
Printed: us per pair (median and minimum over the rounds), the fraction of 8 TB/s the algorithmic bytes make of it, and the
check's time over that of composing the two fields it reads."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_GBS = 8000.0
PAIRS, LEVELS = 8, 5


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", default="3840x2160")
    args = ap.parse_args()
    import torch
    from cuda_optical_flow_2_amd import engine, lib

    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    w, h = (int(v) for v in args.size.split("x"))
    L = lib.load()
    vp = C.c_void_p
    scale = engine.ITER_SCALE
    gen = torch.Generator(device="cuda").manual_seed(7)
    fwd, bwd = [], []
    for i in range(PAIRS):
        t = torch.tensor([1.7 - 0.5 * i, -0.9 + 0.3 * i], device="cuda")
        fwd.append(((t + 0.35 * torch.randn((h, w, 2), device="cuda", generator=gen)) / scale).contiguous())
        bwd.append(((-t + 0.35 * torch.randn((h, w, 2), device="cuda", generator=gen)) / scale).contiguous())
    mask = [torch.empty((h, w), dtype=torch.uint8, device="cuda") for _ in range(PAIRS)]
    err = [torch.empty((h, w), dtype=torch.float32, device="cuda") for _ in range(PAIRS)]
    stats = torch.zeros((PAIRS, 4), dtype=torch.int64, device="cuda")
    # the compose arm: eight 5-level pyramids and eight destinations
    pyr = [[torch.randn((h >> k, w >> k, 2), device="cuda", generator=gen) for k in range(LEVELS)] for _ in range(PAIRS)]
    dst = [torch.empty((h, w, 2), dtype=torch.float32, device="cuda") for _ in range(PAIRS)]
    lv = [(vp * lib.OFX_MAX_LEVELS)(*[t.data_ptr() for t in p]) for p in pyr]

    arr = lambda ts: (vp * PAIRS)(*[t.data_ptr() for t in ts])
    a_f, a_b, a_m, a_e = arr(fwd), arr(bwd), arr(mask), arr(err)
    a_s = (vp * PAIRS)(*[stats.data_ptr() + 32 * i for i in range(PAIRS)])
    beta = engine._beta(0.5, scale)
    st = engine._stream_ptr()

    def check(with_err):
        lib.check(L.ofx_flow_consistency_batch(a_f, a_b, PAIRS, w, h, scale, 0.01, beta, a_m, w, a_e if with_err else None, a_s, st),
                  "ofx_flow_consistency_batch")

    def compose():
        for i in range(PAIRS):
            lib.check(L.ofx_compose_flow(lv[i], w, h, LEVELS, 0, dst[i].data_ptr(), st), "ofx_compose_flow")

    arms = {"mask+stats": lambda: check(False), "mask+err+stats": lambda: check(True), "compose": compose}
    times = {k: [] for k in arms}
    for r in range(args.warmup + args.rounds):
        evs = {}
        for k, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            evs[k] = (e0, e1)
        torch.cuda.synchronize()
        if r >= args.warmup:
            for k, (e0, e1) in evs.items():
                times[k].append(e0.elapsed_time(e1) * 1e3 / PAIRS)
    px = w * h
    share = (stats[:, 1:].sum(dim=0).double() / stats[:, 0].sum().double()).tolist()
    bytes_px = {"mask+stats": 17.0, "mask+err+stats": 21.0, "compose": 8 + 8 * sum(4.0 ** -k for k in range(1, LEVELS)) + 8}
    out = {"w": w, "h": h, "pairs_per_launch": PAIRS, "rounds": args.rounds,
           "class_shares_1_2_3": [round(v, 4) for v in share]}
    for k, us in times.items():
        med = statistics.median(us)
        out[k] = {"us_per_pair_median": round(med, 1), "us_per_pair_min": round(min(us), 1), "B_per_px": round(bytes_px[k], 2),
                  "frac_of_8TBs": round(px * bytes_px[k] / (HBM_GBS * 1e3) / med, 3)}
    for k in ("mask+stats", "mask+err+stats"):
        out[k]["over_composing_its_two_fields"] = round(statistics.median(times[k]) / (2 * statistics.median(times["compose"])), 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
