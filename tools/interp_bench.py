#!/usr/bin/env python3
"""Frame interpolation's batched launch (ofx_interpolate_frames_batch) measured on its own terms at 4K, beside the chain of existing
calls it replaces.

  python tools/interp_bench.py [--rounds R] [--warmup W] [--size WxH] [--colour]

(--colour: the colour launch, ofx_interpolate_frames_3ch_batch, beside three grey launches and beside the split / three launches /
interleave chain; see colour() below.)

One launch interpolates eight pairs.  Every pair has its own two planes (8.3 MB each at 4K), its own two displacement fields (66 MB
each) and its own output frames: 1.2 GB of inputs per launch, more than four times the 256 MiB Infinity Cache, so by the time a
launch comes back to a field nothing of it is cached.  The fields are a translation of a few pixels plus noise and its inverse plus
noise, in pixels, so the taps have the locality of a real pair.  The arms take turns R times in one process, each between two HIP
events:
  fused T=1, 3, 7   ONE ofx_interpolate_frames_batch launch writing T in-between frames of each of the eight pairs; algorithmic
                    HBM traffic (16 + T) B/px per pair: both fields once, T bytes stored (the tap bytes come from two planes that
                    stay cached across the T passes and are not counted)
  chain             what ONE in-between frame of each of the eight pairs costs with the calls that existed before: two
                    ofx_motion_compensate launches (image only, uv = NULL, scale 1, on fields scaled beforehand -- the scaling is not
                    timed) and a torch blend of the two warped images; T frames cost T times that, each re-reading both fields
Printed: us per pair and per output frame (median and minimum over the rounds), the fraction of 8 TB/s the algorithmic bytes make
of the fused launch, and the fused launch's time over the chain's for the same T frames."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_GBS = 8000.0
PAIRS = 8
TIMES = (1, 3, 7)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--colour", action="store_true", help="the colour launch (ofx_interpolate_frames_3ch_batch) beside three grey launches")
    args = ap.parse_args()
    if args.colour:
        return colour(args)
    import numpy as np
    import torch
    from cuda_optical_flow_2_amd import engine, lib

    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    w, h = (int(v) for v in args.size.split("x"))
    L = lib.load()
    vp = C.c_void_p
    gen = torch.Generator(device="cuda").manual_seed(7)
    dab, dba, pa, pb = [], [], [], []
    for i in range(PAIRS):
        t = torch.tensor([1.7 - 0.5 * i, -0.9 + 0.3 * i], device="cuda")
        dab.append((t + 0.35 * torch.randn((h, w, 2), device="cuda", generator=gen)).contiguous())
        dba.append((-t + 0.35 * torch.randn((h, w, 2), device="cuda", generator=gen)).contiguous())
        pa.append(torch.randint(0, 256, (h, w), dtype=torch.uint8, device="cuda", generator=gen))
        pb.append(torch.randint(0, 256, (h, w), dtype=torch.uint8, device="cuda", generator=gen))
    out = [torch.empty((max(TIMES), h, w), dtype=torch.uint8, device="cuda") for _ in range(PAIRS)]
    stats = torch.zeros((PAIRS, max(TIMES), 4), dtype=torch.int64, device="cuda")
    # the chain's inputs: the two fields of t = 0.5 (Ta = -0.25 Dab + 0.25 Dba, Tb = 0.25 Dab - 0.25 Dba), made beforehand
    ta = [(-0.25 * f + 0.25 * b).contiguous() for f, b in zip(dab, dba)]
    tb = [(0.25 * f - 0.25 * b).contiguous() for f, b in zip(dab, dba)]
    wa = [torch.empty((h, w), dtype=torch.uint8, device="cuda") for _ in range(PAIRS)]
    wb = [torch.empty((h, w), dtype=torch.uint8, device="cuda") for _ in range(PAIRS)]
    mid = [torch.empty((h, w), dtype=torch.uint8, device="cuda") for _ in range(PAIRS)]

    arr = lambda ts: (vp * PAIRS)(*[t.data_ptr() for t in ts])
    a_a, a_b, a_ab, a_ba, a_o = arr(pa), arr(pb), arr(dab), arr(dba), arr(out)
    a_s = (vp * PAIRS)(*[stats.data_ptr() + 32 * max(TIMES) * i for i in range(PAIRS)])
    pitches = (C.c_int * PAIRS)(*([w] * PAIRS))
    st = engine._stream_ptr()

    def fused(T):
        t = np.array([(k + 1) / (T + 1) for k in range(T)], np.float32)
        lib.check(L.ofx_interpolate_frames_batch(a_a, pitches, a_b, pitches, PAIRS, w, h, a_ab, a_ba, t.ctypes.data_as(C.POINTER(C.c_float)), T,
                                                 a_o, w, h * w, a_s, st), "ofx_interpolate_frames_batch")

    def chain():
        for i in range(PAIRS):
            lib.check(L.ofx_motion_compensate(pa[i].data_ptr(), w, pa[i].data_ptr(), w, w, h, ta[i].data_ptr(), None, 1.0, wa[i].data_ptr(), w, None,
                                              st), "ofx_motion_compensate")
            lib.check(L.ofx_motion_compensate(pb[i].data_ptr(), w, pb[i].data_ptr(), w, w, h, tb[i].data_ptr(), None, 1.0, wb[i].data_ptr(), w, None,
                                              st), "ofx_motion_compensate")
            mid[i].copy_(torch.lerp(wa[i].float(), wb[i].float(), 0.5).add_(0.5))

    arms = {f"fused_T{T}": (lambda T=T: fused(T)) for T in TIMES}
    arms["chain_1_frame"] = chain
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
    res = {"w": w, "h": h, "pairs_per_launch": PAIRS, "rounds": args.rounds,
           "input_MB_per_launch": round(PAIRS * (16 + 2) * px / 1e6, 1)}
    chain_med = statistics.median(times["chain_1_frame"])
    res["chain_1_frame"] = {"us_per_pair_median": round(chain_med, 1), "us_per_pair_min": round(min(times["chain_1_frame"]), 1),
                            "what": "2 ofx_motion_compensate + torch blend, per output frame"}
    for T in TIMES:
        us = times[f"fused_T{T}"]
        med = statistics.median(us)
        res[f"fused_T{T}"] = {"us_per_pair_median": round(med, 1), "us_per_pair_min": round(min(us), 1),
                              "us_per_output_frame_median": round(med / T, 1), "B_per_px": 16 + T,
                              "frac_of_8TBs": round(px * (16 + T) / (HBM_GBS * 1e3) / med, 3),
                              "chain_us_per_pair_for_T_frames": round(T * chain_med, 1), "fused_over_chain": round(med / (T * chain_med), 3)}
    print(json.dumps(res), flush=True)


def colour(args):
    """--colour: eight colour pairs per launch, every pair with its own two interleaved planes (24.9 MB each at 4K), its own two
    fields (66 MB each) and its own outputs: 1.5 GB of inputs per launch.  The arms take turns in one process, each between two HIP
    events, for T = 1, 3, 7:
      fused3_T    ONE ofx_interpolate_frames_3ch_batch launch; algorithmic HBM traffic (16 + 6 + 3T) B/px per pair: both fields once,
                  both planes once, 3T bytes stored
      grey3_T     THREE ofx_interpolate_frames_batch launches on planes split beforehand (the split is not timed), into planar
                  outputs: 3 * (16 + 2 + T) B/px
      chain_T     what a user has without the colour call: torch split of both planes, the three grey launches, torch interleave"""
    import numpy as np
    import torch
    from cuda_optical_flow_2_amd import engine, lib

    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    w, h = (int(v) for v in args.size.split("x"))
    L = lib.load()
    vp = C.c_void_p
    gen = torch.Generator(device="cuda").manual_seed(7)
    Tmax = max(TIMES)
    dab, dba, pa, pb = [], [], [], []
    for i in range(PAIRS):
        t = torch.tensor([1.7 - 0.5 * i, -0.9 + 0.3 * i], device="cuda")
        dab.append((t + 0.35 * torch.randn((h, w, 2), device="cuda", generator=gen)).contiguous())
        dba.append((-t + 0.35 * torch.randn((h, w, 2), device="cuda", generator=gen)).contiguous())
        pa.append(torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device="cuda", generator=gen))
        pb.append(torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device="cuda", generator=gen))
    out3 = [torch.empty((Tmax, h, w, 3), dtype=torch.uint8, device="cuda") for _ in range(PAIRS)]
    # planar: [channel][pair], split beforehand for grey3, split anew inside chain
    sa = [[p[..., c].contiguous() for p in pa] for c in range(3)]
    sb = [[p[..., c].contiguous() for p in pb] for c in range(3)]
    so = [[torch.empty((Tmax, h, w), dtype=torch.uint8, device="cuda") for _ in range(PAIRS)] for c in range(3)]
    back = [torch.empty((Tmax, h, w, 3), dtype=torch.uint8, device="cuda") for _ in range(PAIRS)]

    arr = lambda ts: (vp * PAIRS)(*[t.data_ptr() for t in ts])
    a_ab, a_ba = arr(dab), arr(dba)
    a_a3, a_b3, a_o3 = arr(pa), arr(pb), arr(out3)
    a_so = [arr(so[c]) for c in range(3)]
    p1, p3 = (C.c_int * PAIRS)(*([w] * PAIRS)), (C.c_int * PAIRS)(*([3 * w] * PAIRS))
    st = engine._stream_ptr()
    tps = {T: np.array([(k + 1) / (T + 1) for k in range(T)], np.float32) for T in TIMES}
    fp = lambda T: tps[T].ctypes.data_as(C.POINTER(C.c_float))

    def fused3(T):
        lib.check(L.ofx_interpolate_frames_3ch_batch(a_a3, p3, a_b3, p3, PAIRS, w, h, a_ab, a_ba, fp(T), T, a_o3, 3 * w, 3 * h * w, None, st),
                  "ofx_interpolate_frames_3ch_batch")

    def grey3(T, a=None, b=None):
        for c in range(3):
            lib.check(L.ofx_interpolate_frames_batch(arr((a or sa)[c]), p1, arr((b or sb)[c]), p1, PAIRS, w, h, a_ab, a_ba, fp(T), T, a_so[c], w, h * w,
                                                     None, st), "ofx_interpolate_frames_batch")

    def chain(T):
        a = [[p[..., c].contiguous() for p in pa] for c in range(3)]
        b = [[p[..., c].contiguous() for p in pb] for c in range(3)]
        grey3(T, a, b)
        for i in range(PAIRS):
            torch.stack([so[c][i][:T] for c in range(3)], dim=3, out=back[i][:T])

    arms = {}
    for T in TIMES:
        arms[f"fused3_T{T}"] = lambda T=T: fused3(T)
        arms[f"grey3_T{T}"] = lambda T=T: grey3(T)
        arms[f"chain_T{T}"] = lambda T=T: chain(T)
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
    # the arms computed the same frames
    for i in (0, PAIRS - 1):
        fused3(Tmax)
        chain(Tmax)
        torch.cuda.synchronize()
        assert torch.equal(out3[i], back[i]), f"pair {i}: the fused launch and the chain differ"
    px = w * h
    res = {"w": w, "h": h, "pairs_per_launch": PAIRS, "rounds": args.rounds, "input_MB_per_launch": round(PAIRS * (16 + 6) * px / 1e6, 1)}
    for T in TIMES:
        med = {k: statistics.median(times[f"{k}_T{T}"]) for k in ("fused3", "grey3", "chain")}
        res[f"T{T}"] = {
            "fused3": {"us_per_pair_median": round(med["fused3"], 1), "us_per_pair_min": round(min(times[f"fused3_T{T}"]), 1),
                       "us_per_output_frame_median": round(med["fused3"] / T, 1), "B_per_px": 16 + 6 + 3 * T,
                       "frac_of_8TBs": round(px * (16 + 6 + 3 * T) / (HBM_GBS * 1e3) / med["fused3"], 3)},
            "grey3": {"us_per_pair_median": round(med["grey3"], 1), "us_per_pair_min": round(min(times[f"grey3_T{T}"]), 1),
                      "us_per_output_frame_median": round(med["grey3"] / T, 1), "B_per_px": 3 * (16 + 2 + T),
                      "frac_of_8TBs": round(px * 3 * (16 + 2 + T) / (HBM_GBS * 1e3) / med["grey3"], 3)},
            "chain": {"us_per_pair_median": round(med["chain"], 1), "us_per_pair_min": round(min(times[f"chain_T{T}"]), 1),
                      "us_per_output_frame_median": round(med["chain"] / T, 1)},
            "fused3_over_grey3": round(med["fused3"] / med["grey3"], 3), "fused3_over_chain": round(med["fused3"] / med["chain"], 3)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
