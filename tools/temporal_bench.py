#!/usr/bin/env python3
"""The temporal noise filter (ofx_temporal_filter) beside the chain of calls it replaces and a plain copy, per frame.

  python tools/temporal_bench.py [--turns T] [--size WxH] [--frames N] [--out profiles/temporal_bench.txt]

4K frames of a smooth texture plus noise, grey and colour, S = 2 neighbours (the frames before and after, mod N), fields of a few
pixels with fractions, table temporal_weights(10).  N frames (default 32) with their 2 N fields: 32 grey 4K frames and 64 fields
are 4.5 GB, far beyond the 256 MB Infinity Cache, and every launch works on frames the launches before it did not touch.  Per
channel count the arms take turns in one process, T turns (default 12), each turn of an arm between two events on the stream;
an arm named ..16 filters 16 frames in one call (reported per frame):
  F1, F16  ofx_temporal_filter without stats
  G1, G16  ofx_temporal_filter with d_stats
  H1       grey only -- the chain F1 replaces, for ONE frame: two ofx_motion_compensate launches (scale 1, no shift, no stats), each
           writing a whole plane, and a torch blend (c + a + b + 1) / 3 in int32.  It has NO patch test and another bilinear
           rounding: its bytes are not the filter's.
  E        a device-to-device copy of one frame
The descriptors of F and G are built before the timing; a one-frame arm is still ONE short launch between two events, so its time
holds the gap before the launch starts (the arms ..16 spread it over 16 frames); H1 and E go through torch inside their windows.
Printed: microseconds per frame (median, minimum and maximum of the turns) and the bytes the definition needs -- per pixel 2 * 8 of
the fields, 3 C read and C written -- over the median as a share of 8 TB/s.  Nothing is asserted.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--turns", type=int, default=12)
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_bench.txt"))
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "temporal_bench needs the GPU: nothing here is measured without one"
    from cuda_optical_flow_2_amd import engine

    w, h = (int(v) for v in args.size.split("x"))
    N = args.frames
    assert N >= 16 and N % 16 == 0
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# python tools/temporal_bench.py   ({torch.cuda.get_device_name(0)}; {w}x{h}; {N} frames; {args.turns} turns per arm, the arms "
         f"taking turns; no counters were taken)")
    L = engine._lib.load()
    prm = engine._temporal_params(10.0, 256)
    # two fields per frame: smooth, a few pixels, with fractions
    yy, xx = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float32), torch.arange(w, device="cuda", dtype=torch.float32), indexing="ij")
    fields = torch.empty((N, 2, h, w, 2), dtype=torch.float32, device="cuda")
    for i in range(N):
        for s, sign in enumerate((1.0, -1.0)):
            fields[i, s, :, :, 0] = sign * (2.3 + 0.1 * i) + 0.4 * torch.sin(xx * 0.003 + i)
            fields[i, s, :, :, 1] = sign * (-1.6) + 0.3 * torch.cos(yy * 0.004 + s)
    results = []
    for ch in (1, 3):
        base = 128 + 60 * torch.sin(xx * 0.05) * torch.cos(yy * 0.04)
        src = torch.empty((N, h, w) if ch == 1 else (N, h, w, 3), dtype=torch.uint8, device="cuda")
        for i in range(N):
            img = base if ch == 1 else base[..., None].expand(h, w, 3)
            src[i] = (img + 10.0 * torch.randn(img.shape, device="cuda")).clamp(0, 255).to(torch.uint8)
        dst = torch.empty_like(src)
        stats = torch.zeros((N, 8), dtype=torch.int64, device="cuda")
        item = lambda i, st: (src[i], [src[(i - 1) % N], src[(i + 1) % N]], [fields[i, 0], fields[i, 1]], dst[i], stats[i] if st else None)
        turn_of = {"n": 0}

        def frames(n):
            """the next n frames, so that no launch finds its inputs in the cache"""
            i0 = turn_of["n"] % N
            turn_of["n"] += n
            return [(i0 + k) % N for k in range(n)]

        mc = torch.empty((2, h, w), dtype=torch.uint8, device="cuda")

        def chain():
            i, = frames(1)
            for s, g in enumerate(((i - 1) % N, (i + 1) % N)):
                engine.check(L.ofx_motion_compensate(src[i].data_ptr(), w, src[g].data_ptr(), w, w, h, fields[i, s].data_ptr(), None, 1.0,
                                                     mc[s].data_ptr(), w, None, engine._stream_ptr()), "ofx_motion_compensate")
            dst[i] = ((src[i].to(torch.int32) + mc[0].to(torch.int32) + mc[1].to(torch.int32) + 1) // 3).to(torch.uint8)

        def copy():
            i, = frames(1)
            dst[i].copy_(src[i])

        # the descriptors of every launch are made here, outside the timed windows: a timed arm is the C call alone
        descs = {(n, st, i0): engine._temporal_descs([item((i0 + k) % N, st) for k in range(n)])
                 for n in (1, 16) for st in (False, True) for i0 in range(N)}
        byref_prm, stream = ctypes.byref(prm), engine._stream_ptr()

        def launch(n, st):
            i0 = frames(n)[0]
            engine.check(L.ofx_temporal_filter(descs[(n, st, i0)], n, byref_prm, stream), "ofx_temporal_filter")

        arms = {"F1": lambda: launch(1, False), "F16": lambda: launch(16, False), "G1": lambda: launch(1, True), "G16": lambda: launch(16, True),
                "E": copy}
        if ch == 1:
            arms["H1"] = chain
        for f in arms.values():
            f()
        torch.cuda.synchronize()
        engine._temporal_launch([item(0, True)], prm)
        st = stats[0].cpu().tolist()
        times = {k: [] for k in arms}
        order = list(arms)
        for turn in range(args.turns):
            for k in order[turn % len(order):] + order[:turn % len(order)]:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                arms[k]()
                b.record()
                times[k].append((a, b))
        torch.cuda.synchronize()
        us = {k: [a.elapsed_time(b) * 1e3 / (16 if k.endswith("16") else 1) for a, b in v] for k, v in times.items()}
        nbytes = (2 * 8 + 3 * ch + ch) * float(w * h)
        res = {"channels": ch, "bytes_per_pixel": 2 * 8 + 4 * ch, "stats_of_frame_0": st,
               "mean_weight_given": round(st[7] / (2.0 * 256 * w * h), 4)}
        for k, v in us.items():
            res[f"us_per_frame_{k}"] = {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
        med = lambda k: res[f"us_per_frame_{k}"]["median"]
        for k in ("F1", "F16", "G1", "G16"):
            res[f"{k}_share_of_8TBs"] = round(nbytes / (HBM_GBS * 1e3) / med(k), 4)
        res["E_share_of_8TBs"] = round(2.0 * ch * w * h / (HBM_GBS * 1e3) / med("E"), 4)
        if ch == 1:
            res["H1_over_F1"] = round(med("H1") / med("F1"), 2)
        results.append(res)
        emit(json.dumps(res))
        del src, dst
    emit("\n| channels | F1: filter | F16 | G1: with stats | G16 | H1: the chain | E: copy | H1 / F1 | F1 share of 8 TB/s | F16 share | G16 share | E share |")
    emit("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in results:
        m = lambda k: r[f"us_per_frame_{k}"]["median"] if f"us_per_frame_{k}" in r else "-"
        emit(f"| {r['channels']} | {m('F1')} | {m('F16')} | {m('G1')} | {m('G16')} | {m('H1')} | {m('E')} | {r.get('H1_over_F1', '-')} | "
             f"{r['F1_share_of_8TBs']} | {r['F16_share_of_8TBs']} | {r['G16_share_of_8TBs']} | {r['E_share_of_8TBs']} |")
    emit("(us per frame, medians)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
