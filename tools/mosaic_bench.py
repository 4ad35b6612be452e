#!/usr/bin/env python3
"""The frame mosaic (ofx_warp_mosaic) beside the perspective warp, the chain of calls it replaces, and a plain copy, per frame.

  python tools/mosaic_bench.py [--turns T] [--size WxH] [--out profiles/mosaic_bench.txt]

4K frames of noise, grey and colour, constant border.  Source 0 is seen through tools/warp_persp_bench.py's map without the zoom (a
0.01 rad rotation about the centre, a shift of a few pixels and a mild tilt); the four further sources of the shake through the same
rotation with shifts of a few tens of pixels in four directions.  Per channel count the arms take turns in one process, T turns
(default 12), each turn of an arm between two events on the stream; 16 distinct frames, and an arm named ..16 makes 16 output frames
in one call (reported per frame), frame i from the frames i, i - 1, i + 1, i - 2, i + 2 (mod 16):
  A1, A16  ofx_warp_perspective of source 0
  B1, B16  ofx_warp_mosaic with S = 1: the same pixels
  C1, C16  ofx_warp_mosaic with S = 5, with d_counts; the share of the pixels that leave source 0 is printed
  D1       the chain C1 replaces, for ONE output frame: one ofx_warp_perspective launch of the five frames and one of five all-ones
           planes, constant fill 0, then four torch.where merges in priority order (the same bytes as C1: printed)
  E        a device-to-device copy of one frame: the 2 C bytes per pixel that a warp cannot move less than
Printed: microseconds per frame (median, minimum and maximum of the turns), the 2 C w h bytes over the median as a share of 8 TB/s,
B / A and C / B.  Nothing is asserted.
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_GBS = 8000.0
SHIFTS = [(3.3, -1.7), (-41.0, 23.5), (37.25, 29.0), (-33.5, -27.75), (45.0, -38.5)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--turns", type=int, default=12)
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mosaic_bench.txt"))
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "mosaic_bench needs the GPU: nothing here is measured without one"
    from cuda_optical_flow_2_amd import engine

    w, h = (int(v) for v in args.size.split("x"))
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# python tools/mosaic_bench.py   ({torch.cuda.get_device_name(0)}; {w}x{h}; {args.turns} turns per arm, the arms taking turns; "
         f"no counters were taken)")
    c, s = math.cos(0.01), math.sin(0.01)
    cx, cy = (w - 1) / 2, (h - 1) / 2
    models = [[c, -s, cx - (c * cx - s * cy) + tx, s, c, cy - (s * cx + c * cy) + ty, 2e-6 if k == 0 else 0.0, -1.5e-6 if k == 0 else 0.0, 1.0]
              for k, (tx, ty) in enumerate(SHIFTS)]
    results = []
    for ch in (1, 3):
        shape = (16, h, w) if ch == 1 else (16, h, w, 3)
        src = torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        outside = torch.zeros(16, dtype=torch.int64, device="cuda")
        counts = torch.zeros((16, 10), dtype=torch.int64, device="cuda")
        near = lambda i: [src[(i + d) % 16] for d in (0, -1, 1, -2, 2)]
        aitems = [(src[i], dst[i], models[0], 0, 0, outside[i:i + 1]) for i in range(16)]
        bitems = [([src[i]], models[:1], dst[i], 0, 0, None, counts[i]) for i in range(16)]
        citems = [(near(i), models, dst[i], 0, 0, None, counts[i]) for i in range(16)]
        ones = torch.ones((5, h, w), dtype=torch.uint8, device="cuda")
        warped = torch.empty((5,) + tuple(src.shape[1:]), dtype=torch.uint8, device="cuda")
        masks = torch.empty((5, h, w), dtype=torch.uint8, device="cuda")
        ditems = [(near(0)[k], warped[k], models[k], 0, 0, None) for k in range(5)]
        mitems = [(ones[k], masks[k], models[k], 0, 0, None) for k in range(5)]

        def chain():
            engine._warp_launch(ditems, perspective=True)
            engine._warp_launch(mitems, perspective=True)
            out = warped[4]
            for k in (3, 2, 1, 0):
                m = masks[k] != 0
                out = torch.where(m if ch == 1 else m[..., None], warped[k], out)
            return out

        def copy():
            dst[1].copy_(src[1])

        arms = {"A1": lambda: engine._warp_launch(aitems[:1], perspective=True), "A16": lambda: engine._warp_launch(aitems, perspective=True),
                "B1": lambda: engine._mosaic_launch(bitems[:1]), "B16": lambda: engine._mosaic_launch(bitems),
                "C1": lambda: engine._mosaic_launch(citems[:1]), "C16": lambda: engine._mosaic_launch(citems), "D1": chain, "E": copy}
        for f in arms.values():
            f()
        torch.cuda.synchronize()
        arms["A1"]()
        a_frame = dst[0].clone()
        arms["B1"]()
        b_same = bool(torch.equal(dst[0], a_frame)) and int(counts[0, 9].item()) == int(outside[0].item())
        arms["C1"]()
        leave = 1.0 - float(counts[0, 0].item()) / (w * h)
        none = float(counts[0, 9].item()) / (w * h)
        d_same = bool(torch.equal(chain(), dst[0]))
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
        nbytes = 2.0 * ch * w * h
        res = {"channels": ch, "B1_equals_A1": b_same, "D1_equals_C1": d_same, "share_of_pixels_leaving_source_0": round(leave, 4),
               "share_of_pixels_no_source_covers": round(none, 5)}
        for k, v in us.items():
            res[f"us_per_frame_{k}"] = {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
        med = lambda k: res[f"us_per_frame_{k}"]["median"]
        for k in ("A1", "A16", "B1", "B16", "C1", "C16", "E"):
            res[f"{k}_share_of_8TBs"] = round(nbytes / (HBM_GBS * 1e3) / med(k), 4)
        for n in ("1", "16"):
            res[f"B{n}_over_A{n}"] = round(med("B" + n) / med("A" + n), 3)
            res[f"C{n}_over_B{n}"] = round(med("C" + n) / med("B" + n), 3)
        res["D1_over_C1"] = round(med("D1") / med("C1"), 2)
        results.append(res)
        emit(json.dumps(res))
    emit("\n| channels | A1: perspective | B1: mosaic S=1 | C1: mosaic S=5 | D1: the chain | A16 | B16 | C16 | E: copy | B16 / A16 | C16 / B16 | D1 / C1 | "
         "A16 share of 8 TB/s | B16 share | C16 share | E share | leave source 0 |")
    emit("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in results:
        m = lambda k: r[f"us_per_frame_{k}"]["median"]
        emit(f"| {r['channels']} | {m('A1')} | {m('B1')} | {m('C1')} | {m('D1')} | {m('A16')} | {m('B16')} | {m('C16')} | {m('E')} | {r['B16_over_A16']} | "
             f"{r['C16_over_B16']} | {r['D1_over_C1']} | {r['A16_share_of_8TBs']} | {r['B16_share_of_8TBs']} | {r['C16_share_of_8TBs']} | {r['E_share_of_8TBs']} | "
             f"{r['share_of_pixels_leaving_source_0']} |")
    emit("(us per frame, medians)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
