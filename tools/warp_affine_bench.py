#!/usr/bin/env python3
"""The affine frame warp (ofx_warp_affine) beside what a user could write today, per frame.

  python tools/warp_affine_bench.py [--turns T] [--size WxH] [--out profiles/warp_affine_bench.txt]

4K frames of noise, grey and colour, warped by a small rotation about the centre (0.01 rad, scale 1.005, a shift of (3.3, -1.7) px),
replicate border.  Per channel count the arms take turns in one process, T turns (default 12), each turn of an arm between two
events on the stream; 16 distinct source and destination frames, so that a turn of W16 moves 16 frames' worth of memory:
  W1   one ofx_warp_affine call of ONE frame
  W16  one call of 16 frames; reported per frame
  G    torch on the device for one frame: affine_grid + grid_sample (bilinear, border padding) on a float32 copy of the frame and
       the conversion back to uint8 -- what a user could write today; its result is not the same bits
  C    a device-to-device copy of one frame: the 2 C bytes per pixel that a warp cannot move less than
Printed: microseconds per frame (median and minimum of the turns) and the 2 C w h bytes over the time as a share of 8 TB/s.
Nothing is asserted.
"""
import argparse
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_affine_bench.txt"))
    args = ap.parse_args()
    import math
    import torch
    import torch.nn.functional as F

    assert torch.cuda.is_available(), "warp_affine_bench needs the GPU: nothing here is measured without one"
    from cuda_optical_flow_2_amd import engine

    w, h = (int(v) for v in args.size.split("x"))
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# python tools/warp_affine_bench.py   ({torch.cuda.get_device_name(0)}; {w}x{h}; {args.turns} turns per arm, the arms taking turns; "
         f"no counters were taken)")
    c, s = 1.005 * math.cos(0.01), 1.005 * math.sin(0.01)
    cx, cy = (w - 1) / 2, (h - 1) / 2
    model = [c, -s, cx - (c * cx - s * cy) + 3.3, s, c, cy - (s * cx + c * cy) - 1.7]
    # the same map for affine_grid: normalised coordinates, align_corners=True
    theta = torch.tensor([[c, -s * (h - 1) / (w - 1), (model[2] + c * cx - s * cy - cx) / cx],
                          [s * (w - 1) / (h - 1), c, (model[5] + s * cx + c * cy - cy) / cy]], dtype=torch.float32, device="cuda")[None]
    results = []
    for ch in (1, 3):
        shape = (16, h, w) if ch == 1 else (16, h, w, 3)
        src = torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        outside = torch.zeros(16, dtype=torch.int64, device="cuda")
        items = [(src[i], dst[i], model, 1, 0, outside[i:i + 1]) for i in range(16)]

        def w1():
            engine._warp_affine_launch(items[:1])

        def w16():
            engine._warp_affine_launch(items)

        def g():
            x = src[0].reshape(h, w, ch).permute(2, 0, 1)[None].float()
            grid = F.affine_grid(theta, (1, ch, h, w), align_corners=True)
            return F.grid_sample(x, grid, mode="bilinear", padding_mode="border", align_corners=True).round().to(torch.uint8)

        def copy():
            dst[1].copy_(src[1])

        arms = {"W1": w1, "W16": w16, "G": g, "C": copy}
        for f in arms.values():
            f()
        torch.cuda.synchronize()
        # (the two routes agree to a grey level or two where both are in range: the same map, other roundings)
        diff = (g()[0].permute(1, 2, 0).reshape(dst[0].shape).int() - dst[0].int()).abs()
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
        us = {k: [a.elapsed_time(b) * 1e3 / (16 if k == "W16" else 1) for a, b in v] for k, v in times.items()}
        nbytes = 2.0 * ch * w * h
        res = {"channels": ch, "outside_px": int(outside[0].item()), "torch_vs_warp_mean_abs_diff": round(float(diff.float().mean()), 3)}
        for k, v in us.items():
            res[f"us_per_frame_{k}"] = {"median": round(statistics.median(v), 2), "min": round(min(v), 2)}
        for k in ("W1", "W16", "C"):
            res[f"{k}_share_of_8TBs"] = round(nbytes / (HBM_GBS * 1e3) / res[f"us_per_frame_{k}"]["median"], 4)
        results.append(res)
        emit(json.dumps(res))
    emit("\n| channels | W1: one frame | W16: per frame of 16 | G: torch grid_sample | C: copy of a frame | W1 share of 8 TB/s | W16 share | C share |")
    emit("|---|---|---|---|---|---|---|---|")
    for r in results:
        emit(f"| {r['channels']} | {r['us_per_frame_W1']['median']} | {r['us_per_frame_W16']['median']} | {r['us_per_frame_G']['median']} | "
             f"{r['us_per_frame_C']['median']} | {r['W1_share_of_8TBs']} | {r['W16_share_of_8TBs']} | {r['C_share_of_8TBs']} |")
    emit("(us per frame, medians)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
