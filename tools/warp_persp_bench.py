#!/usr/bin/env python3
"""The perspective frame warp (ofx_warp_perspective) beside its affine sibling, torch, and a plain copy, per frame.

  python tools/warp_persp_bench.py [--turns T] [--size WxH] [--out profiles/warp_persp_bench.txt]

4K frames of noise, grey and colour, warped by tools/warp_affine_bench.py's small rotation about the centre with a mild tilt
added (m6 = 2e-6, m7 = -1.5e-6), replicate border.  Per channel count the arms take turns in one process, T turns (default 12),
each turn of an arm between two events on the stream; 16 distinct source and destination frames:
  P1   one ofx_warp_perspective call of ONE frame
  P16  one call of 16 frames; reported per frame
  A1   one ofx_warp_affine call of ONE frame, the same map without the tilt
  A16  the same of 16 frames; reported per frame
  G    torch on the device for one frame: a homography grid (a [h, w, 3] product and a division) + grid_sample (bilinear, border
       padding) on a float32 copy of the frame and the conversion back to uint8 -- what a user could write today; not the same bits
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_persp_bench.txt"))
    args = ap.parse_args()
    import math
    import torch
    import torch.nn.functional as F

    assert torch.cuda.is_available(), "warp_persp_bench needs the GPU: nothing here is measured without one"
    from cuda_optical_flow_2_amd import engine

    w, h = (int(v) for v in args.size.split("x"))
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# python tools/warp_persp_bench.py   ({torch.cuda.get_device_name(0)}; {w}x{h}; {args.turns} turns per arm, the arms taking turns; "
         f"no counters were taken)")
    c, s = 1.005 * math.cos(0.01), 1.005 * math.sin(0.01)
    cx, cy = (w - 1) / 2, (h - 1) / 2
    affine = [c, -s, cx - (c * cx - s * cy) + 3.3, s, c, cy - (s * cx + c * cy) - 1.7]
    model = affine + [2e-6, -1.5e-6, 1.0]
    m3 = torch.tensor(model, dtype=torch.float32, device="cuda").reshape(3, 3)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32, device="cuda"), torch.arange(w, dtype=torch.float32, device="cuda"), indexing="ij")
    pix = torch.stack([xs, ys, torch.ones_like(xs)], dim=-1)
    results = []
    for ch in (1, 3):
        shape = (16, h, w) if ch == 1 else (16, h, w, 3)
        src = torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        outside = torch.zeros(16, dtype=torch.int64, device="cuda")
        pitems = [(src[i], dst[i], model, 1, 0, outside[i:i + 1]) for i in range(16)]
        aitems = [(src[i], dst[i], affine, 1, 0, outside[i:i + 1]) for i in range(16)]

        def g():
            x = src[0].reshape(h, w, ch).permute(2, 0, 1)[None].float()
            t = pix @ m3.T
            grid = torch.stack([t[..., 0] / t[..., 2] / cx - 1.0, t[..., 1] / t[..., 2] / cy - 1.0], dim=-1)[None]
            return F.grid_sample(x, grid, mode="bilinear", padding_mode="border", align_corners=True).round().to(torch.uint8)

        def copy():
            dst[1].copy_(src[1])

        arms = {"P1": lambda: engine._warp_launch(pitems[:1], perspective=True), "P16": lambda: engine._warp_launch(pitems, perspective=True),
                "A1": lambda: engine._warp_launch(aitems[:1]), "A16": lambda: engine._warp_launch(aitems), "G": g, "C": copy}
        for f in arms.values():
            f()
        torch.cuda.synchronize()
        arms["P1"]()
        # (the two routes agree to a grey level or two where both are in range: the same map, other roundings)
        diff = (g()[0].permute(1, 2, 0).reshape(dst[0].shape).int() - dst[0].int()).abs()
        n_out = int(outside[0].item())
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
        res = {"channels": ch, "outside_px": n_out, "torch_vs_warp_mean_abs_diff": round(float(diff.float().mean()), 3)}
        for k, v in us.items():
            res[f"us_per_frame_{k}"] = {"median": round(statistics.median(v), 2), "min": round(min(v), 2)}
        for k in ("P1", "P16", "A1", "A16", "C"):
            res[f"{k}_share_of_8TBs"] = round(nbytes / (HBM_GBS * 1e3) / res[f"us_per_frame_{k}"]["median"], 4)
        results.append(res)
        emit(json.dumps(res))
    emit("\n| channels | P1: one frame | P16: per frame of 16 | A1: affine, one frame | A16: affine, per frame of 16 | G: torch grid_sample | C: copy of a frame | "
         "P1 share of 8 TB/s | P16 share | A16 share | C share |")
    emit("|---|---|---|---|---|---|---|---|---|---|---|")
    for r in results:
        emit(f"| {r['channels']} | {r['us_per_frame_P1']['median']} | {r['us_per_frame_P16']['median']} | {r['us_per_frame_A1']['median']} | "
             f"{r['us_per_frame_A16']['median']} | {r['us_per_frame_G']['median']} | {r['us_per_frame_C']['median']} | {r['P1_share_of_8TBs']} | "
             f"{r['P16_share_of_8TBs']} | {r['A16_share_of_8TBs']} | {r['C_share_of_8TBs']} |")
    emit("(us per frame, medians)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
