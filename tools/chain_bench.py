#!/usr/bin/env python3
"""The displacement chain's launch (ofx_displacement_chain), measured on its own terms at 4K.

  python tools/chain_bench.py [--rounds R] [--warmup W] [--size WxH] [--clip WxHxN]

Sixteen items, each with four links and a destination of its own (66 MB a field at 4K: 5.3 GB in all, twenty times the 256 MiB
Infinity Cache, so by the time a launch comes back to a field nothing of it is cached).  The links are a translation of a few
pixels plus 0.35 px of noise, its sign alternating from link to link, in pixels: the taps have the locality of a real clip and
nearly every path stays inside.  The arms take turns R times in one process, each between two HIP events:
  chain L x16        one launch of sixteen items of L = 2, 3, 4 links: 8 B/px per link read + 8 B/px written
  chain L x1         the same sixteen items, one launch each (the rotation keeps the cache cold)
  fold L x16         the L-link chain as L - 1 two-link launches through the destination, in place from the second on: what the
                     one launch replaces (24 B/px per step: 16 (L - 2) B/px more, for the intermediate field written and read back)
  consistency x16    ofx_flow_consistency_batch on links 0 and 1 of the same items, mask + stats: the same gather, 17 B/px
  grid_sample x16    the two-link chain restated in torch: a grid from link 0, grid_sample of link 1, an add (interior pixels agree
                     to rounding; it has no classes)
  copy x16           a plain copy of link 0 into the destination: 16 B/px
Printed: us per item (median and minimum over the rounds), the share of 8 TB/s the algorithmic bytes make of the median, and the
k-link launch's time over its fold's.  Then video_denoise_dense on one clip, reach 2 against reach 1, by a host clock around
calls that end in a synchronise, alternating."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_GBS = 8000.0
ITEMS, LINKS = 16, 4


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--clip", default="1920x1080x7")
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from cuda_optical_flow_2_amd import engine, lib

    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    w, h = (int(v) for v in args.size.split("x"))
    L_ = lib.load()
    vp = C.c_void_p
    st = engine._stream_ptr()
    gen = torch.Generator(device="cuda").manual_seed(11)
    links = []
    for i in range(ITEMS):
        t = torch.tensor([1.7 - 0.2 * i, -0.9 + 0.1 * i], device="cuda")
        links.append([((t if j % 2 == 0 else -t) + 0.35 * torch.randn((h, w, 2), device="cuda", generator=gen)).contiguous() for j in range(LINKS)])
    dst = [torch.empty((h, w, 2), dtype=torch.float32, device="cuda") for _ in range(ITEMS)]
    mask = [torch.empty((h, w), dtype=torch.uint8, device="cuda") for _ in range(ITEMS)]
    stats = torch.zeros((ITEMS, 4), dtype=torch.int64, device="cuda")

    def descs(L, first=0, count=ITEMS, fold_step=None):
        """count items from `first` on: their first L links, or, for step j >= 1 of a fold, (what the fold has so far, link j)"""
        d = (lib.ChainDesc * count)()
        for n, i in enumerate(range(first, first + count)):
            if fold_step is None:
                ptrs = [links[i][k].data_ptr() for k in range(L)]
            else:
                ptrs = [(links[i][0] if fold_step == 1 else dst[i]).data_ptr(), links[i][fold_step].data_ptr()]
            for k, p in enumerate(ptrs):
                d[n].d_link[k] = p
            d[n].n_links, d[n].w, d[n].h, d[n].d_dst = len(ptrs), w, h, dst[i].data_ptr()
        return d

    whole = {L: descs(L) for L in (2, 3, 4)}
    single = {L: [descs(L, i, 1) for i in range(ITEMS)] for L in (2, 3, 4)}
    steps = {j: descs(2, fold_step=j) for j in (1, 2, 3)}

    def launch(d, n):
        lib.check(L_.ofx_displacement_chain(d, n, st), "ofx_displacement_chain")

    def fold(L):
        for j in range(1, L):
            launch(steps[j], ITEMS)

    arr = lambda ts: (vp * ITEMS)(*[t.data_ptr() for t in ts])
    a_f, a_b, a_m = arr([l[0] for l in links]), arr([l[1] for l in links]), arr(mask)
    a_s = (vp * ITEMS)(*[stats.data_ptr() + 32 * i for i in range(ITEMS)])

    def consistency():
        lib.check(L_.ofx_flow_consistency_batch(a_f, a_b, ITEMS, w, h, 1.0, 0.01, 0.5, a_m, w, None, a_s, st), "ofx_flow_consistency_batch")

    ys, xs = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float32), torch.arange(w, device="cuda", dtype=torch.float32), indexing="ij")
    base = torch.stack([xs, ys], -1)
    norm = torch.tensor([2.0 / max(w - 1, 1), 2.0 / max(h - 1, 1)], device="cuda")

    def grid_sample():
        for i in range(ITEMS):
            grid = ((base + links[i][0]) * norm - 1.0)[None]
            r = F.grid_sample(links[i][1].permute(2, 0, 1)[None], grid, mode="bilinear", padding_mode="border", align_corners=True)
            torch.add(links[i][0], r[0].permute(1, 2, 0), out=dst[i])

    def copy():
        for i in range(ITEMS):
            dst[i].copy_(links[i][0])

    arms = {}
    for L in (2, 3, 4):
        arms[f"chain {L} x16"] = lambda L=L: launch(whole[L], ITEMS)
        arms[f"chain {L} x1"] = lambda L=L: [launch(d, 1) for d in single[L]]
    for L in (3, 4):
        arms[f"fold {L} x16"] = lambda L=L: fold(L)
    arms.update({"consistency x16": consistency, "grid_sample x16": grid_sample, "copy x16": copy})
    bytes_px = {f"chain {L} x{n}": 8.0 * L + 8 for L in (2, 3, 4) for n in (1, 16)}
    bytes_px.update({"fold 3 x16": 48.0, "fold 4 x16": 72.0, "consistency x16": 17.0, "grid_sample x16": 24.0, "copy x16": 16.0})

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
                times[k].append(e0.elapsed_time(e1) * 1e3 / ITEMS)
    # the classes of the four-link chain, for the record
    d = descs(4, 0, 1)
    d[0].d_stats = stats.data_ptr()
    launch(d, 1)
    torch.cuda.synchronize()
    px = w * h
    out = {"w": w, "h": h, "items": ITEMS, "rounds": args.rounds, "four_link_classes_2_3_0": [round(v / px, 4) for v in stats[0, 1:].tolist()]}
    for k, us in times.items():
        med = statistics.median(us)
        out[k] = {"us_per_item_median": round(med, 1), "us_per_item_min": round(min(us), 1), "B_per_px": bytes_px[k],
                  "frac_of_8TBs": round(px * bytes_px[k] / (HBM_GBS * 1e3) / med, 3)}
    for L in (3, 4):
        out[f"chain {L} x16"]["over_its_fold"] = round(statistics.median(times[f"chain {L} x16"]) / statistics.median(times[f"fold {L} x16"]), 3)
    print(json.dumps(out), flush=True)
    del links, dst, mask

    # one clip through video_denoise_dense, reach 2 against reach 1
    cw, ch, cn = (int(v) for v in args.clip.split("x"))
    tex = F.avg_pool2d(torch.rand((1, 1, ch + 2 * cn + 8, cw + 3 * cn + 8), device="cuda", generator=gen), 9, 1, 4)[0, 0]
    tex = 128.0 + 80.0 * (tex - tex.mean()) / (tex - tex.mean()).abs().max()         # a texture panning by (3, 2) px a frame, sigma 10 noise
    clip = torch.stack([tex[2 * f:2 * f + ch, 3 * f:3 * f + cw] for f in range(cn)])
    clip = (clip + 10.0 * torch.randn(clip.shape, device="cuda", generator=gen)).round().clamp(0, 255).to(torch.uint8)
    ms = {1: [], 2: []}
    for r in range(2 + 5):
        for reach in (1, 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            engine.video_denoise_dense(clip, 4, 9, 10.0, median=2, reach=reach)
            torch.cuda.synchronize()
            if r >= 2:
                ms[reach].append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"clip": [cn, ch, cw], "video_denoise_dense_ms_median": {f"reach {k}": round(statistics.median(v), 2) for k, v in ms.items()},
                      "reach_2_over_reach_1": round(statistics.median(ms[2]) / statistics.median(ms[1]), 3)}), flush=True)


if __name__ == "__main__":
    main()
