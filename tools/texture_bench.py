#!/usr/bin/env python3
"""The fused texture-strength launch (ofx_texture_features) against the chain it replaces, and the selection launch.

  python tools/texture_bench.py [--turns T] [--sets S] [--size WxH] [--window W] [--items N]

4K, window 9, eight items per launch.  Three arms take turns in one process, T turns (default 24), each turn of an arm between two
events on the stream; an arm's turn works on the next of S sets of planes and outputs (default 2; one set of eight 4K planes and
their strength planes is 332 MB, more than the 256 MiB Infinity Cache, so nothing an arm reads is left over from its previous turn):
  A   the fused strength launch: ofx_texture_features on eight strength-only items, ONE launch
  B   the chain it replaces: per item ofx_lk_level_sums(p, p) (five int32 planes) and the definition's step 2 as eager torch
      pointwise operations in float64; printed with and without the pointwise part (B_sums: the eight launches alone)
  AC  ofx_texture_features with cells, cell strengths and stats (cell 16, default border): the strength and the selection launch;
      C, the selection launch alone, is AC - A per turn pair (a rocprofv3 --kernel-trace --stats run gives it directly)
Printed: microseconds per frame (median and minimum of the turns), A's share of 8 TB/s at 5 B/px (1 read + 4 written), and A / B.
Before the turns the strengths of A and B on set 0 are compared by the bits and the number of differing values is printed (the
tests are the referee of both; torch's float64 square root is the only step here that nothing else checks).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_GBS = 8000.0
BYTES_PER_PX = 5.0


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--turns", type=int, default=24)
    ap.add_argument("--sets", type=int, default=2)
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--window", type=int, default=9)
    ap.add_argument("--items", type=int, default=8)
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "texture_bench needs the GPU: nothing here is measured without one"
    from cuda_optical_flow_2_amd import engine, lib, synth

    L = lib.load()
    w, h = (int(v) for v in args.size.split("x"))
    n, win, cell = args.items, args.window, 16
    pitch = engine.pitch_for(w)
    ncx, ncy = -(-w // cell), -(-h // cell)
    st = engine._stream_ptr()
    base = torch.zeros((h, pitch), dtype=torch.uint8, device="cuda")
    base[:, :w] = torch.from_numpy(synth.smooth_pair(w, h, 0.0, 0.0, seed=5)[0]).cuda()
    sets = []
    for s in range(args.sets):
        planes = [torch.roll(base, shifts=((s * n + i) % 7, 4 * (s * n + i)), dims=(0, 1)).contiguous() for i in range(n)]
        strength = [torch.empty((h, w), dtype=torch.float32, device="cuda") for _ in range(n)]
        cells = [torch.empty((ncy, ncx, 2), dtype=torch.int32, device="cuda") for _ in range(n)]
        cs = [torch.empty((ncy, ncx), dtype=torch.float32, device="cuda") for _ in range(n)]
        stats = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
        plain = (lib.TextureDesc * n)(*[lib.TextureDesc(planes[i].data_ptr(), pitch, w, h, strength[i].data_ptr(), w, None, None, None, 0, 0, 0.0)
                                        for i in range(n)])
        full = (lib.TextureDesc * n)(*[lib.TextureDesc(planes[i].data_ptr(), pitch, w, h, strength[i].data_ptr(), w, cells[i].data_ptr(),
                                                       cs[i].data_ptr(), stats[i].data_ptr(), cell, win // 2 + 1, 0.0) for i in range(n)])
        sets.append(dict(planes=planes, strength=strength, cells=cells, cs=cs, stats=stats, plain=plain, full=full))
    sums = [torch.empty((5, h, w), dtype=torch.int32, device="cuda") for _ in range(n)]      # (1.3 GB at 4K: never cache-resident)
    chain_out = [torch.empty((h, w), dtype=torch.float32, device="cuda") for _ in range(n)]
    geom = lib.Geom.full(w, h, pitch)

    def arm_a(S):
        engine.check(L.ofx_texture_features(S["plain"], n, win, st), "ofx_texture_features")

    def arm_ac(S):
        engine.check(L.ofx_texture_features(S["full"], n, win, st), "ofx_texture_features")

    def arm_b_sums(S):
        for i in range(n):
            engine.check(L.ofx_lk_level_sums(S["planes"][i].data_ptr(), S["planes"][i].data_ptr(), C.byref(geom), win, lib.MODE_LK_FLOAT,
                                             sums[i].data_ptr(), 0, st), "ofx_lk_level_sums")

    def pointwise(i):
        sxx, syy, sxy = sums[i][0], sums[i][1], sums[i][2]
        tr, d, b = (sxx + syy).double(), (sxx - syy).double(), sxy.double()
        lam = 0.5 * (tr - torch.sqrt(d * d + 4.0 * (b * b)))
        chain_out[i].copy_(torch.where(lam > 0, lam, torch.zeros_like(lam)))

    def arm_b(S):
        arm_b_sums(S)
        for i in range(n):
            pointwise(i)

    arms = {"A": arm_a, "B": arm_b, "B_sums": arm_b_sums, "AC": arm_ac}
    # the arms compute the same thing (and every code object is loaded before a turn is timed)
    for f in arms.values():
        f(sets[0])
    torch.cuda.synchronize()
    differ = sum(int((sets[0]["strength"][i].view(torch.int32) != chain_out[i].view(torch.int32)).sum()) for i in range(n))
    times = {k: [] for k in arms}
    order = list(arms)
    for t in range(args.turns):
        S = sets[t % len(sets)]
        for k in order[t % len(order):] + order[:t % len(order)]:      # (the arms' order rotates from turn to turn)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            arms[k](S)
            b.record()
            times[k].append((a, b))
    torch.cuda.synchronize()
    us = {k: [a.elapsed_time(b) * 1e3 / n for a, b in v] for k, v in times.items()}
    us["C"] = [ac - a for ac, a in zip(us["AC"], us["A"])]
    res = {"size": [w, h], "window": win, "items_per_launch": n, "turns": args.turns, "sets": len(sets),
           "set_MB": round(n * (h * pitch + 4 * h * w) / 1e6), "values_where_fused_and_chain_differ": differ,
           "device": torch.cuda.get_device_name(0)}
    for k, v in us.items():
        res[f"us_per_frame_{k}"] = {"median": round(statistics.median(v), 2), "min": round(min(v), 2)}
    a_med, b_med, bs_med = (res[f"us_per_frame_{k}"]["median"] for k in ("A", "B", "B_sums"))
    res["A_share_of_8TBs_at_5B_per_px"] = round(BYTES_PER_PX * w * h / (HBM_GBS * 1e3) / a_med, 3)
    res["A_over_B"] = round(a_med / b_med, 3)
    res["A_over_B_sums"] = round(a_med / bs_med, 3)
    print(json.dumps(res), flush=True)
    print("\n| arm | us per frame, median | minimum |\n|---|---|---|")
    names = {"A": "A: fused strength launch", "B": "B: ofx_lk_level_sums + torch pointwise", "B_sums": "B without the pointwise part",
             "AC": "strength + selection (cell 16)", "C": "C: selection alone (AC - A)"}
    for k in ("A", "B", "B_sums", "AC", "C"):
        print(f"| {names[k]} | {res[f'us_per_frame_{k}']['median']} | {res[f'us_per_frame_{k}']['min']} |")
    print(f"\nA: {res['A_share_of_8TBs_at_5B_per_px']} of 8 TB/s at 5 B/px; A / B = {res['A_over_B']}; A / B without the pointwise part = {res['A_over_B_sums']}")


if __name__ == "__main__":
    main()
