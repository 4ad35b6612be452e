#!/usr/bin/env python3
"""The camera-motion fit (ofx_fit_motion) beside what a user could write today, per pair.

  python tools/fit_motion_bench.py [--turns T] [--matches 1024,16384,262144] [--hypotheses 256,1024] [--out profiles/fit_motion_bench.txt]

Synthetic matches of a similarity in a 3840 x 2160 frame: 0.05 px noise, 40 % uniform outliers, 10 % unusable; similarity model,
radius 1 px, two refits.  Per (n, H) the arms take turns in one process, T turns (default 12), each turn of an arm between two
events on the stream:
  F1   one ofx_fit_motion call of ONE item
  F16  one call of 16 items (16 copies of the matches in buffers of their own); reported per item
  T    a torch restatement of the scoring alone on the device: the H models applied to the n matches as [h, n] float64 tensors in
       slabs of 128 hypotheses, the residual test and a count per hypothesis (no sampling, no refit, no mask: less than F does)
  D    the floor of the host route: the matches (16 n bytes) copied to pinned host memory and a synchronise, on the host clock
Printed: microseconds per pair (median and minimum of the turns) and, for F, the share of the float64 issue rate the H x n
residual tests reach: 14 float64 operations each (ten for the two residuals, three for the squared error, one comparison), a
wave-instruction per 64 of them, over 1024 SIMDs at the 1.875 ns per float64 wave-instruction that tools/ubench/valu_rates
measured (profiles/r01_valu_rates.txt).  The refit passes and the launches' fixed costs are in F's time and not in that count, so
the share is a lower bound of the score launch's.  Nothing is asserted.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F64_NS_PER_WAVE_INSTR, SIMDS, OPS_PER_TEST = 1.875, 1024, 14
W, H = 3840, 2160


def matches(n, seed):
    import numpy as np

    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(0, W - 1, n), rng.uniform(0, H - 1, n)], axis=1)
    s, r = 1.01, 0.004
    A = np.array([[s * np.cos(r), -s * np.sin(r)], [s * np.sin(r), s * np.cos(r)]])
    q = (p - [W / 2, H / 2]) @ A.T + [W / 2 + 2.3, H / 2 - 1.1] + rng.normal(0, 0.05, (n, 2))
    kind = rng.uniform(0, 1, n)
    out = kind < 0.4
    q[out] = np.stack([rng.uniform(0, W - 1, out.sum()), rng.uniform(0, H - 1, out.sum())], axis=1)
    q[(kind >= 0.4) & (kind < 0.5)] = np.nan
    return p.astype(np.float32), q.astype(np.float32)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--turns", type=int, default=12)
    ap.add_argument("--matches", default="1024,16384,262144")
    ap.add_argument("--hypotheses", default="256,1024")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fit_motion_bench.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch

    assert torch.cuda.is_available(), "fit_motion_bench needs the GPU: nothing here is measured without one"
    from cuda_optical_flow_2_amd import engine

    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# python tools/fit_motion_bench.py   ({torch.cuda.get_device_name(0)}; {W}x{H}, similarity, radius 1 px, two refits; {args.turns} turns per "
         f"arm, the arms taking turns; no counters were taken)")
    results = []
    for n in (int(v) for v in args.matches.split(",")):
        p, q = matches(n, n)
        tp = [torch.from_numpy(p).cuda() for _ in range(16)]
        tq = [torch.from_numpy(q).cuda() for _ in range(16)]
        host = torch.empty((2, n, 2), dtype=torch.float32).pin_memory()
        for hyp in (int(v) for v in args.hypotheses.split(",")):
            prm = engine._fit_params("similarity", hyp, 1.0, 2, 0)
            models = torch.empty((16, 6), dtype=torch.float64, device="cuda")
            info = torch.empty((16, 8), dtype=torch.int32, device="cuda")
            work = engine._fit_work(prm, 16, "cuda")
            items = [(tp[i], tq[i], None, n, 0, W, H) for i in range(16)]
            # the torch arm's models: any H plausible ones (the scoring costs the same whatever they are)
            gen = torch.Generator(device="cuda").manual_seed(1)
            tm = torch.tensor([1.0, 0.0, 0.0, 0.0, 1.0, 0.0], dtype=torch.float64, device="cuda") + 0.01 * torch.randn((hyp, 6), dtype=torch.float64, device="cuda", generator=gen)
            o = torch.tensor([16.0 * (W - 1), 16.0 * (H - 1)], dtype=torch.float64, device="cuda")

            def f1():
                engine._fit_launch(items[:1], prm, models, info, work)

            def f16():
                engine._fit_launch(items, prm, models, info, work)

            def t():
                u = torch.round(tp[0].double() * 32.0) - o
                v = torch.round(tq[0].double() * 32.0) - o
                ok = torch.isfinite(u).all(dim=1) & torch.isfinite(v).all(dim=1)
                counts = []
                for h0 in range(0, hyp, 128):
                    m = tm[h0:h0 + 128]
                    rx = (m[:, 0:1] * u[:, 0] + m[:, 1:2] * u[:, 1]) + (m[:, 2:3] - v[:, 0])
                    ry = (m[:, 3:4] * u[:, 0] + m[:, 4:5] * u[:, 1]) + (m[:, 5:6] - v[:, 1])
                    counts.append((((rx * rx + ry * ry) <= 1024.0) & ok).sum(dim=1))
                return torch.cat(counts)

            arms = {"F1": f1, "F16": f16, "T": t}
            for f in arms.values():
                f()
            torch.cuda.synchronize()
            got = info.cpu().numpy()
            times, host_us = {k: [] for k in arms}, []
            order = list(arms)
            for turn in range(args.turns):
                for k in order[turn % len(order):] + order[:turn % len(order)]:
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    arms[k]()
                    b.record()
                    times[k].append((a, b))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host[0].copy_(tp[0], non_blocking=True)
                host[1].copy_(tq[0], non_blocking=True)
                torch.cuda.synchronize()
                host_us.append((time.perf_counter() - t0) * 1e6)
            us = {k: [a.elapsed_time(b) * 1e3 / (16 if k == "F16" else 1) for a, b in v] for k, v in times.items()}
            us["D"] = host_us
            floor_us = hyp * n * OPS_PER_TEST / 64.0 * F64_NS_PER_WAVE_INSTR / SIMDS * 1e-3
            res = {"matches": n, "hypotheses": hyp, "usable": int(got[0, 1]), "valid": int(got[0, 2]), "inliers": int(got[0, 5])}
            for k, v in us.items():
                res[f"us_per_pair_{k}"] = {"median": round(statistics.median(v), 2), "min": round(min(v), 2)}
            res["f64_floor_us"] = round(floor_us, 3)
            res["F1_share_of_f64_issue"] = round(floor_us / res["us_per_pair_F1"]["median"], 4)
            res["F16_share_of_f64_issue"] = round(floor_us / res["us_per_pair_F16"]["median"], 4)
            results.append(res)
            emit(json.dumps(res))
    emit("\n| matches | H | F1: one item | F16: per item of 16 | T: torch scoring | D: copy out + synchronise | F1 share of f64 issue | F16 share |")
    emit("|---|---|---|---|---|---|---|---|")
    for r in results:
        emit(f"| {r['matches']} | {r['hypotheses']} | {r['us_per_pair_F1']['median']} | {r['us_per_pair_F16']['median']} | {r['us_per_pair_T']['median']} | "
             f"{r['us_per_pair_D']['median']} | {r['F1_share_of_f64_issue']} | {r['F16_share_of_f64_issue']} |")
    emit("(us per pair, medians)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
