#!/usr/bin/env python3
"""The homography fit (ofx_fit_homography) beside its affine sibling (ofx_fit_motion, affine model), per pair.

  python tools/homography_bench.py [--turns T] [--matches 1024,16384,262144] [--hypotheses 256,1024] [--out profiles/homography_bench.txt]

tools/fit_motion_bench.py's grid: synthetic matches in a 3840 x 2160 frame, here of a mild homography: 0.05 px noise, 40 % uniform
outliers, 10 % unusable; radius 1 px, two refits.  Per (n, H) the arms take turns in one process, T turns (default 12), each turn
of an arm between two events on the stream:
  H1   one ofx_fit_homography call of ONE item
  H16  one call of 16 items (16 copies of the matches in buffers of their own); reported per item
  A1   one ofx_fit_motion call of ONE item, affine model, on the same matches
  A16  the same of 16 items; reported per item
Printed: microseconds per pair (median and minimum of the turns) and, for H, the share of the float64 issue rate the residual
tests of the VALID hypotheses x n reach (a sample that holds an outlier often folds the plane over, W <= 0 at a sample, and such a
hypothesis is not scored): 23 float64 operations each (four for W, six for each residual, three for the squared error, two for the
radius, two comparisons), a wave-instruction per 64 of them, over 1024 SIMDs at the 1.875 ns per float64 wave-instruction that
tools/ubench/valu_rates measured (profiles/r01_valu_rates.txt); for A the 14 operations of tools/fit_motion_bench.py.  The
hypotheses' solves, the refit passes and the launches' fixed costs are in the times and not in that count, so the share is a
lower bound of the score launch's.  Nothing is asserted.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F64_NS_PER_WAVE_INSTR, SIMDS = 1.875, 1024
OPS = {"H": 23, "A": 14}
W, H = 3840, 2160


def matches(n, seed):
    import numpy as np

    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(0, W - 1, n), rng.uniform(0, H - 1, n)], axis=1)
    m = np.array([[1.01, -0.004, 2.3], [0.004, 1.01, -1.1], [2e-6, -1.5e-6, 1.0]])
    t = np.concatenate([p, np.ones((n, 1))], axis=1) @ m.T
    q = t[:, :2] / t[:, 2:3] + rng.normal(0, 0.05, (n, 2))
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "homography_bench.txt"))
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "homography_bench needs the GPU: nothing here is measured without one"
    from cuda_optical_flow_2_amd import engine

    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# python tools/homography_bench.py   ({torch.cuda.get_device_name(0)}; {W}x{H}, radius 1 px, two refits; {args.turns} turns per arm, the arms "
         f"taking turns; no counters were taken)")
    results = []
    for n in (int(v) for v in args.matches.split(",")):
        p, q = matches(n, n)
        tp = [torch.from_numpy(p).cuda() for _ in range(16)]
        tq = [torch.from_numpy(q).cuda() for _ in range(16)]
        items = [(tp[i], tq[i], None, n, 0, W, H) for i in range(16)]
        for hyp in (int(v) for v in args.hypotheses.split(",")):
            hprm, aprm = engine._homography_params(hyp, 1.0, 2, 0), engine._fit_params("affine", hyp, 1.0, 2, 0)
            hmodels = torch.empty((16, 9), dtype=torch.float64, device="cuda")
            amodels = torch.empty((16, 6), dtype=torch.float64, device="cuda")
            hinfo, ainfo = (torch.empty((16, 8), dtype=torch.int32, device="cuda") for _ in range(2))
            hwork, awork = engine._homography_work(hprm, 16, "cuda"), engine._fit_work(aprm, 16, "cuda")
            arms = {"H1": lambda: engine._homography_launch(items[:1], hprm, hmodels, hinfo, hwork),
                    "H16": lambda: engine._homography_launch(items, hprm, hmodels, hinfo, hwork),
                    "A1": lambda: engine._fit_launch(items[:1], aprm, amodels, ainfo, awork),
                    "A16": lambda: engine._fit_launch(items, aprm, amodels, ainfo, awork)}
            for f in arms.values():
                f()
            torch.cuda.synchronize()
            got, agot = hinfo.cpu().numpy(), ainfo.cpu().numpy()
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
            res = {"matches": n, "hypotheses": hyp, "usable": int(got[0, 1]), "valid": int(got[0, 2]), "affine_valid": int(agot[0, 2]), "inliers": int(got[0, 5]),
                   "affine_inliers": int(agot[0, 5])}
            for k, v in us.items():
                res[f"us_per_pair_{k}"] = {"median": round(statistics.median(v), 2), "min": round(min(v), 2)}
            for k in arms:
                scored = res["valid"] if k[0] == "H" else res["affine_valid"]        # (an invalid hypothesis is skipped, not scored)
                floor_us = scored * n * OPS[k[0]] / 64.0 * F64_NS_PER_WAVE_INSTR / SIMDS * 1e-3
                res[f"{k}_share_of_f64_issue"] = round(floor_us / res[f"us_per_pair_{k}"]["median"], 4)
            results.append(res)
            emit(json.dumps(res))
    emit("\n| matches | H | valid | H1: one item | H16: per item of 16 | A1: affine, one item | A16: affine, per item of 16 | H1 share of f64 issue | H16 share | A16 share |")
    emit("|---|---|---|---|---|---|---|---|---|---|")
    for r in results:
        emit(f"| {r['matches']} | {r['hypotheses']} | {r['valid']} | {r['us_per_pair_H1']['median']} | {r['us_per_pair_H16']['median']} | {r['us_per_pair_A1']['median']} | "
             f"{r['us_per_pair_A16']['median']} | {r['H1_share_of_f64_issue']} | {r['H16_share_of_f64_issue']} | {r['A16_share_of_f64_issue']} |")
    emit("(us per pair, medians)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
