#!/usr/bin/env python3
"""The sparse Lucas-Kanade launch (ofx_track_points) beside the path video_tracks runs, per pair.

  python tools/klt_bench.py [--turns T] [--size WxH] [--levels L] [--windows 9,21] [--points 1024,16384,262144] [--out profiles/klt_bench.txt]

4K, 5 levels.  The frames are a texture drifting by (3, 1) px per frame, 33 distinct frames whose pyramids (366 MB) are larger than
the 256 MiB Infinity Cache; the points are good_features of frame 0, thinned evenly to the count asked (where the frame has
fewer, a regular grid makes up the rest).  Per window and point count four arms take turns in one process, T turns (default 12),
each turn of an arm between two events on the stream, the points reset before it (outside the events):
  K1  eight consecutive pairs, one ofx_track_points launch per pair
  K8  the same eight pairs in ONE launch
  V   what video_tracks runs for the same eight pairs: a stream tick of eight borrowed frames (two stages, one iteration) with the
      sampled stage tracking the same points (tools/sampled_bench.py's method); V0 is the tick without the sampled stage
Printed: microseconds per pair (median and minimum of the turns), the iterations per point and pair from d_stats, the bytes the
launch asks for -- (2R + 4)^2 per point and level plus (2R + 2)^2 per iteration -- as a share of 8 TB/s, and the point count at which
K8 stops being cheaper than V (linear between the counts measured).  No threshold is asserted.
A companion line: the share of good_features within 0.25 px of the truth after a pan by (9, 5) on the 192 x 128 texture of
tests/klt_ref.py, for engine.video_klt and for engine.video_tracks_auto, both on the device.  Recorded, not asserted.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_GBS = 8000.0
PAIRS = 8


def quality():
    import numpy as np
    import torch
    import klt_ref as K
    from cuda_optical_flow_2_amd import engine

    w, h, levels, win = 192, 128, 4, 9
    clip = torch.from_numpy(np.stack([K.cosine_texture(w, h), K.cosine_texture(w, h, 9.0, 5.0)])).cuda()
    out = {}
    pos, status, _ = engine.video_klt(clip, None, levels, win)
    err = (pos[1] - pos[0] - torch.tensor([9.0, 5.0], device="cuda")).abs().amax(dim=1)
    out["video_klt"] = {"features": int(pos.shape[1]), "tracked": int((status == 0).sum()), "within_0.25px": round(float(((status == 0) & (err <= 0.25)).float().mean()), 3)}
    pos, status, _ = engine.video_tracks_auto(clip, levels, win)
    err = (pos[1] - pos[0] - torch.tensor([9.0, 5.0], device="cuda")).abs().amax(dim=1)
    out["video_tracks_auto"] = {"features": int(pos.shape[1]), "tracked": int((status == 0).sum()),
                                "within_0.25px": round(float(((status == 0) & (err <= 0.25)).float().mean()), 3)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--turns", type=int, default=12)
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--windows", default="9,21")
    ap.add_argument("--points", default="1024,16384,262144")
    ap.add_argument("--frames", type=int, default=33)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "klt_bench.txt"))
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "klt_bench needs the GPU: nothing here is measured without one"
    from cuda_optical_flow_2_amd import engine, synth

    w, h = (int(v) for v in args.size.split("x"))
    L = args.levels
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    base = torch.from_numpy(synth.smooth_pair(w, h, 0.0, 0.0, seed=5)[0]).cuda()
    frames = [torch.roll(base, shifts=(i, 3 * i), dims=(0, 1)).contiguous() for i in range(args.frames)]
    pyr = [engine.klt_pyramid(f, L) for f in frames]
    pyr_mb = sum(p.numel() for p in pyr[0].planes) * len(pyr) / 1e6
    n_chains = (len(frames) - 1) // PAIRS
    groups = [engine.FrameGroup([frames[c * PAIRS + 1 + k] for k in range(PAIRS)]) for c in range(n_chains)]
    emit(f"# python tools/klt_bench.py   ({torch.cuda.get_device_name(0)}; {w}x{h}, {L} levels, {len(frames)} frames drifting by (3, 1) px, pyramids "
         f"{pyr_mb:.0f} MB; {args.turns} turns per arm, the arms taking turns, eight pairs per turn; no counters were taken)")
    results = []
    for win in (int(v) for v in args.windows.split(",")):
        R = win // 2
        prm = engine._track_params(win, 10, 1 / 32, 0.0, 0)
        for n_want in (int(v) for v in args.points.split(",")):
            cell = 4
            while (w // (2 * cell)) * (h // (2 * cell)) >= n_want and cell < 128:
                cell *= 2
            seeds, _ = engine.good_features(frames[0], win, cell)
            assert seeds.shape[0] >= 1
            pick = torch.linspace(0, seeds.shape[0] - 1, min(n_want, seeds.shape[0]), device="cuda").round().long()
            pts0 = seeds[pick].contiguous()
            n_feat = int(pts0.shape[0])
            if n_feat < n_want:                       # (the frame has fewer features than asked: the rest is a regular grid inside the border)
                m = n_want - n_feat
                gx = max(int((m * w / h) ** 0.5), 1)
                i = torch.arange(m, device="cuda")
                grid = torch.stack([(win + (i % gx) * (w - 2 * win) / gx).floor(), (win + (i // gx) * (h - 2 * win) / (m // gx + 1)).floor()], dim=1)
                pts0 = torch.cat([pts0, grid.float()]).contiguous()
            n = int(pts0.shape[0])
            pts, st = pts0.clone(), torch.zeros(n, dtype=torch.int32, device="cuda")
            stats = torch.zeros((PAIRS, 7), dtype=torch.int64, device="cuda")
            sess = {}
            for name in ("V", "V0"):
                s = engine.Session(w, h, L, win, "lk_float", iters=1, stream_batch=PAIRS, borrow_frames=True, two_stage=True)
                if name == "V":
                    s.stream_tracks(pts, st, None, 0)
                s.stream_begin()
                sess[name] = s

            def k1(c):
                for b in range(PAIRS):
                    engine._track_launch(pyr[c * PAIRS + b:c * PAIRS + b + 2], prm, 1 + b, pts, st)

            def k8(c):
                engine._track_launch(pyr[c * PAIRS:c * PAIRS + PAIRS + 1], prm, 1, pts, st)

            def v(c):
                sess["V"].stream_submit_frames(groups[c])

            def v0(c):
                sess["V0"].stream_submit_frames(groups[c])

            arms = {"K1": k1, "K8": k8, "V": v, "V0": v0}
            engine._track_launch(pyr[:PAIRS + 1], prm, 1, pts, st, None, None, stats)      # untimed: the counts, and the code object
            torch.cuda.synchronize()
            counts = stats.cpu().numpy()
            for f in arms.values():
                pts.copy_(pts0), st.zero_()
                f(0)
            torch.cuda.synchronize()
            times = {k: [] for k in arms}
            order = list(arms)
            for t in range(args.turns):
                c = t % n_chains
                for k in order[t % len(order):] + order[:t % len(order)]:
                    pts.copy_(pts0), st.zero_()
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    arms[k](c)
                    b.record()
                    times[k].append((a, b))
            torch.cuda.synchronize()
            for s in sess.values():
                s.close()
            us = {k: [a.elapsed_time(b) * 1e3 / PAIRS for a, b in v_] for k, v_ in times.items()}
            iters = float(counts[:, 5].sum()) / (n * PAIRS)
            tracked = int(counts[:, 0].sum())
            req_bytes = float(counts[:, 0].sum() + counts[:, 1:5].sum()) * L * (2 * R + 4) ** 2 + float(counts[:, 5].sum()) * (2 * R + 2) ** 2
            res = {"window": win, "points": n, "features_among_them": n_feat, "cell": cell, "alive_after_8_pairs": int(counts[-1, 0]), "iterations_per_point_pair": round(iters, 2)}
            for k, v_ in us.items():
                res[f"us_per_pair_{k}"] = {"median": round(statistics.median(v_), 2), "min": round(min(v_), 2)}
            k8_med = res["us_per_pair_K8"]["median"]
            res["K8_ns_per_point_pair"] = round(1e3 * k8_med / n, 2)
            res["K8_ns_per_point_iteration"] = round(1e3 * k8_med * PAIRS / max(float(counts[:, 5].sum()), 1.0), 3)
            res["K8_requested_bytes_share_of_8TBs"] = round(req_bytes / PAIRS / (HBM_GBS * 1e3) / k8_med, 4)
            res["point_pairs_tracked"] = tracked
            results.append(res)
            emit(json.dumps(res))
    emit("\n| window | points | K1: a launch per pair | K8: eight pairs per launch | V: stream tick + sampled stage | V0: the tick alone | iterations per point and pair |")
    emit("|---|---|---|---|---|---|---|")
    for r in results:
        emit(f"| {r['window']} | {r['points']} | {r['us_per_pair_K1']['median']} | {r['us_per_pair_K8']['median']} | {r['us_per_pair_V']['median']} | "
             f"{r['us_per_pair_V0']['median']} | {r['iterations_per_point_pair']} |")
    emit("(us per pair, medians)")
    for win in sorted({r["window"] for r in results}):
        rs = sorted((r for r in results if r["window"] == win), key=lambda r: r["points"])
        d = [(r["points"], r["us_per_pair_K8"]["median"] - r["us_per_pair_V"]["median"]) for r in rs]
        if all(x < 0 for _, x in d):
            cross = f"above {d[-1][0]} points (the sparse launch is the cheaper one at every count measured)"
        elif d[0][1] >= 0:
            cross = f"below {d[0][0]} points (the sparse launch is the dearer one at every count measured)"
        else:
            (n0, x0), (n1, x1) = next((a, b) for a, b in zip(d, d[1:]) if a[1] < 0 <= b[1])
            cross = f"about {int(n0 + (n1 - n0) * (-x0) / (x1 - x0))} points (linear between {n0} and {n1})"
        emit(f"window {win}: K8 stops being cheaper than V at {cross}")
    emit("quality on the pan by (9, 5), 192 x 128, 4 levels, window 9: " + json.dumps(quality()))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
