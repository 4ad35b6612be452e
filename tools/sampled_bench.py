#!/usr/bin/env python3
"""The stream pipeline's sampled output stage (ofx_session_stream_arrows / _stream_tracks) against the compose ring.

  python tools/sampled_bench.py [--reps R] [--ticks K] [--only 4k|1080p] [--trace]

Four arms of the same pipeline (borrowed frames, two stages; 4K with B = 8, 1080p with B = 16; iters 1 and 5), the frames from a
ring of distinct buffers larger than the Infinity Cache as in bench.py:
  none     no output stage
  sampled  the arrow field at arrow_res 30 plus 4 096 tracked points with a history ring: the reference program's output
  dense    one tracked point per pixel (no history): the gather chain of B dependent steps at full size
  ring     the compose ring (ofx_session_stream_compose)
All four sessions live in one process and take turns: R rounds, in each round every arm runs K ticks between two events on the
stream, so drift of the machine falls on all arms alike.  Printed per tick; "added" is the arm's tick minus the arm none's.  The
dense arm also as bytes per point and pair -- levels x 8 B gathered, plus position and status read once and the position
written once per launch, (8 + 4 + 8) / B -- over the added time, as a fraction of 8 TB/s.  Points and statuses are reset before
every timed block (outside the events), so lost points do not make later blocks cheaper.
--trace: one short 1080p stream with only the sampled stage on, printing the calls that completed pairs (for a
rocprofv3 --kernel-trace --stats run: sample_ring_kernel must appear exactly that many times, compose_ring_kernel never).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_GBS = 8000.0
CONFIGS = {"4k": (3840, 2160, 5, 9, 8), "1080p": (1920, 1080, 4, 7, 16)}   # w, h, levels, window, B (bench.py's workloads)
ARMS = ("none", "sampled", "dense", "ring")
ARROW_RES, TRACKED = 30, 4096


def frame_ring(w, h, min_bytes=320e6):
    """distinct device frames (a texture rolled by i pixels), together larger than the 256 MB Infinity Cache"""
    import torch
    from cuda_optical_flow_2_amd import synth

    base = torch.from_numpy(synth.smooth_pair(w, h, 0.0, 0.0, seed=5)[0]).cuda()
    n = max(24, int(min_bytes // (w * h)) + 1)
    return [torch.roll(base, shifts=(i % 7, 3 * i), dims=(0, 1)).contiguous() for i in range(n)]


class Arm:
    def __init__(self, name, cfg, iters, groups):
        import torch
        from cuda_optical_flow_2_amd import engine

        w, h, L, win, B = cfg
        self.name, self.groups, self.j, self.blocks = name, groups, 0, []
        self.s = engine.Session(w, h, L, win, "lk_float", iters=iters, stream_batch=B, borrow_frames=True, two_stage=True)
        self.pts0 = None
        if name == "ring":
            self.ring = torch.empty((B, h, w, 2), dtype=torch.float32, device="cuda")
            self.s.stream_compose(self.ring, 0)
        elif name == "sampled":
            _, ny, nx = engine.arrow_grid(w, h, ARROW_RES)
            self.arrows = torch.empty((B, ny, nx, 4), dtype=torch.int32, device="cuda")
            g = torch.Generator(device="cpu").manual_seed(3)
            self.pts0 = (torch.rand((TRACKED, 2), generator=g) * torch.tensor([w, h], dtype=torch.float32)).cuda()
            self.hist = torch.empty((B, TRACKED, 2), dtype=torch.float32, device="cuda")
            self.s.stream_arrows(self.arrows, 0, ARROW_RES)
        elif name == "dense":
            ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
            self.pts0 = torch.stack([xs.reshape(-1) + 0.5, ys.reshape(-1) + 0.5], dim=1).cuda()
            self.hist = None
        if self.pts0 is not None:
            self.pts = self.pts0.clone()
            self.st = torch.zeros(self.pts.shape[0], dtype=torch.int32, device="cuda")
            self.s.stream_tracks(self.pts, self.st, self.hist, 0)
        self.s.stream_begin()

    def run(self, ticks, timed):
        import torch

        if self.pts0 is not None:
            self.pts.copy_(self.pts0)
            self.st.zero_()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(ticks):
            self.s.stream_submit_frames(self.groups[self.j % len(self.groups)])
            self.j += 1
        b.record()
        if timed:
            self.blocks.append((a, b, ticks))

    def tick_us(self):
        us = [a.elapsed_time(b) * 1e3 / k for a, b, k in self.blocks]
        return sum(us) / len(us), min(us), max(us)

    def alive(self):
        return None if self.pts0 is None else float((self.st == 0).float().mean())


def measure(name, cfg, iters, frames, reps, ticks):
    import torch
    from cuda_optical_flow_2_amd import engine

    w, h, L, win, B = cfg
    n = len(frames)
    groups = [engine.FrameGroup([frames[(j * B + k) % n] for k in range(B)]) for j in range(n)]
    arms = [Arm(a, cfg, iters, groups) for a in ARMS]
    for arm in arms:
        arm.run(4, False)     # fill the pipeline, load the code objects
    torch.cuda.synchronize()
    for _ in range(reps):
        for arm in arms:
            arm.run(ticks, True)
    torch.cuda.synchronize()
    res = {"workload": name, "w": w, "h": h, "levels": L, "B": B, "iters": iters, "reps": reps, "ticks_per_block": ticks}
    base = None
    for arm in arms:
        avg, lo, hi = arm.tick_us()
        base = avg if arm.name == "none" else base
        res[f"tick_us_{arm.name}"] = round(avg, 1)
        res[f"tick_us_{arm.name}_min_max"] = [round(lo, 1), round(hi, 1)]
        if arm.name != "none":
            res[f"added_us_{arm.name}"] = round(avg - base, 1)
        if arm.alive() is not None:
            res[f"alive_after_block_{arm.name}"] = round(arm.alive(), 3)
    per_point_pair = 8 * L + (8 + 4 + 8) / B
    dense_bytes = per_point_pair * w * h * B
    res["dense_bytes_per_point_pair"] = round(per_point_pair, 2)
    res["dense_frac_of_8TBs"] = round(dense_bytes / (HBM_GBS * 1e3) / max(res["added_us_dense"], 1e-3), 3)
    res["sampled_vs_ring_added"] = round(res["added_us_sampled"] / res["added_us_ring"], 4) if res["added_us_ring"] > 0 else None
    for arm in arms:
        arm.s.close()
    return res


def trace(steps):
    import torch

    cfg = CONFIGS["1080p"]
    frames = frame_ring(cfg[0], cfg[1], 24 * cfg[0] * cfg[1])[:24]
    arm = Arm("sampled", cfg, 1, None)   # (frames go in one at a time here)
    calls = 0
    for i in range(steps):
        calls += arm.s.stream_submit(frames[i % len(frames)]) >= 1
    while True:
        d = arm.s.stream_drain()
        if d == -2:
            break
        calls += d >= 1
    torch.cuda.synchronize()
    arm.s.close()
    print(json.dumps({"trace": "1080p B=16, arrows + 4096 tracks, no compose ring", "frames": steps, "calls_completing_pairs": calls,
                      "sample_ring_kernel_launches_expected": calls, "compose_ring_kernel_launches_expected": 0}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--ticks", type=int, default=10)
    ap.add_argument("--only", choices=sorted(CONFIGS))
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available()
    if args.trace:
        trace(80)
        return
    rows = []
    for name, cfg in CONFIGS.items():
        if args.only and name != args.only:
            continue
        frames = frame_ring(cfg[0], cfg[1])
        for iters in (1, 5):
            res = measure(name, cfg, iters, frames, args.reps, args.ticks)
            print(json.dumps(res), flush=True)
            rows.append(res)
    print("\n| workload | iters | tick none | + sampled (arrows 30 + 4096 tracks) | + dense (point per pixel) | + compose ring | dense: B/point/pair, of 8 TB/s |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['workload']} B={r['B']} | {r['iters']} | {r['tick_us_none']} us | +{r['added_us_sampled']} us | +{r['added_us_dense']} us | "
              f"+{r['added_us_ring']} us | {r['dense_bytes_per_point_pair']} B, {r['dense_frac_of_8TBs']} |")


if __name__ == "__main__":
    main()
