#!/usr/bin/env python3
"""The stream pipeline's motion-compensation stage (ofx_session_stream_motion) against the compose ring.

  python tools/motion_bench.py [--reps R] [--ticks K] [--only 4k|1080p] [--quality] [--trace]

Four arms of the same pipeline (borrowed frames, two stages; 4K with B = 8, 1080p with B = 16; iters 1 and 5), the frames from a
ring of distinct buffers larger than the Infinity Cache as in bench.py:
  none     no output stage
  motion   the motion-compensated image and the four sums of every pair (level 0)
  stats    the four sums only (no image is stored: one byte per pixel less)
  ring     the compose ring (ofx_session_stream_compose): the yardstick
All four sessions live in one process and take turns: R rounds (a multiple of four), in each round every arm runs K ticks between
two events on the stream, so drift of the machine falls on all arms alike; four consecutive rounds take the four orders of a Latin
square balanced for carry-over, so that every arm runs directly behind every other arm equally often.  Printed per tick; "added" is the arm's tick minus the arm none's.  The
motion arm also as bytes per pixel -- 8 (flow) + 1 (prev) + 1 (next, the taps mostly hit) + 1 (store) = 11 -- over its added time,
as a fraction of 8 TB/s.
--quality: sum |prev - mc| / sum |prev - next| over 16 pairs of the 4K bench texture at iters 1, 3 and 5 (stats only): what the
flow buys, the repository's first quality figure.  Information, not a test.
--trace: two short 1080p streams, the first with the stage off, the second with image + stats on, printing the calls that
completed pairs (for a rocprofv3 --kernel-trace --stats run: motion_ring_kernel must appear exactly as often as the second
stream's completing calls).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_GBS = 8000.0
BYTES_PER_PX = 11.0
CONFIGS = {"4k": (3840, 2160, 5, 9, 8), "1080p": (1920, 1080, 4, 7, 16)}   # w, h, levels, window, B (bench.py's workloads)
ARMS = ("none", "motion", "stats", "ring")
# the order of the arms in four consecutive rounds: a Latin square balanced for first-order carry-over (Williams design) -- every
# arm is in every position once, and inside the rounds every arm runs directly behind every other arm exactly once
ORDERS = ((0, 1, 3, 2), (1, 2, 0, 3), (2, 3, 1, 0), (3, 0, 2, 1))


def frame_ring(w, h, min_bytes=320e6):
    """distinct device frames (a texture rolled by i pixels), together larger than the 256 MB Infinity Cache"""
    import torch
    from cuda_optical_flow_2_amd import synth

    base = torch.from_numpy(synth.smooth_pair(w, h, 0.0, 0.0, seed=5)[0]).cuda()
    n = max(24, int(min_bytes // (w * h)) + 1)
    return [torch.roll(base, shifts=(i % 7, 3 * i), dims=(0, 1)).contiguous() for i in range(n)]


class Arm:
    def __init__(self, name, cfg, iters, groups, n_slots=None):
        import torch
        from cuda_optical_flow_2_amd import engine

        w, h, L, win, B = cfg
        n_slots = n_slots or B
        self.name, self.groups, self.j, self.blocks = name, groups, 0, []
        self.s = engine.Session(w, h, L, win, "lk_float", iters=iters, stream_batch=B, borrow_frames=True, two_stage=True)
        self.img = self.stats = None
        if name == "ring":
            self.ring = torch.empty((B, h, w, 2), dtype=torch.float32, device="cuda")
            self.s.stream_compose(self.ring, 0)
        elif name in ("motion", "stats"):
            if name == "motion":
                self.img = torch.empty((n_slots, h, w), dtype=torch.uint8, device="cuda")
            self.stats = torch.zeros((n_slots, 4), dtype=torch.int64, device="cuda")
            self.s.stream_motion(self.img, self.stats, 0)
        self.s.stream_begin()

    def run(self, ticks, timed):
        import torch

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
    for r in range(reps):
        for i in ORDERS[r % len(ORDERS)]:
            arms[i].run(ticks, True)
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
    res["motion_frac_of_8TBs"] = round(BYTES_PER_PX * w * h * B / (HBM_GBS * 1e3) / max(res["added_us_motion"], 1e-3), 3)
    res["motion_vs_ring_added"] = round(res["added_us_motion"] / res["added_us_ring"], 3) if res["added_us_ring"] > 0 else None
    res["stats_vs_motion_added"] = round(res["added_us_stats"] / res["added_us_motion"], 3) if res["added_us_motion"] > 0 else None
    st = arms[1].stats.cpu()
    res["last_tick_sad_mc_over_sad_raw"] = round(float(st[:, 2].sum()) / max(float(st[:, 1].sum()), 1.0), 4)
    for arm in arms:
        arm.s.close()
    return res


def quality(frames):
    """sad_mc / sad_raw over 16 consecutive pairs of the 4K bench texture (each frame the one before rolled by a few pixels)"""
    import torch

    cfg = CONFIGS["4k"]
    pairs = 2 * cfg[4]
    out = {}
    for iters in (1, 3, 5):
        arm = Arm("stats", cfg, iters, None, n_slots=pairs)
        for i in range(pairs + 1):
            arm.s.stream_submit(frames[i])
        while arm.s.stream_drain() != -2:
            pass
        torch.cuda.synchronize()
        st = arm.stats.cpu()
        assert int(st[:, 0].min()) == cfg[0] * cfg[1]
        ratios = (st[:, 2].double() / st[:, 1].double()).tolist()
        out[f"iters_{iters}"] = {"sad_mc_over_sad_raw": round(float(st[:, 2].sum()) / float(st[:, 1].sum()), 4),
                                 "min_max_per_pair": [round(min(ratios), 4), round(max(ratios), 4)], "not_warped_px": int(st[:, 3].sum())}
        arm.s.close()
    print(json.dumps({"quality": "4K bench texture, 16 pairs, level 0, lk_float window 9, 5 levels", **out}), flush=True)
    return out


def trace(steps):
    import torch

    cfg = CONFIGS["1080p"]
    frames = frame_ring(cfg[0], cfg[1], 24 * cfg[0] * cfg[1])[:24]
    calls = {}
    for name in ("none", "motion"):      # (frames go in one at a time here)
        arm = Arm(name, cfg, 1, None)
        n = 0
        for i in range(steps):
            n += arm.s.stream_submit(frames[i % len(frames)]) >= 1
        while True:
            d = arm.s.stream_drain()
            if d == -2:
                break
            n += d >= 1
        torch.cuda.synchronize()
        arm.s.close()
        calls[name] = n
    print(json.dumps({"trace": "1080p B=16: a stream with the stage off, then one with image + stats", "frames_per_stream": steps,
                      "calls_completing_pairs_stage_off": calls["none"], "calls_completing_pairs_stage_on": calls["motion"],
                      "motion_ring_kernel_launches_expected": calls["motion"]}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--ticks", type=int, default=10)
    ap.add_argument("--only", choices=sorted(CONFIGS))
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available()
    if args.trace:
        trace(80)
        return
    if args.quality:
        quality(frame_ring(*CONFIGS["4k"][:2]))
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
    print("\n| workload | iters | tick none | + motion (image + stats) | + motion (stats only) | + compose ring | motion / ring | motion: of 8 TB/s at 11 B/px |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['workload']} B={r['B']} | {r['iters']} | {r['tick_us_none']} us | +{r['added_us_motion']} us | +{r['added_us_stats']} us | "
              f"+{r['added_us_ring']} us | {r['motion_vs_ring_added']} | {r['motion_frac_of_8TBs']} |")


if __name__ == "__main__":
    main()
