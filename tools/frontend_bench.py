#!/usr/bin/env python3
"""The stream pipeline's colour front end (ofx_frontend_1ch / ofx_session_stream_frontend), measured on its own terms.

  python tools/frontend_bench.py [--steps K] [--warmup W] [--only 4k|1080p] [--trace]

1. Per frame, event-timed (torch events around K rounds): the fused launch, bit-exact and +-1 LSB, with one frame per launch and
   with the B suggest_stream_batch picks for the fast configuration, against the three-launch chain it replaces
   (ofx_grayscale_avg_3ch -> ofx_bilateral_3ch(g, g) -> ofx_extract_ch0) on the same frames, and against the bilateral launch
   alone on a grey 3-channel frame (bilateral_exact_own_kernel through ofx_bilateral_3ch, bilateral_lut_kernel through
   ofx_bilateral_3ch_fast): the targets are <= 1.05 x those.  The colour frames come from a ring of distinct buffers larger
   than the Infinity Cache.
2. The stream tick at 4K with B = 8 (two stages, borrowed planes), iters 1 and 5: grey frames with the front end off against
   colour frames with the front end on (wall time per tick, torch events around K ticks).
--trace: one short 1080p stream of grey frames (front end off) and one of colour frames (on), printing the calls that
launched a tick (for a rocprofv3 --kernel-trace --stats run: the front-end kernel must appear exactly that many times, and only
in the second stream).
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"1080p": (1920, 1080, 4), "4k": (3840, 2160, 5)}   # w, h, levels
_vp = C.c_void_p


def colour_ring(w, h, min_bytes=320e6):
    """distinct colour frames (a texture rolled by i pixels), together larger than the 256 MB Infinity Cache"""
    import numpy as np
    import torch
    from cuda_optical_flow_2_amd import synth

    g = synth.smooth_pair(w, h, 0.0, 0.0, seed=5)[0].astype(np.int32)
    base = torch.from_numpy(np.stack([np.clip(g + 9, 0, 255), np.clip(g - 7, 0, 255), 255 - g], axis=2).astype(np.uint8)).cuda()
    n = max(12, int(min_bytes // (3 * w * h)) + 1)
    return [torch.roll(base, shifts=(i % 7, 3 * i), dims=(0, 1)).contiguous() for i in range(n)]


def timed(fn, steps, warmup):
    """us per call of fn() (enqueued on the current stream), events around `steps` calls"""
    import torch

    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / steps


def kernels(name, steps, warmup):
    import torch
    from cuda_optical_flow_2_amd import engine, lib

    L = lib.load()
    w, h, levels = SIZES[name]
    frames = colour_ring(w, h)
    n = len(frames)
    B = engine.suggest_stream_batch(w, h, levels, borrow_frames=True, two_stage=True)
    outs = [torch.empty((h, engine.pitch_for(w)), dtype=torch.uint8, device="cuda") for _ in range(B)]
    pitch = engine.pitch_for(w)
    g3 = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
    f3 = torch.empty_like(g3)
    st = {"i": 0}

    def fused(mode, nb):
        def go():
            i = st["i"]
            st["i"] += nb
            src = (_vp * nb)(*[frames[(i + k) % n].data_ptr() for k in range(nb)])
            dst = (_vp * nb)(*[outs[k].data_ptr() for k in range(nb)])
            assert L.ofx_frontend_1ch(src, None, 3 * w, dst, None, pitch, nb, w, h, None, mode, 9, 2.0, 10.0, None) == 0
        return go

    def chain():
        i = st["i"]
        st["i"] += 1
        f = frames[i % n]
        assert L.ofx_grayscale_avg_3ch(f.data_ptr(), g3.data_ptr(), w, h, None) == 0
        assert L.ofx_bilateral_3ch(g3.data_ptr(), g3.data_ptr(), f3.data_ptr(), w, h, 9, 9, 2.0, 10.0, None) == 0
        assert L.ofx_extract_ch0(f3.data_ptr(), outs[0].data_ptr(), w, h, pitch, None) == 0

    assert L.ofx_grayscale_avg_3ch(frames[0].data_ptr(), g3.data_ptr(), w, h, None) == 0

    def alone(fast):
        fn = L.ofx_bilateral_3ch_fast if fast else L.ofx_bilateral_3ch
        return lambda: fn(g3.data_ptr(), g3.data_ptr(), f3.data_ptr(), w, h, 9, 9, 2.0, 10.0, None)

    r = {"workload": name, "w": w, "h": h, "B": B}
    r["bilateral_exact_alone_us"] = round(timed(alone(False), steps, warmup), 1)
    r["bilateral_lut_alone_us"] = round(timed(alone(True), steps, warmup), 1)
    r["chain_us_per_frame"] = round(timed(chain, steps, warmup), 1)
    for tag, mode in (("exact", 2), ("fast", 3)):
        for nb in (1, B):
            r[f"fused_{tag}_B{nb}_us_per_frame"] = round(timed(fused(mode, nb), max(1, steps // nb), warmup) / nb, 1)
    r["exact_vs_alone"] = round(r["fused_exact_B1_us_per_frame"] / r["bilateral_exact_alone_us"], 3)
    r["fast_vs_alone"] = round(r["fused_fast_B1_us_per_frame"] / r["bilateral_lut_alone_us"], 3)
    r["exact_vs_chain"] = round(r["fused_exact_B1_us_per_frame"] / r["chain_us_per_frame"], 3)
    return r


def tick(iters, frontend, steps, warmup, frames, grey):
    """us per tick of the 4K B = 8 stream (two stages, borrowed planes), colour frames with the front end or grey frames without"""
    import torch
    from cuda_optical_flow_2_amd import engine

    w, h, levels = SIZES["4k"]
    B = 8
    s = engine.Session(w, h, levels, 9, "lk_float", iters=iters, stream_batch=B, borrow_frames=True, two_stage=True)
    if frontend:
        s.stream_frontend("bilateral", 9, 2.0, 10.0)
    s.stream_begin()
    src = frames if frontend else grey
    n = len(src)
    groups = [engine.FrameGroup([src[(j * B + k) % n] for k in range(B)]) for j in range(n)]
    submit = s.stream_submit_frames_3ch if frontend else s.stream_submit_frames
    st = {"j": 0}

    def go():
        submit(groups[st["j"] % n])
        st["j"] += 1

    us = timed(go, steps, warmup)
    while s.stream_drain() != -2:
        pass
    torch.cuda.synchronize()
    s.close()
    return us


def trace():
    import torch
    from cuda_optical_flow_2_amd import engine

    w, h, levels = SIZES["1080p"]
    B, nf = 16, 80
    frames = colour_ring(w, h, 0)[:4]
    grey = [f[:, :, 0].contiguous() for f in frames]
    for colour in (False, True):
        s = engine.Session(w, h, levels, 7, "lk_float", stream_batch=B, borrow_frames=True, two_stage=True)
        if colour:
            s.stream_frontend("bilateral", 9, 2.0, 10.0, first_grey=True)
        s.stream_begin()
        launching = 0
        for i in range(nf):
            (s.stream_submit_3ch if colour else s.stream_submit)((frames if colour else grey)[i % 4])
            launching += (i + 1) % B == 0
        while s.stream_drain() != -2:
            pass
        torch.cuda.synchronize()
        s.close()
        print(json.dumps({"trace": f"1080p B={B}", "frames": nf, "frontend": colour, "calls_launching_a_tick_with_frames": launching,
                          "frontend_launches_expected": launching if colour else 0}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=sorted(SIZES))
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    import torch

    assert torch.cuda.is_available()
    if a.trace:
        trace()
        return
    for name in ("1080p", "4k"):
        if a.only and a.only != name:
            continue
        print(json.dumps(kernels(name, a.steps, a.warmup)), flush=True)
    if a.only in (None, "4k"):
        w, h, _ = SIZES["4k"]
        frames = colour_ring(w, h)
        grey = [f[:, :, 0].contiguous() for f in frames]
        for iters in (1, 5):
            steps = a.steps if iters == 1 else max(4, a.steps // 4)
            off = tick(iters, False, steps, a.warmup, frames, grey)
            on = tick(iters, True, steps, a.warmup, frames, grey)
            print(json.dumps({"workload": "4k", "B": 8, "iters": iters, "tick_us_frontend_off": round(off, 1), "tick_us_frontend_on": round(on, 1),
                              "overhead_us": round(on - off, 1), "overhead_frac": round((on - off) / off, 3)}), flush=True)


if __name__ == "__main__":
    main()
