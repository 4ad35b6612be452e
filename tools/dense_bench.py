#!/usr/bin/env python3
"""The coarse-to-fine dense flow (ofx_session_run_flow_dense) against ofx_session_run_flow, and the prolongation launch alone.

  python tools/dense_bench.py [--turns N] [--out profiles/dense_bench.txt]
  python tools/dense_bench.py --median [--turns N] [--valu-ns R1,R2] [--out profiles/dense_median_bench.txt]

One 4K pair (3840 x 2160, 5 levels, 9x9, 3 iterations, min_det 1.0; a texture that moves by (9, 5) pixels), both pyramids resident.
Two sessions with the same parameters live in one process and take turns, N >= 20 of them: in a turn each runs its call once
between two events on the stream, so drift of the machine falls on both alike.  Printed: median and minimum per pair.  The dense
path has (levels - 1) * (iters + 1) dependent launches below its top level on purpose; the number is recorded, not gated.

Then ofx_flow_prolong alone on the dense session's buffers, level 1 -> level 0 (1920 x 1080 -> 3840 x 2160): fused with the warp,
and flow only; median and minimum in microseconds, and the fused launch's algorithmic traffic -- 8 (fine flow stored) + 2 (coarse
flow read, 8 B per four pixels) + 1 (taps, neighbours from the cache) + 1 (warped byte stored) = 12 B per fine pixel -- as a share
of 8 TB/s.  The chain it replaces, the flow-only launch + ofx_warp_levels, is timed the same way (it reads the fine flow back:
about 20 B/px).

--median: the flow median instead (ofx_flow_median, ofx_session_run_flow_dense_median), same pair, one process,
the arms taking turns, HIP events, median / minimum of N turns.
  (a) the launch alone on a level-0 field, radius 1 and 2, flow only and fused with the warp.  The arms rotate over four source /
      destination sets (4 x 133 MB of fields), so no field is in the 256 MiB Infinity Cache when it is read again.  Printed: us, the
      algorithmic traffic -- 8 B read + 8 B written per pixel, with the warp + 1 (taps) + 1 (byte stored) -- as a share of 8 TB/s,
      and, with --valu-ns (the VALU ns per quad step of the two marches, tools/isa_loops.py file.s median_kernel 1 v_min_f32_e32),
      the share of the vector-issue floor: steps per SIMD x ns per step over the time.
  (b) the fused launch against the chain it replaces: the flow-only launch + ofx_warp_levels, on the same sets.
  (c) the pair: run_flow_dense_median (radius 1, 2) beside run_flow_dense, three sessions taking turns."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_GBS = 8000.0
BYTES_PER_PX = 12.0
W, H, LEVELS, WIN, ITERS, MIN_DET = 3840, 2160, 5, 9, 3, 1.0


def timed(fn, turns, warm=3):
    import torch

    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = []
    for _ in range(turns):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        ev.append((a, b))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1e3 for a, b in ev]


def in_turns(arms, turns, warm=2):
    """{name: [us]}: in every turn each arm runs once between two events (arm(t) gets the turn), the order alternating"""
    import torch

    for t in range(warm):
        for fn in arms.values():
            fn(t)
    torch.cuda.synchronize()
    ev = {k: [] for k in arms}
    names = list(arms)
    for t in range(turns):
        for name in (names if t % 2 == 0 else names[::-1]):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            arms[name](t)
            b.record()
            ev[name].append((a, b))
    torch.cuda.synchronize()
    return {k: [a.elapsed_time(b) * 1e3 for a, b in v] for k, v in ev.items()}


def median_main(args):
    import torch

    assert torch.cuda.is_available()
    from cuda_optical_flow_2_amd import engine, lib, synth

    prev, nxt = synth.smooth_pair(W, H, 9.0, 5.0, seed=5)
    res = {"pair": f"{W}x{H}, {LEVELS} levels, {WIN}x{WIN}, {ITERS} iterations, min_det {MIN_DET}, lk_float", "turns": args.turns}
    sessions = {}
    for name in ("dense", "median1", "median2"):
        s = engine.Session(W, H, LEVELS, WIN, "lk_float", iters=ITERS, min_det=MIN_DET)
        s.push_frame_host(prev)
        s.set_frame_host(nxt)
        s.build_pyramid()
        sessions[name] = s
    # (c) the pair
    arms = {"run_dense": lambda t: sessions["dense"].run_flow_dense(),
            "run_dense_median_r1": lambda t: sessions["median1"].run_flow_dense(median=1),
            "run_dense_median_r2": lambda t: sessions["median2"].run_flow_dense(median=2)}
    for k, v in in_turns(arms, args.turns).items():
        res[f"{k}_us_median"], res[f"{k}_us_min"] = round(statistics.median(v), 1), round(min(v), 1)
    for r in (1, 2):
        res[f"median_r{r}_over_dense_median"] = round(res[f"run_dense_median_r{r}_us_median"] / res["run_dense_us_median"], 3)

    # (a), (b) the launch alone: level-0 fields in four sets, each the pair's own unfiltered level-0 flow
    s = sessions["dense"]
    s.run_flow_dense()
    L, st = s.L, engine._stream_ptr()
    flow0, _ = s.flow(0)
    src, g = s.plane(1, 0)
    n_sets = 4
    fin = [flow0.clone() for _ in range(n_sets)]
    fout = [torch.empty_like(flow0) for _ in range(n_sets)]
    img = [torch.zeros((H, g.pitch), dtype=torch.uint8, device="cuda") for _ in range(n_sets)]
    res["field_sets"] = f"{n_sets} x ({fin[0].numel() * 4 / 1e6:.0f} MB read + {fout[0].numel() * 4 / 1e6:.0f} MB written)"

    def median(r, fused):
        d = [lib.MedianDesc(fin[i].data_ptr(), fout[i].data_ptr(), W, H, r, engine.ITER_SCALE, src.data_ptr() if fused else None, g.pitch if fused else 0,
                            img[i].data_ptr() if fused else None, g.pitch if fused else 0) for i in range(n_sets)]
        return lambda t: engine.check(L.ofx_flow_median(C.byref(d[t % n_sets]), 1, st), "ofx_flow_median")

    def chain(r):
        first = median(r, False)
        wd = [lib.WarpDesc(src.data_ptr(), img[i].data_ptr(), lib.Geom.full(W, H, g.pitch), fout[i].data_ptr(), 0, engine.ITER_SCALE, None, 0) for i in range(n_sets)]

        def run(t):
            first(t)
            engine.check(L.ofx_warp_levels(C.byref(wd[t % n_sets]), 1, st), "ofx_warp_levels")
        return run

    arms = {}
    for r in (1, 2):
        arms[f"median_r{r}_flow_only"] = median(r, False)
        arms[f"median_r{r}_fused"] = median(r, True)
        arms[f"median_r{r}_then_warp_levels"] = chain(r)
    us = in_turns(arms, args.turns)
    valu = [float(x) for x in args.valu_ns.split(",")] if args.valu_ns else None
    steps_per_simd = ((W + 3) // 4) * H / 64.0 / (256 * 4)
    for k, v in us.items():
        res[f"{k}_us_median"], res[f"{k}_us_min"] = round(statistics.median(v), 1), round(min(v), 1)
    for r in (1, 2):
        for kind, bpp in (("flow_only", 16.0), ("fused", 18.0)):
            t = res[f"median_r{r}_{kind}_us_median"]
            res[f"median_r{r}_{kind}_share_of_8TBs_at_{bpp:g}B_per_px"] = round(bpp * W * H / (HBM_GBS * 1e3) / t, 3)
            if valu:
                res[f"median_r{r}_{kind}_share_of_valu_issue_floor"] = round(steps_per_simd * valu[r - 1] * 1e-3 / t, 3)
        res[f"median_r{r}_fused_over_chain_median"] = round(res[f"median_r{r}_fused_us_median"] / res[f"median_r{r}_then_warp_levels_us_median"], 3)
    if valu:
        res["valu_ns_per_quad_step_r1_r2"] = valu
        res["valu_issue_floor_us_r1_r2"] = [round(steps_per_simd * x * 1e-3, 1) for x in valu]
    for s in sessions.values():
        s.close()
    text = json.dumps(res, indent=1)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("tools/dense_bench.py --median, one MI355X\n" + text + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--turns", type=int, default=24)
    ap.add_argument("--median", action="store_true", help="measure the flow median (see the module's text)")
    ap.add_argument("--valu-ns", default=None, help="--median: VALU ns per quad step of the radius-1 and radius-2 marches, R1,R2 (tools/isa_loops.py)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.turns >= 20, "at least 20 turns"
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "dense_median_bench.txt" if args.median else "dense_bench.txt")
    if args.median:
        return median_main(args)
    import torch

    assert torch.cuda.is_available()
    from cuda_optical_flow_2_amd import engine, lib, synth

    prev, nxt = synth.smooth_pair(W, H, 9.0, 5.0, seed=5)
    sessions = {}
    for name in ("dense", "flow"):
        s = engine.Session(W, H, LEVELS, WIN, "lk_float", iters=ITERS, min_det=MIN_DET)
        s.push_frame_host(prev)
        s.set_frame_host(nxt)
        s.build_pyramid()
        sessions[name] = s
    calls = {"dense": sessions["dense"].run_flow_dense, "flow": sessions["flow"].run_flow}
    for fn in calls.values():           # load the code objects
        fn()
    torch.cuda.synchronize()
    us = {"dense": [], "flow": []}
    for t in range(args.turns):
        for name in (("dense", "flow") if t % 2 == 0 else ("flow", "dense")):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            calls[name]()
            b.record()
            us[name].append((a, b))
    torch.cuda.synchronize()
    us = {k: [a.elapsed_time(b) * 1e3 for a, b in v] for k, v in us.items()}
    res = {"pair": f"{W}x{H}, {LEVELS} levels, {WIN}x{WIN}, {ITERS} iterations, min_det {MIN_DET}, lk_float", "turns": args.turns}
    for k, v in us.items():
        res[f"run_{k}_us_median"], res[f"run_{k}_us_min"] = round(statistics.median(v), 1), round(min(v), 1)
    res["dense_over_flow_median"] = round(res["run_dense_us_median"] / res["run_flow_us_median"], 3)

    # the prolongation alone, level 1 -> level 0, on the dense session's own buffers
    s = sessions["dense"]
    L = s.L
    coarse, _ = s.flow(1)
    fine, _ = s.flow(0)
    src, g = s.plane(1, 0)
    dst, _ = s.plane(2, 0)
    st = engine._stream_ptr()
    fused = lib.ProlongDesc(coarse.data_ptr(), W >> 1, H >> 1, fine.data_ptr(), W, H, engine.ITER_SCALE, float(WIN), src.data_ptr(), g.pitch,
                            dst.data_ptr(), g.pitch)
    alone = lib.ProlongDesc(coarse.data_ptr(), W >> 1, H >> 1, fine.data_ptr(), W, H, engine.ITER_SCALE, float(WIN), None, 0, None, 0)

    class WarpDesc(C.Structure):
        _fields_ = [("d_src", C.c_void_p), ("d_dst", C.c_void_p), ("geom", lib.Geom), ("d_flow", C.c_void_p), ("flow_row0", C.c_int),
                    ("scale", C.c_float), ("d_status", C.c_void_p), ("status_bit", C.c_int)]

    wd = WarpDesc(src.data_ptr(), dst.data_ptr(), lib.Geom.full(W, H, g.pitch), fine.data_ptr(), 0, engine.ITER_SCALE, None, 0)

    def chain():
        engine.check(L.ofx_flow_prolong(C.byref(alone), 1, st), "ofx_flow_prolong")
        engine.check(L.ofx_warp_levels(C.byref(wd), 1, st), "ofx_warp_levels")

    arms = {"prolong_fused": lambda: engine.check(L.ofx_flow_prolong(C.byref(fused), 1, st), "ofx_flow_prolong"),
            "prolong_flow_only": lambda: engine.check(L.ofx_flow_prolong(C.byref(alone), 1, st), "ofx_flow_prolong"),
            "prolong_then_warp_levels": chain}
    for name, fn in arms.items():
        v = timed(fn, args.turns)
        res[f"{name}_us_median"], res[f"{name}_us_min"] = round(statistics.median(v), 1), round(min(v), 1)
    res["prolong_fused_share_of_8TBs_at_12B_per_px"] = round(BYTES_PER_PX * W * H / (HBM_GBS * 1e3) / res["prolong_fused_us_median"], 3)
    for s in sessions.values():
        s.close()
    text = json.dumps(res, indent=1)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("tools/dense_bench.py, one MI355X\n" + text + "\n")


if __name__ == "__main__":
    main()
