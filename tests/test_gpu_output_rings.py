"""GPU: the five output stages of the stream pipeline side by side on ONE session, each with a ring of its own size at a level of
its own (csrc/out_ring.h keeps one descriptor per ring): no stage's slots, window or newest pair may follow another's.

    compose 2 slots at level 0 | arrows 3 at level 1 | track history 4 at level 0 | motion image + stats 5 at level 1 | displacement 7 at level 0

136 x 72 with 3 levels (every level a multiple of 4, as the sampled stages ask), stream_batch 2, one iteration, 2 B + 3 frames
streamed and drained, then a second stream of the same frames on the same session.  After each stream every accessor returns every
pair inside ITS window, bit-equal to the stage's stateless call on that pair's inputs -- the flows read through flow_of as the
pairs complete, the shift vectors and planes of a pair-at-a-time session of the same parameters -- and refuses the pair just
outside it (another pair for every stage); right after the second stream_begin every accessor refuses pair 1.  The track history
has no accessor: its slots are read from the ring.  tests/test_out_ring.py checks the descriptor alone, on the host."""
import ctypes as C

import numpy as np
import pytest

from cuda_optical_flow_2_amd import synth

pytestmark = pytest.mark.gpu

_vp = C.c_void_p
W, H, LEVELS, WIN, B, RES, N_POINTS = 136, 72, 3, 9, 2, 30, 300
NF = 2 * B + 3
SLOTS = {"compose": 2, "arrows": 3, "tracks": 4, "motion": 5, "disp": 7}
LEVEL = {"compose": 0, "arrows": 1, "tracks": 0, "motion": 1, "disp": 0}


def same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype}{got.shape} vs {want.dtype}{want.shape}"
    a, b = (got.view(np.uint32), want.view(np.uint32)) if got.dtype == np.float32 else (got, want)   # (floats by their bits: NaN == NaN)
    assert np.array_equal(a, b), f"{what}: {int((a != b).sum())}/{got.size} differ"


def window(stage, newest):
    return range(max(1, newest - SLOTS[stage] + 1), newest + 1)


def test_every_stage_keeps_its_own_ring():
    import torch

    assert torch.cuda.is_available(), "this test needs the MI355X"
    from cuda_optical_flow_2_amd import engine as eng

    lib = eng._lib.load()
    pitch = eng.pitch_for(W)
    frames = []
    for i in range(NF):
        buf = torch.zeros((H, pitch), dtype=torch.uint8, device="cuda")
        buf[:, :W] = torch.from_numpy(synth.smooth_pair(W, H, 1.2 * i, -0.6 * i, seed=41)[1]).cuda()
        frames.append(buf[:, :W])

    # what a pair-at-a-time session holds for every pair: per level the flow, the shift vector and both planes
    plain = eng.Session(W, H, LEVELS, WIN, "lk_float", iters=1)
    plain.set_frame_device(frames[0]); plain.build_pyramid(); plain.swap()
    held = {}
    for p in range(1, NF):
        plain.set_frame_device(frames[p]); plain.build_pyramid(); plain.run_flow()
        torch.cuda.synchronize()
        for lv in range(LEVELS):
            prev1, next1 = (plain.plane(i, lv)[0][:, :W >> lv].cpu().numpy() for i in (0, 1))
            held[p, lv] = (plain.flow_host(lv), plain.uv(lv).cpu().numpy() if lv < LEVELS - 1 else None, prev1, next1)   # (the coarsest level has no shift)
        plain.swap()
    plain.close()

    s = eng.Session(W, H, LEVELS, WIN, "lk_float", iters=1, stream_batch=B)
    wl, hl = W >> 1, H >> 1
    _, ny, nx = eng.arrow_grid(wl, hl, RES)
    rng = np.random.default_rng(5)
    start = (rng.random((N_POINTS, 2)) * [W - 1, H - 1]).astype(np.float32)
    motion_rows = torch.full((SLOTS["motion"], hl, wl + 4), 7, dtype=torch.uint8, device="cuda")   # (four bytes of padding a row)
    ring = {"compose": torch.full((SLOTS["compose"], H, W, 2), 7.0, dtype=torch.float32, device="cuda"),
            "arrows": torch.full((SLOTS["arrows"], ny, nx, 4), 7, dtype=torch.int32, device="cuda"),
            "tracks": torch.full((SLOTS["tracks"], N_POINTS, 2), 7.0, dtype=torch.float32, device="cuda"),
            "motion": motion_rows[:, :, :wl],
            "stats": torch.full((SLOTS["motion"], 4), -1, dtype=torch.int64, device="cuda"),
            "disp": torch.full((SLOTS["disp"], H, W, 2), 7.0, dtype=torch.float32, device="cuda")}
    points, status = torch.from_numpy(start).cuda(), torch.zeros(N_POINTS, dtype=torch.int32, device="cuda")
    s.stream_compose(ring["compose"], LEVEL["compose"])
    s.stream_arrows(ring["arrows"], LEVEL["arrows"], RES)
    s.stream_tracks(points, status, ring["tracks"], LEVEL["tracks"])
    s.stream_motion(ring["motion"], ring["stats"], LEVEL["motion"])
    s.stream_displacement(ring["disp"], LEVEL["disp"])
    accessors = {"compose": s.composed_of, "arrows": s.arrows_of, "motion": s.motion_of, "disp": s.displacement_of}

    want = {}   # the stateless calls' results, computed once (first stream) and shared by both

    def references(flows):
        """flows[p]: the levels' flows of pair p as flow_of returned them"""
        pts_d, st_d = torch.from_numpy(start).cuda(), torch.zeros(N_POINTS, dtype=torch.int32, device="cuda")
        for p in range(1, NF):
            for lv in range(LEVELS):
                same(flows[p][lv], held[p, lv][0], f"pair {p} level {lv}: flow_of against the pair-at-a-time session")
            dev = [torch.from_numpy(f).cuda() for f in flows[p]]
            ptrs = (_vp * 12)(*[t.data_ptr() for t in dev])
            want["compose", p] = eng.compose_flow(flows[p], LEVELS, LEVEL["compose"])
            arrows = torch.zeros((ny, nx, 4), dtype=torch.int32, device="cuda")
            eng.check(lib.ofx_sample_arrows(ptrs, wl, hl, LEVELS, LEVEL["arrows"], RES, arrows.data_ptr(), eng._stream_ptr()), "ofx_sample_arrows")
            eng.check(lib.ofx_advect_points(ptrs, W, H, LEVELS, LEVEL["tracks"], p, pts_d.data_ptr(), st_d.data_ptr(), N_POINTS, eng._stream_ptr()),
                      "ofx_advect_points")
            torch.cuda.synchronize()
            want["arrows", p], want["tracks", p] = arrows.cpu().numpy(), pts_d.cpu().numpy()
            _, uv, prev1, next1 = held[p, LEVEL["motion"]]
            want["motion", p] = eng.motion_compensate(prev1, next1, flows[p][LEVEL["motion"]], uv)
            want["disp", p] = eng.flow_displacement(flows[p][LEVEL["disp"]], held[p, LEVEL["disp"]][1])

    for stream in (1, 2):
        s.stream_begin()
        if stream == 2:   # nothing of the first stream is left in any window
            for name, of in accessors.items():
                with pytest.raises(eng.OfxError, match=r"code 1"):
                    of(1)
            points.copy_(torch.from_numpy(start)); status.zero_()
            for name in ("compose", "tracks", "disp"):
                ring[name].fill_(7.0)
            ring["arrows"].fill_(7); motion_rows.fill_(7); ring["stats"].fill_(-1)
        flows, seen = {}, 0
        calls = [lambda f=f: s.stream_submit(f) for f in frames] + [s.stream_drain] * 8
        for call in calls:
            d = call()
            if d == -2:
                break
            if d >= 1:
                torch.cuda.synchronize()
                for p in range(seen + 1, d + 1):
                    flows[p] = [s.flow_of(p, lv)[0].cpu().numpy() for lv in range(LEVELS)]
                seen = d
        assert d == -2 and seen == NF - 1
        if stream == 1:
            references(flows)
        torch.cuda.synchronize()
        newest = NF - 1
        for p in window("compose", newest):
            same(s.composed_of(p).cpu().numpy(), want["compose", p], f"stream {stream}: composed_of({p})")
        for p in window("arrows", newest):
            same(s.arrows_of(p).cpu().numpy(), want["arrows", p], f"stream {stream}: arrows_of({p})")
        for p in window("tracks", newest):
            same(ring["tracks"][(p - 1) % SLOTS["tracks"]].cpu().numpy(), want["tracks", p], f"stream {stream}: history slot of pair {p}")
        same(points.cpu().numpy(), want["tracks", newest], f"stream {stream}: final positions")
        for p in window("motion", newest):
            img, st = s.motion_of(p)
            same(img.cpu().numpy(), want["motion", p][0], f"stream {stream}: motion_of({p}) image")
            same(st.cpu().numpy(), want["motion", p][1], f"stream {stream}: motion_of({p}) stats")
        for p in window("disp", newest):
            same(s.displacement_of(p).cpu().numpy(), want["disp", p], f"stream {stream}: displacement_of({p})")
        outside = {name: newest - SLOTS[name] for name in accessors}   # the pair just below each window: 4, 3, 1 and -1
        assert len(set(outside.values())) == len(outside)
        for name, of in accessors.items():
            for p in (outside[name], newest + 1):
                with pytest.raises(eng.OfxError, match=r"code 1"):
                    of(p)
        assert bool((motion_rows[:, :, wl:] == 7).all()), f"stream {stream}: the motion ring's row padding was written"
    s.close()
