"""GPU: the stream pipeline's colour front end -- grayscale_avg + the 9x9 bilateral pre-filter of main.cu:222-240 in one batched
launch (ofx_frontend_1ch) -- against the oracle and the existing three-launch chain, and the stream pipeline fed colour frames
(ofx_session_stream_frontend / _submit_3ch) against the same pipeline fed the chain's filtered grey frames, bit for bit."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_same
from cuda_optical_flow_2_amd import synth

pytestmark = pytest.mark.gpu

GUARD = 64   # bytes of 0x5A before and after every destination
GREY, BIL, FAST = 1, 2, 3   # OFX_FRONTEND_GREY / _BILATERAL / _BILATERAL_FAST
_vp = C.c_void_p


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cuda_optical_flow_2_amd import engine

    return engine


@pytest.fixture(scope="module")
def L(eng):
    from cuda_optical_flow_2_amd import lib

    return lib.load()


def _colour(w, h, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "saturated":
        return rng.choice(np.array([0, 1, 254, 255], np.uint8), (h, w, 3))
    g = synth.smooth_pair(w, h, 0.0, 0.0, seed=seed)[1].astype(np.int32)   # a channel mean that equals no single channel
    return np.stack([np.clip(g + 9, 0, 255), np.clip(g - 7, 0, 255), np.clip(255 - g, 0, 255)], axis=2).astype(np.uint8)


class Src:
    """A colour frame in device memory at row pitch `pitch` (>= 3w; 3w itself = tightly packed), padding bytes 0xA5."""

    def __init__(self, img, pitch):
        import torch

        h, w, _ = img.shape
        self.pitch = pitch
        self.buf = torch.full((h * pitch,), 0xA5, dtype=torch.uint8, device="cuda")
        self.buf.view(h, pitch)[:, :3 * w] = torch.from_numpy(np.ascontiguousarray(img).reshape(h, 3 * w)).cuda()
        self.ptr = self.buf.data_ptr()


class Dst:
    """A one-channel plane at row pitch `pitch` with GUARD guard bytes before and after, everything 0x5A."""

    def __init__(self, w, h, pitch):
        import torch

        self.w, self.h, self.pitch = w, h, pitch
        self.buf = torch.full((2 * GUARD + h * pitch,), 0x5A, dtype=torch.uint8, device="cuda")
        self.ptr = self.buf.data_ptr() + GUARD

    def check(self, want, what):
        b = self.buf.cpu().numpy()
        body = b[GUARD:GUARD + self.h * self.pitch].reshape(self.h, self.pitch)
        assert_same(body[:, :self.w], want, what)
        assert (b[:GUARD] == 0x5A).all() and (b[GUARD + self.h * self.pitch:] == 0x5A).all(), f"{what}: guard bytes written"
        assert (body[:, self.w:] == 0x5A).all(), f"{what}: row padding written"


def _run(L, srcs, dsts, w, h, modes, window=9, ss=2.0, sb=10.0):
    import torch

    n = len(srcs)
    rc = L.ofx_frontend_1ch((_vp * n)(*[s.ptr for s in srcs]), (C.c_int * n)(*[s.pitch for s in srcs]), 0, (_vp * n)(*[d.ptr for d in dsts]),
                            (C.c_int * n)(*[d.pitch for d in dsts]), 0, n, w, h, (C.c_int * n)(*modes), 0, window, ss, sb, None)
    torch.cuda.synchronize()
    return rc


def _oracle_1ch(oracle, img, mode, window=9, ss=2.0, sb=10.0):
    g = oracle.grayscale_avg(img)
    if mode == GREY:
        return g[:, :, 0]
    return oracle.bilateral_3ch(g, g, window, window, ss, sb)[:, :, 0]


@pytest.mark.parametrize("size", [(1, 1), (7, 5), (127, 40), (128, 33), (129, 35), (333, 121)])
@pytest.mark.parametrize("pitched", [False, True])
def test_frontend_exact_against_oracle(L, oracle, size, pitched):
    w, h = size
    for kind, seed in (("mean", 3), ("saturated", 4), ("random", 5)):
        img = _colour(w, h, kind, seed + w)
        for mode in (BIL, GREY):
            src = Src(img, 3 * w + (52 if pitched else 0))
            dst = Dst(w, h, w + (21 if pitched else 0))
            assert _run(L, [src], [dst], w, h, [mode]) == 0
            dst.check(_oracle_1ch(oracle, img, mode), f"{w}x{h} {kind} mode {mode}")


@pytest.mark.parametrize("window", [3, 5, 7, 9, 11, 13])
def test_frontend_windows_and_sigmas(L, oracle, window):
    w, h = 203, 77
    for i, (ss, sb) in enumerate(((2.0, 10.0), (1.0, 3.0), (3.5, 40.0))):
        img = _colour(w, h, ("mean", "random", "saturated")[i], 11 + window)
        src, dst = Src(img, 3 * w), Dst(w, h, w)
        assert _run(L, [src], [dst], w, h, [BIL], window, ss, sb) == 0
        dst.check(_oracle_1ch(oracle, img, BIL, window, ss, sb), f"window {window} sigmas ({ss}, {sb})")


def test_frontend_fast_is_within_one_lsb(L, oracle):
    worst = 0
    for (w, h, window, ss, sb) in ((333, 121, 9, 2.0, 10.0), (130, 131, 5, 1.5, 20.0), (64, 4, 13, 3.0, 40.0), (203, 77, 9, 2.0, 400.0)):
        for kind in ("mean", "random"):
            img = _colour(w, h, kind, w + window)
            src, dst = Src(img, 3 * w), Dst(w, h, w + 3)
            assert _run(L, [src], [dst], w, h, [FAST], window, ss, sb) == 0
            b = dst.buf.cpu().numpy()
            body = b[GUARD:GUARD + h * dst.pitch].reshape(h, dst.pitch)
            d = np.abs(body[:, :w].astype(int) - _oracle_1ch(oracle, img, BIL, window, ss, sb).astype(int))
            worst = max(worst, int(d.max()))
            assert (b[:GUARD] == 0x5A).all() and (b[GUARD + h * dst.pitch:] == 0x5A).all() and (body[:, w:] == 0x5A).all()
    assert worst <= 1, worst


def test_frontend_batch_of_sixteen_mixed_modes(L, oracle):
    w, h = 161, 53
    modes = [BIL, GREY, FAST, BIL, BIL, GREY, FAST, FAST, BIL, GREY, BIL, FAST, GREY, BIL, BIL, FAST]
    imgs = [_colour(w, h, ("mean", "random", "saturated")[i % 3], 40 + i) for i in range(16)]
    srcs = [Src(img, 3 * w + 4 * (i % 3)) for i, img in enumerate(imgs)]
    dsts = [Dst(w, h, w + 7 * (i % 4)) for i in range(16)]
    assert _run(L, srcs, dsts, w, h, modes) == 0
    for i, (img, m, d) in enumerate(zip(imgs, modes, dsts)):
        want = _oracle_1ch(oracle, img, GREY if m == GREY else BIL)
        if m == FAST:
            b = d.buf.cpu().numpy()[GUARD:GUARD + h * d.pitch].reshape(h, d.pitch)[:, :w]
            assert np.abs(b.astype(int) - want.astype(int)).max() <= 1, f"frame {i}"
        else:
            d.check(want, f"frame {i} mode {m}")


def _chain(L, src3, w, h, dst1, dst_pitch, bilateral=True, window=9, ss=2.0, sb=10.0):
    """The existing three-launch chain on device tensors: grayscale_avg -> bilateral(g, g) -> channel 0."""
    import torch

    g = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
    assert L.ofx_grayscale_avg_3ch(src3.data_ptr(), g.data_ptr(), w, h, None) == 0
    if bilateral:
        f = torch.empty_like(g)
        assert L.ofx_bilateral_3ch(g.data_ptr(), g.data_ptr(), f.data_ptr(), w, h, window, window, ss, sb, None) == 0
        g = f
    assert L.ofx_extract_ch0(g.data_ptr(), dst1.data_ptr(), w, h, dst_pitch, None) == 0


@pytest.mark.parametrize("size", [(3840, 2160), (7680, 4320)])
def test_frontend_large_frames_equal_the_chain(L, size):
    import torch

    w, h = size
    img = torch.from_numpy(_colour(w, h, "mean", 9)).cuda()
    img[h // 3:h // 2] = torch.from_numpy(_colour(w, h // 2 - h // 3, "random", 10)).cuda()
    want = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    _chain(L, img, w, h, want, w)
    for mode in (BIL, FAST):
        got = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
        rc = L.ofx_frontend_1ch((_vp * 1)(img.data_ptr()), None, 3 * w, (_vp * 1)(got.data_ptr()), None, w, 1, w, h, None, mode, 9, 2.0, 10.0, None)
        assert rc == 0
        torch.cuda.synchronize()
        if mode == BIL:
            assert torch.equal(got, want), f"{w}x{h}: {int((got != want).sum())} bytes differ"
        else:
            assert int((got.int() - want.int()).abs().max()) <= 1


# ---- the stream pipeline --------------------------------------------------------------------------------------------------

def _clip(w, h, nf, seed=21):
    out = []
    for i in range(nf):
        g = synth.smooth_pair(w, h, 1.3 * i, -0.7 * i, seed=seed)[1].astype(np.int32)
        out.append(np.stack([np.clip(g + 11, 0, 255), np.clip(g - 5, 0, 255), np.clip(g + (i % 3), 0, 255)], axis=2).astype(np.uint8))
    return out


def _stream(s, frames, submit, L_levels, B):
    """Run one stream (stream_batch B); returns {pair: [flow per level]} as host arrays, read while each pair is among the newest B."""
    import torch

    got, seen = {}, 0

    def take(done):
        nonlocal seen
        if done >= 1:
            torch.cuda.synchronize()
            for pair in range(seen + 1, done + 1):
                if pair > done - B:
                    got[pair] = [s.flow_of(pair, k)[0].cpu().numpy() for k in range(L_levels)]
            seen = done

    s.stream_begin()
    for f in frames:
        take(submit(f))
    while True:
        done = s.stream_drain()
        if done == -2:
            break
        take(done)
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("B", [1, 2, 8])
@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("borrow", [0, 1])
def test_pipeline_colour_equals_grey_on_the_chains_frames(eng, L, B, iters, borrow):
    import torch

    w, h, lv, win, nf = 192, 128, 3, 9, 2 * B + 5
    clip = [torch.from_numpy(f).cuda() for f in _clip(w, h, nf, seed=B * 10 + iters)]
    pitch = eng.pitch_for(w)
    for first_grey in (False, True):
        grey = torch.zeros((nf, h, pitch), dtype=torch.uint8, device="cuda")
        for i, f in enumerate(clip):
            _chain(L, f, w, h, grey[i], pitch, bilateral=not (first_grey and i == 0))
        results = []
        for colour in (False, True):
            s = eng.Session(w, h, lv, win, "lk_float", iters=iters, stream_batch=B, borrow_frames=bool(borrow), two_stage=bool(borrow))
            ring = torch.full((nf - 1, h, w, 2), float("nan"), dtype=torch.float32, device="cuda")
            s.stream_compose(ring, 0)
            if colour:
                s.stream_frontend("bilateral", 9, 2.0, 10.0, first_grey=first_grey)
            runs = []
            for rep in range(2):   # a second stream on the same session, after stream_begin
                if colour:
                    got = _stream(s, clip, s.stream_submit_3ch, lv, B)
                else:
                    got = _stream(s, [grey[i, :, :w] for i in range(nf)], s.stream_submit, lv, B)
                runs.append((got, ring.cpu().numpy().copy()))
            s.close()
            results.append(runs)
        for rep in range(2):
            (g_flow, g_ring), (c_flow, c_ring) = results[0][rep], results[1][rep]
            assert sorted(g_flow) == sorted(c_flow) and len(c_flow) > 0
            what = f"B={B} iters={iters} borrow={borrow} first_grey={first_grey} stream {rep}"
            assert_same(c_ring, g_ring, what + ": composed ring")
            assert not np.isnan(c_ring).all()
            for p in c_flow:
                for k in range(lv):
                    assert_same(c_flow[p][k], g_flow[p][k], f"{what}: pair {p} level {k}")


def test_pipeline_batched_submit_equals_single_submits(eng, L):
    """stream_submit_frames_3ch = n calls of stream_submit_3ch; grey front-end mode = the chain without the filter."""
    import torch

    w, h, lv, nf = 128, 96, 3, 11
    clip = [torch.from_numpy(f).cuda() for f in _clip(w, h, nf, seed=5)]
    rings = []
    for batched in (False, True):
        s = eng.Session(w, h, lv, 9, "lk_float", stream_batch=4, borrow_frames=True, two_stage=True)
        ring = torch.zeros((nf - 1, h, w, 2), dtype=torch.float32, device="cuda")
        s.stream_compose(ring, 0)
        s.stream_frontend("grey")
        s.stream_begin()
        if batched:
            s.stream_submit_frames_3ch(clip[:6])
            s.stream_submit_frames_3ch(clip[6:])
        else:
            for f in clip:
                s.stream_submit_3ch(f)
        while s.stream_drain() != -2:
            pass
        torch.cuda.synchronize()
        rings.append(ring.cpu().numpy())
        s.close()
    assert_same(rings[1], rings[0], "batched vs single submits")
    grey = torch.zeros((nf, h, w), dtype=torch.uint8, device="cuda")
    for i, f in enumerate(clip):
        _chain(L, f, w, h, grey[i], w, bilateral=False)
    assert_same(rings[0], eng.video_flow(grey, lv, 9, batch=4).cpu().numpy(), "grey front end vs grey clip")


def _main_cu_loop(oracle, frames, levels):
    """main.cu:192-272 restated on the oracle (as tests/test_gpu_surface.py's replay test): the first frame grey only, the others
    grey + bilateral 9x9 (2, 10); pyramid; calc_opt_flow (window 19) per level; the composed level-0 field per pair."""
    h, w, _ = frames[0].shape
    prev_pyr = oracle.gauss_pyramid(oracle.grayscale_avg(frames[0]), levels)
    out, filtered = [], [oracle.grayscale_avg(frames[0])[:, :, 0]]
    for f in range(1, len(frames)):
        gray = oracle.grayscale_avg(frames[f])
        filt = oracle.bilateral_3ch(gray, gray, 9, 9, 2.0, 10.0)
        filtered.append(filt[:, :, 0])
        pyr = oracle.gauss_pyramid(filt, levels)
        flow = [np.zeros((h >> k, w >> k, 2), np.float32) for k in range(levels)]
        for k in range(levels - 1, -1, -1):
            oracle.calc_opt_flow_gpu(prev_pyr[k], pyr[k], flow, k, levels, 19, exact_sums=True)
        out.append(oracle.compose_flow(flow, levels, 0))
        prev_pyr = pyr
    return np.stack(out), np.stack(filtered)


def test_video_flow_of_a_colour_clip_is_main_cu(eng, oracle):
    import torch

    w, h, levels = 320, 240, 4
    frames = _clip(w, h, 4, seed=77)
    want, filtered = _main_cu_loop(oracle, frames, levels)
    clip = torch.from_numpy(np.stack(frames)).cuda()
    got = eng.video_flow(clip, levels, 19, "lk_float")
    assert_same(got.cpu().numpy(), want, "video_flow([N, H, W, 3]) vs the oracle's main.cu loop")
    grey = eng.video_flow(torch.from_numpy(filtered).cuda(), levels, 19, "lk_float")
    assert_same(got.cpu().numpy(), grey.cpu().numpy(), "colour clip vs its filtered grey clip")
    # a clip whose layout needs the copy (channels-last view of a planar tensor), two pairs per launch
    planar = torch.from_numpy(np.ascontiguousarray(np.stack(frames).transpose(0, 3, 1, 2))).cuda()
    got2 = eng.video_flow(planar.permute(0, 2, 3, 1), levels, 19, "lk_float", batch=2)
    assert_same(got2.cpu().numpy(), want, "video_flow of a strided colour clip")


def test_video_flow_frontend_choices(eng, L, oracle):
    import torch

    w, h, levels, nf = 128, 96, 3, 5
    frames = _clip(w, h, nf, seed=12)
    clip = torch.from_numpy(np.stack(frames)).cuda()
    for frontend in ("bilateral", "grey"):
        grey = torch.zeros((nf, h, w), dtype=torch.uint8, device="cuda")
        for i in range(nf):
            _chain(L, clip[i], w, h, grey[i], w, bilateral=frontend == "bilateral", window=5, ss=1.5, sb=20.0)
        got = eng.video_flow(clip, levels, 9, frontend=frontend, bilateral=(5, 1.5, 20.0))
        assert_same(got.cpu().numpy(), eng.video_flow(grey, levels, 9).cpu().numpy(), f"frontend={frontend}")


def test_refusals(eng, L):
    import torch

    from cuda_optical_flow_2_amd.lib import OfxError
    from cuda_optical_flow_2_amd.parallel import ShardPlan

    w, h, lv = 128, 96, 3
    f3 = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    f1 = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    done = C.c_int()
    # a sharded session: unsupported
    plan = ShardPlan(w, h, lv, 9, 0, 2)
    s = eng.Session(w, h, lv, 9, "lk_float", shard=plan, local_corner=True, stream_batch=2)
    assert L.ofx_session_stream_frontend(s._h, 2, 9, 2.0, 10.0, 0) == 3
    s.close()
    s = eng.Session(w, h, lv, 9, "lk_float", stream_batch=2, borrow_frames=True, two_stage=True)
    # an unsupported window; a bad mode / flag
    for win in (1, 4, 15):
        assert L.ofx_session_stream_frontend(s._h, 2, win, 2.0, 10.0, 0) == 3
    assert L.ofx_session_stream_frontend(s._h, 4, 9, 2.0, 10.0, 0) == 1
    assert L.ofx_session_stream_frontend(s._h, 2, 9, 2.0, 10.0, 8) == 1
    # a colour submit with the front end off
    s.stream_begin()
    assert L.ofx_session_stream_submit_3ch(s._h, f3.data_ptr(), 3 * w, None, C.byref(done)) == 4
    # a setter call after the first frame
    s.stream_frontend("bilateral")
    s.stream_begin()
    s.stream_submit_3ch(f3)
    assert L.ofx_session_stream_frontend(s._h, 2, 9, 2.0, 10.0, 0) == 4
    assert L.ofx_session_stream_frontend(s._h, 0, 0, 0.0, 0.0, 0) == 4
    # mixed submits, both ways
    assert L.ofx_session_stream_submit(s._h, f1.data_ptr(), w, None, C.byref(done)) == 4
    s.stream_begin()
    s.stream_submit(f1)
    assert L.ofx_session_stream_submit_3ch(s._h, f3.data_ptr(), 3 * w, None, C.byref(done)) == 4
    # a bad pitch / alignment
    s.stream_begin()
    assert L.ofx_session_stream_submit_3ch(s._h, f3.data_ptr(), 3 * w - 1, None, C.byref(done)) == 1
    assert L.ofx_session_stream_submit_3ch(s._h, f3.data_ptr() + 1, 3 * w, None, C.byref(done)) == 1
    with pytest.raises(OfxError):
        s.stream_frontend("bilateral", window=11, sigma_s=-1.0)
    s.stream_frontend("off")
    s.close()
    torch.cuda.synchronize()
