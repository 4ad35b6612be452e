"""GPU: camera motion from point matches -- ofx_fit_motion, engine.fit_motion and engine.video_camera_motion -- against
tests/fit_motion_ref.py.  Every comparison is exact: the float64 models by their bits (viewed as int64), the info words, the masks.
Outputs sit in buffers of 0x5A, so that a store outside an output shows."""
import ctypes as C

import numpy as np
import pytest

import fit_motion_ref as R
import klt_ref as K
import test_fit_motion_ref as T
from test_gpu_interp import Guarded

pytestmark = pytest.mark.gpu

OFX_E_INVALID = 1
NAN, INF = float("nan"), float("inf")
MODELS = ("translation", "similarity", "affine")


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cuda_optical_flow_2_amd import engine

    return engine


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def matches(n, size, seed, status=False):
    """n matches of a slightly sheared similarity in a frame of `size`: noise on and off the lattice, outliers, NaN, infinities,
    points outside the frame, duplicates; with `status`, an int32 array in ofx_track_points' encoding around pair 5"""
    w, h = size
    rng = np.random.RandomState(seed + 13 * n)
    p = np.stack([rng.uniform(0, w - 1, n), rng.uniform(0, h - 1, n)], axis=1)
    c = np.array([(w - 1) / 2, (h - 1) / 2])
    A = np.array([[1.01, -0.015], [0.02, 0.995]])
    q = (p - c) @ A.T + c + np.array([0.8, -0.6]) + rng.normal(0, 0.03, (n, 2))
    kind = rng.randint(0, 20, n)
    on = kind < 6                                                # on the lattice, a whole-lattice pan: exact inliers at thr_q = 0
    p[on] = np.rint(p[on] * 32) / 32
    q[on] = p[on] + np.array([1.0 + 3 / 32, -2.0 + 7 / 32])
    out = kind == 6
    q[out] = np.stack([rng.uniform(0, w - 1, out.sum()), rng.uniform(0, h - 1, out.sum())], axis=1)
    p, q = p.astype(np.float32), q.astype(np.float32)
    if n > 8:
        p[kind == 7, 0] = NAN
        q[kind == 8, 1] = INF
        p[kind == 9, 1] = -INF
        q[kind == 10, 0] = np.float32(w - 1) + np.float32(0.25)
        p[kind == 11] = np.float32(-0.03125)
        dup = np.flatnonzero(kind == 12)
        if len(dup):
            p[dup], q[dup] = p[dup[0]], q[dup[0]]                # coincident matches: invalid similarity / affine samples
        p[1], q[1] = (np.float32(w - 1), np.float32(h - 1)), (np.float32(0), np.float32(0))   # the frame's corners are inside
    st = None
    if status:
        st = np.zeros(n, np.int32)
        lost = rng.randint(0, 6, n)
        st[lost == 1] = (4 << 8) | 2
        st[lost == 2] = (5 << 8) | 3
        st[lost == 3] = (6 << 8) | 1
        st[lost == 4] = (400 << 8) | 4
    return p, q, st


_WANT = {}


def want(key, *args, **kw):
    """the referee's answer, computed once per key and shared"""
    if key not in _WANT:
        _WANT[key] = R.fit_motion(*args, **kw)
    return _WANT[key]


# ---- a launch on guarded buffers ------------------------------------------------------------------------------------------------------
def run(eng, items, model, H, thr_q, refits, seed, mask=True, expect=0):
    """one ofx_fit_motion call on items (p, q, status or None, pair, (w, h)); returns [(model float64 [6], info int32 [8], mask uint8
    [n] or None)], having checked that nothing around the outputs was written"""
    import torch

    lib = eng._lib
    prm = lib.FitParams(R.MODELS[model], H, thr_q, refits, seed)
    nbytes = max(int(lib.load().ofx_fit_motion_work_bytes(C.byref(prm))), 8)
    g_model = Guarded(np.float64, len(items), 1, 6, 6, 1)
    g_info = Guarded(np.int32, len(items), 1, 8, 8, 3)
    keep, descs, g_masks = [], (lib.FitDesc * len(items))(), []
    for i, (p, q, st, pair, (w, h)) in enumerate(items):
        n = len(p)
        tp, tq = torch.from_numpy(np.ascontiguousarray(p, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(q, np.float32)).cuda()
        ts = None if st is None else torch.from_numpy(np.ascontiguousarray(st, np.int32)).cuda()
        work = torch.full((nbytes // 8,), NAN, dtype=torch.float64, device="cuda")
        g_mask = Guarded(np.uint8, 1, 1, n, n, 1 + i) if mask else None      # (odd addresses: the mask needs no alignment)
        keep += [tp, tq, ts, work]
        g_masks.append(g_mask)
        descs[i] = lib.FitDesc(tp.data_ptr(), tq.data_ptr(), None if ts is None else ts.data_ptr(), n, pair, w, h, g_model.slot(i), g_info.slot(i),
                               g_mask.ptr if mask else None, work.data_ptr())
    rc = lib.load().ofx_fit_motion(descs, len(items), C.byref(prm), eng._stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, (rc, lib.load().ofx_last_error())
    models, clean_m = g_model.host()
    infos, clean_i = g_info.host()
    assert clean_m and clean_i, "a store outside d_model or d_info"
    out = []
    for i, g in enumerate(g_masks):
        m = None
        if g is not None:
            got, clean = g.host()
            assert clean, f"item {i}: a store outside d_inlier"
            m = got[0, 0]
        out.append((models[i, 0], infos[i, 0], m))
    return out


def check(got, ref, what):
    m, info, mask = got
    wm, winfo, wmask = ref
    assert info.tolist() == winfo.tolist(), f"{what}: info {info.tolist()} vs {winfo.tolist()}"
    assert m.view(np.int64).tolist() == wm.view(np.int64).tolist(), f"{what}: model {m.tolist()} vs {wm.tolist()}"
    if mask is not None:
        assert np.array_equal(mask, wmask), f"{what}: {int((mask != wmask).sum())} mask bytes differ"


# ---- sizes ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 257, 4099])
def test_every_size_equals_the_referee(eng, n):
    size = (192, 128)
    p, q, _ = matches(n, size, 1)
    for model in MODELS:
        got = run(eng, [(p, q, None, 0, size)], model, 64, 32, 2, 9)[0]
        check(got, want(("n", n, model), p, q, size, None, 0, model, 64, 32, 2, 9), f"n={n} {model}")


@pytest.mark.parametrize("H", [1, 7, 64, 513, 4096])
def test_every_hypothesis_count_equals_the_referee(eng, H):
    size = (262, 74)
    p, q, _ = matches(257, size, 2)
    for model in MODELS:
        got = run(eng, [(p, q, None, 0, size)], model, H, 16, 1, 77)[0]
        check(got, want(("H", H, model), p, q, size, None, 0, model, H, 16, 1, 77), f"H={H} {model}")


BATCH_SIZES = [(192, 128), (67, 45), (262, 74), (33, 17), (640, 480), (5, 4), (1, 1), (65536, 3)]


@pytest.mark.parametrize("n_items", [1, 2, 16])
def test_items_of_different_sizes_in_one_launch(eng, n_items):
    ns = [300, 1, 1025, 2, 64, 3, 2049, 65, 5000, 17, 1024, 100, 257, 63, 4099, 7][:n_items]
    items = []
    for i, n in enumerate(ns):
        size = BATCH_SIZES[i % len(BATCH_SIZES)]
        p, q, st = matches(n, size, 30 + i, status=i % 2 == 1)
        items.append((p, q, st, 5 if i % 4 == 1 else 4, size))
    for model in ("similarity", "affine"):
        got = run(eng, items, model, 40, 32, 2, 5)
        for i, (p, q, st, pair, size) in enumerate(items):
            check(got[i], want(("batch", i, model), p, q, size, st, pair, model, 40, 32, 2, 5), f"item {i} of {n_items} {model}")


# ---- parameters -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("thr_q", [0, 32, 1 << 15])
def test_every_model_refit_count_and_radius(eng, model, thr_q):
    size = (192, 128)
    p, q, st = matches(300, size, 3, status=True)
    for refits in range(4):
        use_status, mask = refits % 2 == 0, refits < 2
        got = run(eng, [(p, q, st if use_status else None, 5, size)], model, 48, thr_q, refits, 1234, mask=mask)[0]
        ref = want(("prm", model, thr_q, refits), p, q, size, st if use_status else None, 5, model, 48, thr_q, refits, 1234)
        check(got, ref, f"{model} thr_q={thr_q} refits={refits}")
        if thr_q == 0 and model != "translation":
            assert ref[1][0] == R.FIT_OK and ref[1][4] > 30, "the whole-lattice pan is found at radius 0"


@pytest.mark.parametrize("pair", [0, 3, 4, 5, 6, 399, 400, 1 << 22])
def test_the_status_rule_on_both_sides_of_a_loss(eng, pair):
    size = (192, 128)
    p, q, st = matches(300, size, 4, status=True)
    usable = {int(R.lattice(p, q, size, st, k)[2].sum()) for k in (3, 4, 5, 6, 399, 400)}
    assert len(usable) == 5, "every loss changes the usable matches"
    got = run(eng, [(p, q, st, pair, size)], "similarity", 32, 32, 1, 0)[0]
    check(got, want(("pair", pair), p, q, size, st, pair, "similarity", 32, 32, 1, 0), f"pair={pair}")


@pytest.mark.parametrize("seed", [0, 1, 0xFFFFFFFF])
def test_seeds(eng, seed):
    size = (192, 128)
    p, q, _ = matches(300, size, 5)
    got = run(eng, [(p, q, None, 0, size)], "affine", 64, 2, 0, seed)[0]
    check(got, want(("seed", seed), p, q, size, None, 0, "affine", 64, 2, 0, seed), f"seed={seed}")


# ---- special inputs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(T.degenerate_cases()))
def test_few_and_degenerate(eng, name):
    p, q, model, status, usable = T.degenerate_cases()[name]
    ref = R.fit_motion(p, q, T.SIZE, model=model, hypotheses=32, thr_q=0, refits=1, seed=1)
    assert ref[1][0] == status
    check(run(eng, [(p, q, None, 0, T.SIZE)], model, 32, 0, 1, 1)[0], ref, name)


def test_equal_counts_go_to_the_smallest_j(eng):
    p = np.tile(np.float32([[30.0, 30.0]]), (20, 1))
    q = p.copy()
    q[:10, 0] += 1
    q[10:, 1] += 1
    for seed in range(6):
        ref = R.fit_motion(p, q, T.SIZE, model="translation", hypotheses=16, thr_q=0, refits=0, seed=seed)
        assert ref[1][3] == 0 and ref[1][4] == 10
        check(run(eng, [(p, q, None, 0, T.SIZE)], "translation", 16, 0, 0, seed)[0], ref, f"tie, seed {seed}")


def test_nothing_but_unusable_matches_of_every_kind(eng):
    size = (67, 45)
    bad = np.float32([[NAN, 1], [1, NAN], [INF, 1], [1, -INF], [-0.5, 1], [1, -0.5], [66.5, 1], [1, 44.5], [1e30, 1], [-1e-30, 1]])
    good = np.tile(np.float32([[5.0, 6.0]]), (len(bad), 1))
    for p, q in ((bad, good), (good, bad)):
        ref = R.fit_motion(p, q, size, model="translation", hypotheses=8, thr_q=32, refits=1, seed=0)
        assert ref[1].tolist() == [R.FIT_FEW, 0, 0, -1, 0, 0, 0, 0]
        check(run(eng, [(p, q, None, 0, size)], "translation", 8, 32, 1, 0)[0], ref, "unusable")
    # -0.0 and the last pixel are inside
    edge = np.float32([[-0.0, 44.0], [66.0, 0.0]])
    ref = R.fit_motion(edge, edge[::-1].copy(), size, model="similarity", hypotheses=8, thr_q=32, refits=1, seed=0)
    assert ref[1][1] == 2
    check(run(eng, [(edge, edge[::-1].copy(), None, 0, size)], "similarity", 8, 32, 1, 0)[0], ref, "edges")


def test_a_refused_call_writes_nothing(eng):
    size = (192, 128)
    p, q, _ = matches(65, size, 6)
    for kw in (dict(H=4097), dict(thr_q=-1), dict(refits=4), dict(size=(0, 128)), dict(size=(192, (1 << 16) + 1))):
        got = run(eng, [(p, q, None, 0, size), (p, q, None, 0, kw.get("size", size))], "similarity", kw.get("H", 16), kw.get("thr_q", 32),
                  kw.get("refits", 1), 0, expect=OFX_E_INVALID)
        for m, info, mask in got:
            assert (m.view(np.uint8) == 0x5A).all() and (info.view(np.uint8) == 0x5A).all() and (mask == 0x5A).all(), kw


# ---- large sums -------------------------------------------------------------------------------------------------------------------------
def test_sums_near_2_to_the_60_round_to_nearest_even(eng):
    """2^20 matches at the corners of a 65536 x 65536 frame, drawn towards the centre by about two pixels: sum ux^2 is near 2^60, so
    the int64 -> float64 conversions of the refit round"""
    n, size = 1 << 20, (1 << 16, 1 << 16)
    rng = np.random.RandomState(8)
    corner = rng.randint(0, 4, n)
    p = np.stack([(corner & 1) * 65535.0, (corner >> 1) * 65535.0], axis=1)
    q = 32767.5 + (p - 32767.5) * (1 - 2.0 ** -14) + rng.randint(-3, 4, (n, 2)) / 32.0
    p, q = p.astype(np.float32), np.clip(q, 0, 65535).astype(np.float32)
    u, v, ok = R.lattice(p, q, size)
    assert ok.all()
    sxvx = int((u[:, 0] * v[:, 0]).sum())
    assert sxvx > 1 << 59 and int(float(sxvx)) != sxvx, "a sum that float64 cannot hold"
    for model in ("similarity", "affine"):
        ref = R.fit_motion(p, q, size, model=model, hypotheses=4, thr_q=32, refits=2, seed=0)
        assert ref[1][0] == R.FIT_OK and ref[1][6] == 2 and ref[1][5] > n // 2
        check(run(eng, [(p, q, None, 0, size)], model, 4, 32, 2, 0)[0], ref, f"2^20 matches, {model}")


# ---- the calls on arrays and clips ------------------------------------------------------------------------------------------------------
def test_engine_fit_motion(eng):
    import torch

    size = (192, 128)
    p, q, st = matches(300, size, 7, status=True)
    for model in MODELS:
        ref = R.fit_motion(p, q, size, st, 5, model, 100, 48, 2, 21)
        m, info, mask = eng.fit_motion(p, q, size, status=st, pair=5, model=model, hypotheses=100, thr=1.5, refits=2, seed=21, return_inliers=True)
        assert isinstance(m, np.ndarray) and m.dtype == np.float64 and info.dtype == np.int32 and mask.dtype == np.uint8
        check((m, info, mask), ref, f"host arrays, {model}")
        out = eng.fit_motion(torch.from_numpy(p).cuda(), torch.from_numpy(q).cuda(), size, status=torch.from_numpy(st).cuda(), pair=5, model=model,
                             hypotheses=100, thr=1.5, refits=2, seed=21)
        assert len(out) == 2 and all(t.is_cuda for t in out)
        check((out[0].cpu().numpy(), out[1].cpu().numpy(), None), ref, f"CUDA tensors, {model}")
    m, info = eng.fit_motion(p, q, size)
    check((m, info, None), R.fit_motion(p, q, size), "defaults")
    with pytest.raises(eng.OfxError):
        eng.fit_motion(p, q, size, hypotheses=5000)


def camera_clip():
    """six 192 x 128 crops of one texture: whole-pixel pans, then a sub-pixel drift"""
    offs = [(0, 0), (4, 4), (1, 2), (3, 0)]
    big = K.cosine_texture(224, 160)
    frames = [big[16 + oy:16 + oy + 128, 16 + ox:16 + ox + 192] for ox, oy in offs]
    frames += [K.cosine_texture(224, 160, -(3.0 + 0.4 * k), -0.3 * k)[16:144, 16:208] for k in (1, 2)]      # on from the crop at (3, 0)
    return np.ascontiguousarray(np.stack(frames))


@pytest.mark.parametrize("model,reseed", [("similarity", 16), ("affine", 2), ("translation", 1)])
def test_video_camera_motion_equals_the_referee_on_the_devices_own_tracks(eng, model, reseed):
    import torch

    clip = camera_clip()
    N, H, W = clip.shape
    frames = torch.from_numpy(clip).cuda()
    models, info = eng.video_camera_motion(frames, model=model, reseed=reseed, hypotheses=64, thr=0.5, refits=2, seed=3)
    assert models.is_cuda and tuple(models.shape) == (N - 1, 6) and models.dtype == torch.float64
    assert info.is_cuda and tuple(info.shape) == (N - 1, 8) and info.dtype == torch.int32
    models, info = models.cpu().numpy(), info.cpu().numpy()
    for f0 in range(0, N - 1, reseed):
        f1 = min(f0 + reseed, N - 1)
        pos, status, _ = eng.video_klt(frames[f0:f1 + 1].contiguous(), None, 3, 9, 16, 16)
        pos, status = pos.cpu().numpy(), status.cpu().numpy()
        assert pos.shape[1] > 20
        for b in range(f1 - f0):
            ref = R.fit_motion(pos[b], pos[b + 1], (W, H), status, b + 1, model, 64, 16, 2, 3)
            check((models[f0 + b], info[f0 + b], None), ref, f"pair {f0 + b + 1}")
            assert ref[1][0] == R.FIT_OK and ref[1][5] > 20
    # the pans of the crops (frames 0 .. 3) and the drift after them, to the 0.1 px at the frame's corners that the referee's own
    # accuracy test asks: 0.1 px in the shift, 0.1 px over the 96 px from the centre to a corner in the linear part
    for pair, (dx, dy) in enumerate([(-4, -4), (3, 2), (-2, 2), (-0.4, -0.3), (-0.4, -0.3)]):
        m = models[pair]
        cx, cy = (W - 1) / 2, (H - 1) / 2
        assert abs(m[0] * cx + m[1] * cy + m[2] - cx - dx) <= 0.1 and abs(m[3] * cx + m[4] * cy + m[5] - cy - dy) <= 0.1, (pair, m)
        assert np.abs(m[[0, 1, 3, 4]] - [1, 0, 0, 1]).max() <= 0.1 / 96, (pair, m)


def test_a_clip_without_features_gets_the_identity_and_few(eng):
    import torch

    frames = torch.full((3, 64, 96), 128, dtype=torch.uint8, device="cuda")
    models, info = eng.video_camera_motion(frames, hypotheses=8)
    assert models.cpu().numpy().tolist() == [list(R.IDENTITY)] * 2
    assert info.cpu().numpy().tolist() == [[R.FIT_FEW, 0, 0, -1, 0, 0, 0, 0]] * 2
