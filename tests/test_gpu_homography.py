"""GPU: planar homography from point matches -- ofx_fit_homography and engine.fit_homography -- against tests/homography_ref.py.
Every comparison is exact: the float64 models by their bits (viewed as int64), the info words, the masks.  Outputs sit in buffers
of 0x5A, so that a store outside an output shows."""
import ctypes as C

import numpy as np
import pytest

import homography_cases as Cs
import homography_ref as R
import test_homography_ref as T
from fit_motion_ref import FIT_DEGENERATE, FIT_FEW, FIT_OK, lattice
from test_gpu_interp import Guarded

pytestmark = pytest.mark.gpu

OFX_E_INVALID = 1
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cuda_optical_flow_2_amd import engine

    return engine


_WANT = {}


def want(key, *args, **kw):
    """the referee's answer, computed once per key and shared"""
    if key not in _WANT:
        _WANT[key] = R.fit_homography(*args, **kw)
    return _WANT[key]


def run(eng, items, H, thr_q, refits, seed, mask=True, expect=0, model=3):
    """one ofx_fit_homography call on items (p, q, status or None, pair, (w, h)); returns [(model float64 [9], info int32 [8], mask
    uint8 [n] or None)], having checked that nothing around the outputs was written"""
    import torch

    lib = eng._lib
    prm = lib.FitParams(model, H, thr_q, refits, seed)
    nbytes = max(int(lib.load().ofx_fit_homography_work_bytes(C.byref(prm))), 8)
    g_model = Guarded(np.float64, len(items), 1, 9, 9, 1)
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
    rc = lib.load().ofx_fit_homography(descs, len(items), C.byref(prm), eng._stream_ptr())
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
@pytest.mark.parametrize("n", [4, 5, 63, 64, 65, 1023, 1024, 1025, 4099])
def test_every_size_equals_the_referee(eng, n):
    size = (192, 128)
    p, q, _ = Cs.matches(n, size, 1)
    ref = want(("n", n), p, q, size, None, 0, 64, 32, 2, 9)
    check(run(eng, [(p, q, None, 0, size)], 64, 32, 2, 9)[0], ref, f"n={n}")
    assert n < 63 or (ref[1][0] == FIT_OK and ref[1][6] == 2 and ref[1][5] > n // 2)


@pytest.mark.parametrize("H", [1, 31, 32, 33, 256])
def test_every_hypothesis_count_equals_the_referee(eng, H):
    size = (262, 74)
    p, q, _ = Cs.matches(257, size, 2)
    check(run(eng, [(p, q, None, 0, size)], H, 16, 1, 77)[0], want(("H", H), p, q, size, None, 0, H, 16, 1, 77), f"H={H}")


BATCH_SIZES = [(192, 128), (67, 45), (262, 74), (33, 17), (640, 480), (97, 61), (9, 9), (65536, 300)]


@pytest.mark.parametrize("n_items", [1, 2, 16])
def test_items_of_different_sizes_in_one_launch(eng, n_items):
    ns = [300, 4, 1025, 5, 64, 7, 2049, 65, 3000, 17, 1024, 100, 257, 63, 4099, 9][:n_items]
    items = []
    for i, n in enumerate(ns):
        size = BATCH_SIZES[i % len(BATCH_SIZES)]
        p, q, st = Cs.matches(n, size, 30 + i, status=i % 2 == 1)
        items.append((p, q, st, 5 if i % 4 == 1 else 4, size))
    got = run(eng, items, 40, 32, 2, 5)
    for i, (p, q, st, pair, size) in enumerate(items):
        check(got[i], want(("batch", i), p, q, size, st, pair, 40, 32, 2, 5), f"item {i} of {n_items}")


# ---- parameters -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr_q", [0, 32, 1 << 15])
def test_every_refit_count_and_radius(eng, thr_q):
    size = (192, 128)
    p, q, st = Cs.matches(300, size, 3, status=True)
    for refits in range(4):
        use_status, mask = refits % 2 == 0, refits < 2
        got = run(eng, [(p, q, st if use_status else None, 5, size)], 48, thr_q, refits, 1234, mask=mask)[0]
        ref = want(("prm", thr_q, refits), p, q, size, st if use_status else None, 5, 48, thr_q, refits, 1234)
        check(got, ref, f"thr_q={thr_q} refits={refits}")
        assert ref[1][0] == FIT_OK and (thr_q == 0 or ref[1][6] == refits)


@pytest.mark.parametrize("pair", [3, 4, 5, 6, 399, 400])
def test_the_status_rule_on_both_sides_of_a_loss(eng, pair):
    size = (192, 128)
    p, q, st = Cs.matches(300, size, 4, status=True)
    usable = {int(lattice(p, q, size, st, k)[2].sum()) for k in (3, 4, 5, 6, 399, 400)}
    assert len(usable) == 5, "every loss changes the usable matches"
    check(run(eng, [(p, q, st, pair, size)], 32, 32, 1, 0)[0], want(("pair", pair), p, q, size, st, pair, 32, 32, 1, 0), f"pair={pair}")


@pytest.mark.parametrize("seed", [0, 1, 0xFFFFFFFF])
def test_seeds(eng, seed):
    size = (192, 128)
    p, q, _ = Cs.matches(300, size, 5)
    check(run(eng, [(p, q, None, 0, size)], 64, 2, 0, seed)[0], want(("seed", seed), p, q, size, None, 0, 64, 2, 0, seed), f"seed={seed}")


# ---- special inputs ---------------------------------------------------------------------------------------------------------------------
def test_few_degenerate_and_the_w_rule(eng):
    size = (97, 61)
    p, q = Cs.noisy_matches(40, T.SIZE, 1, 0.0)
    p[3:, 0] = np.nan
    cases = {"three usable": (p, q, T.SIZE, FIT_FEW), "the middle row": T.row_matches(size) + (size, FIT_DEGENERATE), "a bow tie": T.bow_tie() + (T.SIZE, FIT_DEGENERATE),
             "four dyadic matches": Cs.dyadic_four() + (FIT_OK,)}
    for name, (p, q, sz, status) in cases.items():
        ref = R.fit_homography(p, q, sz, hypotheses=32, thr_q=1, refits=1, seed=1)
        assert ref[1][0] == status, name
        check(run(eng, [(p, q, None, 0, sz)], 32, 1, 1, 1)[0], ref, name)


def test_equal_counts_go_to_the_smallest_j(eng):
    p, q = T.exact_pan()
    for seed in range(3):
        ref = R.fit_homography(p, q, T.SIZE, hypotheses=24, thr_q=2, refits=0, seed=seed)
        assert ref[1][4] == 60
        check(run(eng, [(p, q, None, 0, T.SIZE)], 24, 2, 0, seed)[0], ref, f"tie, seed {seed}")


def test_nothing_but_unusable_matches_of_every_kind(eng):
    size = (67, 45)
    bad = np.float32([[NAN, 1], [1, NAN], [INF, 1], [1, -INF], [-0.5, 1], [1, -0.5], [66.5, 1], [1, 44.5], [1e30, 1], [-1e-30, 1]])
    good = np.tile(np.float32([[5.0, 6.0]]), (len(bad), 1))
    for p, q in ((bad, good), (good, bad)):
        ref = R.fit_homography(p, q, size, hypotheses=8, thr_q=32, refits=1, seed=0)
        assert ref[1].tolist() == [FIT_FEW, 0, 0, -1, 0, 0, 0, 0]
        check(run(eng, [(p, q, None, 0, size)], 8, 32, 1, 0)[0], ref, "unusable")


def test_a_refused_call_writes_nothing(eng):
    size = (192, 128)
    p, q, _ = Cs.matches(65, size, 6)
    for kw in (dict(H=4097), dict(thr_q=-1), dict(refits=4), dict(size=(0, 128)), dict(size=(192, (1 << 16) + 1)), dict(model=2)):
        got = run(eng, [(p, q, None, 0, size), (p, q, None, 0, kw.get("size", size))], kw.get("H", 16), kw.get("thr_q", 32), kw.get("refits", 1), 0,
                  expect=OFX_E_INVALID, model=kw.get("model", 3))
        for m, info, mask in got:
            assert (m.view(np.uint8) == 0x5A).all() and (info.view(np.uint8) == 0x5A).all() and (mask == 0x5A).all(), kw


# ---- wide sums --------------------------------------------------------------------------------------------------------------------------
def test_sums_that_need_128_bits(eng):
    """2048 matches near the corners of a 65536 x 65536 frame: the degree-4 sums pass 2^90, the degree-3 sums 2^64 with both signs,
    so both halves, the carry between them and the sign extension all take part"""
    p, q, size = Cs.wide_sum_matches()
    u, v, ok = lattice(p, q, size)
    assert ok.all()
    ref = R.fit_homography(p, q, size, hypotheses=4, thr_q=32, refits=2, seed=0)
    s = R.sums(u, v, ref[2].astype(bool))
    assert s["SxxR"].bit_length() > 90 and s["SxxX"] < -(1 << 64) and s["SxxY"] > 1 << 64 and s["SxR"] < -(1 << 64)
    terms = [int(u[i][0]) * int(u[i][1]) * int(v[i][0]) for i in range(len(u))]
    assert min(terms) < -(1 << 58) and max(terms) > 1 << 58, "the mixed terms change sign"
    assert ref[1][0] == FIT_OK and ref[1][6] == 2 and ref[1][5] > 1024
    check(run(eng, [(p, q, None, 0, size)], 4, 32, 2, 0)[0], ref, "wide sums")


# ---- the call on arrays -----------------------------------------------------------------------------------------------------------------
def test_engine_fit_homography(eng):
    import torch

    size = (192, 128)
    p, q, st = Cs.matches(300, size, 7, status=True)
    ref = R.fit_homography(p, q, size, st, 5, 100, 48, 2, 21)
    m, info, mask = eng.fit_homography(p, q, size, status=st, pair=5, hypotheses=100, thr=1.5, refits=2, seed=21, return_inliers=True)
    assert isinstance(m, np.ndarray) and m.dtype == np.float64 and m.shape == (9,) and info.dtype == np.int32 and mask.dtype == np.uint8
    check((m, info, mask), ref, "host arrays")
    out = eng.fit_homography(torch.from_numpy(p).cuda(), torch.from_numpy(q).cuda(), size, status=torch.from_numpy(st).cuda(), pair=5, hypotheses=100, thr=1.5,
                             refits=2, seed=21)
    assert len(out) == 2 and all(t.is_cuda for t in out)
    check((out[0].cpu().numpy(), out[1].cpu().numpy(), None), ref, "CUDA tensors")
    m, info = eng.fit_homography(p, q, size)
    check((m, info, None), R.fit_homography(p, q, size), "defaults")
    assert Cs.corner_error(m, Cs.true_model(size), size) <= 0.25
    with pytest.raises(eng.OfxError):
        eng.fit_homography(p, q, size, hypotheses=5000)


def test_engine_fit_homography_on_the_devices_own_tracks(eng):
    import torch

    import klt_ref as K

    big = K.cosine_texture(224, 160)
    clip = np.ascontiguousarray(np.stack([big[16:144, 16:208], big[18:146, 19:211]]))
    frames = torch.from_numpy(clip).cuda()
    pos, status, _ = eng.video_klt(frames, None, 3, 9, 16, 16)
    assert pos.shape[1] > 20
    m, info = eng.fit_homography(pos[0], pos[1], (192, 128), status=status, pair=1, hypotheses=64, thr=0.5, seed=3)
    ref = R.fit_homography(pos[0].cpu().numpy(), pos[1].cpu().numpy(), (192, 128), status.cpu().numpy(), 1, 64, 16, 2, 3)
    check((m.cpu().numpy(), info.cpu().numpy(), None), ref, "tracks")
    assert ref[1][0] == FIT_OK and ref[1][5] > 20
    assert Cs.corner_error(m.cpu().numpy(), (1.0, 0.0, -3.0, 0.0, 1.0, -2.0, 0.0, 0.0, 1.0), (192, 128)) <= 0.1
