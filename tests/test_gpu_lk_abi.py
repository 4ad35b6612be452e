"""GPU: the stateless launch ABI of include/ofx.h on caller-owned buffers -- ofx_lk_levels (plain levels, the fused shift, several
descriptors, row windows, the determinant guard, accumulate in compat_cpu and on the buffer march, d_warp_out, d_warp_status),
ofx_lk_level_sums, ofx_shift_levels, ofx_warp_levels, ofx_downsample_1ch, ofx_pyramid_1ch, ofx_corner_flows, and a whole pair made of
nothing but these calls -- against the CPU oracle, by the bits.

What the header allows and a session never does: a pitch of (w + 3) & ~3, planes that are only 4-byte aligned, flows that are only
8-byte aligned, pad columns that hold anything.  Every input lies inside a larger allocation (tests/lk_abi_child.py: at least 256
bytes before it, max(256, 2 * pitch) after it) and every case runs with the three surroundings of tests/test_gpu_interp.py, pad
columns included: an over-read lands in the test's own memory and shows as a changed result.  Outputs are windows of buffers of
0x5A: flow rows outside [out_y0, out_y1), the bytes around a buffer and the pad bytes the header says are left alone must still hold
it.  Cases, frames and expected values: tests/lk_abi_cases.py (tests/test_lk_abi_ref.py shows they are what they claim)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import dense_ref
import iter_hard as ih
import lk_abi_cases as K
import lk_abi_child as B
from lk_abi_child import Item, key, launch_lk, results

pytestmark = pytest.mark.gpu

F32 = np.float32
RUNS = B.RUNS
CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lk_abi_child.py")
CHILD_LIMIT = 300   # seconds; the child needs a few


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cuda_optical_flow_2_amd import engine

    return engine


def same(got, want, what):
    """floats by their bits (two NaNs are the same value: dense_ref.same_bits), integers as they are"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype}{got.shape} vs {want.dtype}{want.shape}"
    ok = dense_ref.same_bits(got, want) if got.dtype == np.float32 else got == want
    if not ok.all():
        bad = np.argwhere(~ok)
        raise AssertionError(f"{what}: {len(bad)}/{got.size} differ, first at {bad[:3].tolist()}: {got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}")


def pad4(w):
    return (w + 3) & ~3


def fast_level(oracle, prev, nxt, win, old, got, what):
    """lk_float_fast: the project's 1-ulp rule (iter_hard.check_fast_step) for one launch on whole-level arrays: got against
    old + the exact level of (prev, warp(nxt, old)).  old = None: a launch that sets the flow (a zero flow warps nothing)."""
    ih.check_fast_step(oracle, prev, nxt, win, np.zeros(got.shape, F32) if old is None else old, got, what)


# ---- a. plain levels --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", K.PLAIN, ids=[c.id for c in K.PLAIN])
def test_plain_levels(eng, oracle, c):
    p, n = K.frames(c.w, c.h, c.kind)
    nr, want = K.plain_want(oracle, c)
    y0, y1 = (c.rows[2], c.rows[3]) if c.rows else (0, c.h)
    items = [Item(p, n, c.geo, run, rows=c.rows, uv=K.uv_of(c.uv, c.w), min_det=c.min_det) for run in RUNS]
    for it in items:
        launch_lk(eng, [it], c.win, c.mode)
    got = results(items)
    for run, r in zip(RUNS, got):
        what = f"{c.id} run {run}"
        assert r["clean"], f"{what}: flow rows outside [out_y0, out_y1) or bytes around the flow were written"
        if c.mode != "lk_float_fast":
            same(r["flow"], want[y0:y1], what)
        elif run == 0:
            full = want.copy()
            full[y0:y1] = r["flow"]
            fast_level(oracle, p, nr, c.win, None, full, what)
        else:
            same(r["flow"], got[0]["flow"], what + " against run 0")
    if c.min_det:
        mask = ih.guarded_mask(oracle, p, c.win, c.min_det)[y0:y1]
        assert (got[0]["flow"][mask] == 0).all() and 0 < int(mask.sum()) < mask.size


def _multi(oracle, mode, min_det):
    out = []
    for (w, h, rows) in K.MULTI:
        p, n = K.frames(w, h)
        out.append((p, n, rows, K.level_ref(oracle, p, n, K.MULTI_WIN, mode, min_det)))
    return out


@pytest.mark.parametrize("mode", ["lk_float", "compat_cpu"])
@pytest.mark.parametrize("order", list(K.MULTI_ORDERS))
def test_three_descriptors_in_one_launch_and_whose_min_det_counts(eng, oracle, mode, order):
    """one launch of three levels of different sizes, one of them empty; min_det is levels[0]'s, also when levels[0] is the empty
    one: each order runs with (first, others) = (MIN_DET, 0) and (0, MIN_DET)"""
    idx = K.MULTI_ORDERS[order]
    for first, others in ((ih.MIN_DET, 0.0), (0.0, ih.MIN_DET)) if mode == "lk_float" else ((0.0, 0.0),):
        levels = _multi(oracle, mode, first)
        for run in RUNS:
            items = [Item(levels[i][0], levels[i][1], K.geo(i + run), run, rows=levels[i][2], min_det=first if pos == 0 else others)
                     for pos, i in enumerate(idx)]
            launch_lk(eng, items, K.MULTI_WIN, mode)
            for i, it, r in zip(idx, items, results(items)):
                what = f"{order} {mode} min_det {first}/{others} run {run} level {K.MULTI[i][:2]}"
                assert r["clean"], f"{what}: bytes outside the out rows were written"
                rows = levels[i][2]
                same(r["flow"], levels[i][3][rows[2]:rows[3]] if rows else levels[i][3], what)


def test_level_sums_on_a_row_window_with_a_tight_pitch(eng, oracle):
    from test_gpu_interp import Guarded

    c = K.SUMS
    p, n = K.frames(c.w, c.h)
    want = K.sums_ref(oracle, p, n, c.win)
    row0, rows, y0, y1, f0 = c.rows
    lib = eng._lib
    for run in RUNS:
        it = Item(p, n, c.geo, run, rows=c.rows)
        out = Guarded(np.int32, 5, y1 - f0, c.w, c.w, 65, (y1 - f0) * c.w)
        g = lib.Geom(c.w, c.h, it.pitch, row0, rows, y0, y1)
        eng.check(lib.load().ofx_lk_level_sums(it.prev.ptr, it.next.ptr, C.byref(g), c.win, lib.MODES[c.mode], out.ptr, f0, eng._stream_ptr()), "ofx_lk_level_sums")
        import torch

        torch.cuda.synchronize()
        got, clean = out.host()
        assert clean and (got[:, :y0 - f0] == 0x5A5A5A5A).all(), f"run {run}: rows before out_y0 or bytes around the sums were written"
        same(got[:, y0 - f0:].astype(F32), want[:, y0:y1], f"sums run {run}")


# ---- b. accumulate ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("acc", K.ACC_COMPAT, ids=[a.id for a in K.ACC_COMPAT])
def test_accumulate_in_compat_cpu(eng, oracle, acc):
    """lk_level_kernel's MAY_ACC path: d_flow += result with the old flow holding NaN, +-Inf, 1e30 and -0.0"""
    for run in RUNS:
        items, wants = [], []
        for (w, h, rows, g) in acc.items:
            p, n = K.frames(w, h)
            old, want = K.acc_compat_want(oracle, w, h, acc.win)
            items.append(Item(p, n, g, run, rows=rows, old=old))
            wants.append(want[rows[2]:rows[3]] if rows else want)
        launch_lk(eng, items, acc.win, "compat_cpu")
        for (w, h, _, _), r, want in zip(acc.items, results(items), wants):
            assert r["clean"], f"{acc.id} {w}x{h} run {run}: bytes outside the out rows were written"
            same(r["flow"], want, f"{acc.id} {w}x{h} run {run}")


@pytest.mark.parametrize("case", K.ITER_UV, ids=lambda c: f"{c[0]}x{c[1]}-win{c[2]}-uv_{c[3]}" + ("-warp" if c[4] else ""))
def test_accumulate_through_the_fused_shift(eng, oracle, case):
    """accumulate (and d_warp_out) with d_uv: the buffer march reads next through the shift vector"""
    w, h, win, uv, warp, g = case
    p, n, old, want = K.iter_uv_want(oracle, w, h, win, uv)
    items = [Item(p, n, g, run, uv=K.uv_of(uv, w), old=old, warp_src=n if warp else None) for run in RUNS]
    for it in items:
        launch_lk(eng, [it], win, "lk_float")
    for run, r in zip(RUNS, results(items)):
        what = f"{w}x{h} win {win} uv {uv} run {run}"
        assert r["clean"], f"{what}: bytes around the flow were written"
        same(r["flow"], want, what)
        if warp:
            assert r["warp_clean"], f"{what}: bytes around d_warp_out were written"
            same(r["warp"][:, :w], oracle.warp_bilinear_u8(n, want, K.ITER_SCALE), what + ": d_warp_out")
            assert (r["warp"][:, pad4(w):] == B.FILL).all(), f"{what}: pad bytes of d_warp_out were written"


def check_iter_case(oracle, got, variant, shape, mode):
    """one whole-level launch of the buffer march, every run: the flow against the oracle (lk_float_fast: the 1-ulp rule on run 0,
    the other runs equal to it), nothing written outside it, and d_warp_out = the oracle's warp of d_warp_src by the flow the
    launch left, its pad bytes as include/ofx.h says"""
    w, h, win = shape
    d = K.iter_inputs(oracle, w, h, win)
    old = None if variant == "set+warp" else d["old"]
    want = d["delta"] if old is None else K.add_ref(old, d["delta"])
    first = None
    for run in RUNS:
        r = {name: got[key(variant, f"{w}x{h}-win{win}", mode, f"run{run}", name)] for name in ("flow", "clean") + (("warp", "warp_clean") if variant != "add" else ())}
        what = f"{variant} {w}x{h} win {win} {mode} run {run}"
        assert r["clean"], f"{what}: bytes around the flow were written"
        if mode == "lk_float":
            same(r["flow"], want, what)
        elif first is None:
            first = r["flow"]
            fast_level(oracle, d["prev"], d["next"] if old is not None else d["fed"], win, old, first, what)
        else:
            same(r["flow"], first, what + " against run 0")
        if variant != "add":
            assert r["warp_clean"], f"{what}: bytes around d_warp_out were written"
            same(r["warp"][:, :w], oracle.warp_bilinear_u8(d["next"], r["flow"], K.ITER_SCALE), what + ": d_warp_out")
            assert (r["warp"][:, pad4(w):] == B.FILL).all(), f"{what}: pad bytes of d_warp_out from column (w + 3) & ~3 on were written"


def check_rows_case(oracle, got, c, mode):
    """kIterAddWarpRows: flow and warped rows of the window against the whole-level launch of the same inputs and against the
    restated nearest-row rule; the status word"""
    d = K.rows_inputs(oracle, c)
    row0, rows, y0, y1, f0 = c["rows"]
    w = c["w"]
    for run in RUNS:
        g = lambda tag, name: got[key("rows", c["id"], mode, f"run{run}", tag, name)]   # noqa: E731
        what = f"{c['id']} {mode} run {run}"
        if mode == "lk_float":
            same(g("whole", "flow"), d["flow"], what + ": whole level")
            same(g("whole", "warp")[:, :w], d["warped"], what + ": whole level, d_warp_out")
        assert g("window", "clean") and g("window", "warp_clean"), f"{what}: bytes outside the outputs were written"
        flow = g("whole", "flow")
        same(g("window", "flow"), flow[y0:y1], what + ": flow of the window")
        ref, needs = K.warp_rows(d["next"], flow, K.ITER_SCALE, row0, row0 + rows)
        plane = g("window", "warp")
        keep = ~needs[y0:y1]
        assert 2 * int(keep.sum()) >= keep.size
        out_rows = plane[y0 - row0:y1 - row0, :w]
        same(out_rows[keep], g("whole", "warp")[y0:y1, :w][keep], what + ": pixels that need no row outside the window")
        same(out_rows, ref[y0:y1], what + ": nearest row held")
        assert (plane[:y0 - row0] == B.FILL).all() and (plane[y1 - row0:] == B.FILL).all(), f"{what}: rows of d_warp_out that are no out rows were written"
        assert (plane[:, pad4(w):] == B.FILL).all(), f"{what}: pad bytes of d_warp_out were written"
        missing = bool(needs[y0:y1].any())
        assert missing == (c is K.ROWS_MISS), what
        assert int(g("window", "status")) == c["preload"] | (int(missing) << c["bit"]), f"{what}: status {int(g('window', 'status')):#x}"


@pytest.fixture(scope="module")
def iter_runs(eng, oracle):
    return B.run_iter_cases(eng, oracle, {})


_ITER_PARAMS = [(v, s, m) for m in K.ITER_MODES for v in K.ITER_VARIANTS for s in K.ITER_SHAPES]
_ITER_IDS = [f"{v}-{s[0]}x{s[1]}-win{s[2]}-{m}" for v, s, m in _ITER_PARAMS]


@pytest.mark.parametrize("variant,shape,mode", _ITER_PARAMS, ids=_ITER_IDS)
def test_accumulate_and_warp_out_on_the_buffer_march(oracle, iter_runs, variant, shape, mode):
    check_iter_case(oracle, iter_runs, variant, shape, mode)


@pytest.mark.parametrize("mode", K.ITER_MODES)
@pytest.mark.parametrize("c", [K.ROWS_NO_MISS, K.ROWS_MISS], ids=lambda c: c["id"])
def test_accumulate_and_warp_out_on_a_row_window(oracle, iter_runs, c, mode):
    check_rows_case(oracle, iter_runs, c, mode)


@pytest.fixture(scope="module")
def deep_runs(tmp_path_factory):
    """the same launches in the deep-fetch form: one fresh child process started with OFX_ITER_DMA=1, under a time limit"""
    import torch

    try:
        torch.cuda.synchronize()
    except RuntimeError as e:       # (a fault in this process: nothing more is started on the device)
        pytest.fail(f"the child is not started: the device reported {e}")
    path = str(tmp_path_factory.mktemp("lk_abi_deep") / "out.npz")
    env = dict(os.environ, OFX_ITER_DMA="1")
    env.pop("OFX_LK_DMA", None)
    try:
        r = subprocess.run([sys.executable, CHILD, path], env=env, timeout=CHILD_LIMIT, capture_output=True)
    except subprocess.TimeoutExpired:
        pytest.fail(f"the child did not end within {CHILD_LIMIT} s")
    out, err = r.stdout.decode(errors="replace"), r.stderr.decode(errors="replace")
    if r.returncode != 0 or not out.rstrip().endswith("lk abi ok"):
        pytest.fail(f"the child ended with status {r.returncode}: {out[-500:]} {err[-2000:]}")
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def test_the_deep_fetch_form_of_the_same_launches(oracle, deep_runs):
    """stops at the first failure"""
    assert len(deep_runs) > 0
    for variant, shape, mode in _ITER_PARAMS:
        check_iter_case(oracle, deep_runs, variant, shape, mode)
    for mode in K.ITER_MODES:
        for c in (K.ROWS_NO_MISS, K.ROWS_MISS):
            check_rows_case(oracle, deep_runs, c, mode)


# ---- c. refusals ------------------------------------------------------------------------------------------------------------------

def test_refusals_happen_on_the_host(eng):
    """every address lies inside one real allocation: a call that were wrongly accepted would still run inside it"""
    import torch

    lib = eng._lib
    L = lib.load()
    arena = torch.zeros(4 << 20, dtype=torch.uint8, device="cuda")
    assert arena.data_ptr() % 256 == 0
    for what, code, word, call in K.refusals(lib, arena.data_ptr()):
        rc = call(L)
        msg = L.ofx_last_error()
        assert rc == code, (what, rc, msg)
        assert msg and word in msg, (what, msg)
    torch.cuda.synchronize()
    assert int(arena.max()) == 0, "a refused call wrote something"


# ---- d. the companions ------------------------------------------------------------------------------------------------------------

def test_shift_levels(eng, oracle):
    import torch

    lib = eng._lib
    for run in RUNS:
        keep, descs, outs = [], [], []
        for (w, h, uv, rows, g) in K.SHIFT:
            src = K.frames(w, h)[1]
            row0, nrows, y0, y1, _ = rows if rows else (0, h, 0, h, 0)
            s = B.in_plane(src[row0:row0 + nrows], g, run)
            d = B.out_plane(nrows, s.pitch, g.lead)
            u = B.in_floats(uv, run)
            keep += [s, u]
            outs.append(d)
            descs.append(lib.ShiftDesc(s.ptr, d.ptr, lib.Geom(w, h, s.pitch, row0, nrows, y0, y1), u.ptr))
        eng.check(lib.load().ofx_shift_levels((lib.ShiftDesc * len(descs))(*descs), len(descs), eng._stream_ptr()), "ofx_shift_levels")
        torch.cuda.synchronize()
        for (w, h, uv, rows, g), d in zip(K.SHIFT, outs):
            what = f"shift {w}x{h} uv {uv} run {run}"
            row0, nrows, y0, y1, _ = rows if rows else (0, h, 0, h, 0)
            got, clean = d.host()
            plane = got[0]
            assert clean, f"{what}: bytes around d_dst were written"
            same(plane[y0 - row0:y1 - row0, :w], K.shift_ref(oracle, K.frames(w, h)[1], uv)[y0:y1], what)
            assert (plane[y0 - row0:y1 - row0, w:] == 0).all(), f"{what}: the pad bytes of the out rows are written as 0"
            assert (plane[:y0 - row0] == B.FILL).all() and (plane[y1 - row0:] == B.FILL).all(), f"{what}: rows that are no out rows were written"


def test_warp_levels(eng, oracle):
    import torch

    lib = eng._lib
    for run in RUNS:
        keep, descs, outs = [], [], []
        for (w, h, win, rows, g, bit) in K.WARP:
            src, flow = K.warp_flow(oracle, w, h, win)
            row0, nrows, y0, y1, f0 = rows if rows else (0, h, 0, h, 0)
            s = B.in_plane(src[row0:row0 + nrows], g, run)
            d = B.out_plane(nrows, s.pitch, g.lead)
            f = B.in_field(flow[f0:y1], (run + 1) % 3, g.flow_lead)
            st = B.out_words(np.int32, 1)
            B.put(st, np.array([[K.WARP_PRELOAD]], np.int32))
            keep += [s, f]
            outs.append((d, st))
            descs.append(lib.WarpDesc(s.ptr, d.ptr, lib.Geom(w, h, s.pitch, row0, nrows, y0, y1), f.ptr, f0, float(K.ITER_SCALE), st.ptr, bit))
        eng.check(lib.load().ofx_warp_levels((lib.WarpDesc * len(descs))(*descs), len(descs), eng._stream_ptr()), "ofx_warp_levels")
        torch.cuda.synchronize()
        for (w, h, win, rows, g, bit), (d, st) in zip(K.WARP, outs):
            what = f"warp {w}x{h} run {run}"
            src, flow = K.warp_flow(oracle, w, h, win)
            row0, nrows, y0, y1, f0 = rows if rows else (0, h, 0, h, 0)
            got, clean = d.host()
            plane = got[0]
            assert clean, f"{what}: bytes around d_dst were written"
            want, needs = K.warp_rows(src, flow, K.ITER_SCALE, row0, row0 + nrows)
            if rows is None:
                want = oracle.warp_bilinear_u8(src, flow, K.ITER_SCALE)
            same(plane[y0 - row0:y1 - row0, :w], want[y0:y1], what)
            assert (plane[y0 - row0:y1 - row0, w:] == 0).all(), f"{what}: the pad bytes of the out rows are written as 0"
            assert (plane[:y0 - row0] == B.FILL).all() and (plane[y1 - row0:] == B.FILL).all(), f"{what}: rows that are no out rows were written"
            missing = bool(needs[y0:y1].any())
            assert missing == (rows is not None), what
            assert int(st.host()[0][0, 0, 0]) == K.WARP_PRELOAD | (int(missing) << bit), what


def test_downsample_with_a_source_row_window(eng, oracle):
    import torch

    c = K.DOWN
    lib = eng._lib
    w, h = c["w"], c["h"]
    src = K.frames(2 * w, 2 * h)[0]
    want = np.ascontiguousarray(oracle.gauss_pyramid(K.synth.to_3ch(src), 2)[1][:, :, 0])
    row0, nrows, y0, y1 = c["rows"]
    for run in RUNS:
        s = B.in_plane(src[c["src_row0"]:c["src_row0"] + c["src_rows"]], K.geo(4 + run), run)
        d = B.out_plane(nrows, K.pitch_of(K.geo(run).pitch, w), K.geo(run).lead)
        g = lib.Geom(w, h, d.pitch, row0, nrows, y0, y1)
        eng.check(lib.load().ofx_downsample_1ch(s.ptr, s.pitch, c["src_row0"], c["src_rows"], d.ptr, C.byref(g), eng._stream_ptr()), "ofx_downsample_1ch")
        torch.cuda.synchronize()
        got, clean = d.host()
        plane = got[0]
        assert clean
        same(plane[y0 - row0:y1 - row0, :w], want[y0:y1], f"downsample run {run}")
        assert (plane[y0 - row0:y1 - row0, w:pad4(w)] == 0).all() and (plane[:, pad4(w):] == B.FILL).all(), f"run {run}: pad bytes"
        assert (plane[:y0 - row0] == B.FILL).all() and (plane[y1 - row0:] == B.FILL).all(), f"run {run}: rows that are no out rows were written"


def _pyramid(eng, img, levels, geos, run):
    """ofx_pyramid_1ch of img on caller-owned planes: (the level-0 input plane, [None, output plane of level 1, ...])"""
    lib = eng._lib
    h, w = img.shape
    src = B.in_plane(img, geos[0], run)
    outs = [None] + [B.out_plane(h >> k, K.pitch_of(geos[k].pitch, w >> k), geos[k].lead) for k in range(1, levels)]
    planes = (C.c_void_p * levels)(None, *[o.ptr for o in outs[1:]])
    pitches = (C.c_int * levels)(0, *[o.pitch for o in outs[1:]])
    eng.check(lib.load().ofx_pyramid_1ch(src.ptr, src.pitch, w, h, planes, pitches, levels, eng._stream_ptr()), "ofx_pyramid_1ch")
    return src, outs


@pytest.mark.parametrize("shape", K.PYRAMIDS, ids=lambda s: f"{s[0]}x{s[1]}-L{s[2]}")
def test_pyramid_equals_gauss_pyramid(eng, oracle, shape):
    import torch

    w, h, levels = shape
    img = K.frames(w, h)[0]
    want = oracle.gauss_pyramid(K.synth.to_3ch(img), levels)
    for run in RUNS:
        _, outs = _pyramid(eng, img, levels, [K.geo(run + 2 * k) for k in range(levels)], run)
        torch.cuda.synchronize()
        for k in range(1, levels):
            got, clean = outs[k].host()
            assert clean, f"level {k} run {run}: bytes around the plane were written"
            same(got[0][:, :w >> k], np.ascontiguousarray(want[k][:, :, 0]), f"level {k} run {run}")
            assert (got[0][:, w >> k:] == B.FILL).all(), f"level {k} run {run}: the pad bytes of a pyramid plane are left untouched"


def _corner_descs(lib, planes, w, h, levels, flows):
    return [lib.LkDesc(planes[0][k].ptr, planes[1][k].ptr, lib.Geom.full(w >> k, h >> k, planes[0][k].pitch), flows[k].ptr, 0, None, 0, 0.0, None, None,
                       0.0, None, 0) for k in range(levels)]


@pytest.mark.parametrize("mode", ["lk_float", "compat_cpu"])
@pytest.mark.parametrize("cfg", K.CORNERS, ids=lambda c: f"{c[0]}x{c[1]}-L{c[2]}-win{c[3]}-corner{c[4]}")
def test_corner_flows(eng, oracle, cfg, mode):
    import torch

    w, h, levels, win, corner = cfg
    lib = eng._lib
    p, n = K.corner_frames(w, h, corner)
    pyr = [[np.ascontiguousarray(x[:, :, 0]) for x in oracle.gauss_pyramid(K.synth.to_3ch(f), levels)] for f in (p, n)]
    want_uv, want_px0 = K.corner_want(oracle, w, h, levels, win, mode, corner)
    if corner:
        assert np.isnan(want_uv).any(), "the black corner was meant to leave a NaN shift"
    for run in RUNS:
        planes = [[B.in_plane(pyr[f][k], K.geo(run + k + 3 * f), (run + f) % 3) for k in range(levels)] for f in (0, 1)]
        flows = [B.out_flow(h >> k, w >> k, K.geo(run + k).flow_lead) for k in range(levels)]
        uv = B.out_words(np.float32, 2 * levels, 66)
        descs = _corner_descs(lib, planes, w, h, levels, flows)
        eng.check(lib.load().ofx_corner_flows((lib.LkDesc * levels)(*descs), levels, win, lib.MODES[mode], uv.ptr, eng._stream_ptr()), "ofx_corner_flows")
        torch.cuda.synchronize()
        got_uv, clean = uv.host()
        got_uv = got_uv[0, 0].reshape(levels, 2)
        assert clean
        same(got_uv[:levels - 1], want_uv[:levels - 1], f"d_uv run {run}")
        assert (got_uv[levels - 1].view(np.uint32) == 0x5A5A5A5A).all(), "the top level has no shift: its two floats are left alone"
        for k in range(levels):
            got, clean = flows[k].host()
            px = got[0].reshape(h >> k, w >> k, 2)
            same(px[0, 0], want_px0[k], f"pixel 0 of level {k} run {run}")
            rest = px.view(np.uint32).reshape(-1)[2:]
            assert clean and (rest == 0x5A5A5A5A).all(), f"level {k} run {run}: more than pixel 0 was written"


# ---- e. a whole pair by stateless calls only --------------------------------------------------------------------------------------

def test_a_whole_pair_by_stateless_calls(eng, oracle):
    """the recipe of include/ofx.h (ofx_warp_levels) on tight-pitch, 4-byte aligned caller buffers: two ofx_pyramid_1ch,
    ofx_corner_flows, one ofx_lk_levels over all levels with d_uv, then per refinement iteration pair ofx_shift_levels, ofx_warp_levels,
    ofx_lk_levels with accumulate and d_warp_out, ofx_lk_levels with accumulate"""
    import torch

    c = K.PAIR
    w, h, L, win = c["w"], c["h"], c["levels"], c["win"]
    assert c["iters"] == 3
    lib = eng._lib
    Lb = lib.load()
    st = eng._stream_ptr()
    p, n = K.pair_frames()
    g = K.Geo("tight", 4, 2)
    want = oracle.flow_pair_iter(p, n, L, win, 3)
    session = eng.flow_pair(p, n, L, win, "lk_float", iters=3)
    for run in RUNS:
        pyr = []
        for img in (p, n):
            src, outs = _pyramid(eng, img, L, [g] * L, run)
            pyr.append([src] + outs[1:])                       # level 0 is the caller's own plane
        geom = [lib.Geom.full(w >> k, h >> k, pyr[0][k].pitch) for k in range(L)]
        flows = [B.out_flow(h >> k, w >> k, g.flow_lead) for k in range(L)]
        uv = B.out_words(np.float32, 2 * L, 66)
        shifted = [B.out_plane(h >> k, pyr[0][k].pitch, g.lead) for k in range(L)]
        warped = [[B.out_plane(h >> k, pyr[0][k].pitch, g.lead) for k in range(L)] for _ in range(2)]
        uvp = lambda k: None if k == L - 1 else uv.ptr + 8 * k       # noqa: E731

        def lk(nxt, acc, wsrc=None, wout=None, with_uv=False):
            d = [lib.LkDesc(pyr[0][k].ptr, nxt[k], geom[k], flows[k].ptr, 0, uvp(k) if with_uv else None, acc, 0.0, wsrc and wsrc[k], wout and wout[k],
                            float(K.ITER_SCALE), None, 0) for k in range(L - 1, -1, -1)]      # coarse levels first
            eng.check(Lb.ofx_lk_levels((lib.LkDesc * L)(*d), L, win, lib.MODE_LK_FLOAT, st), "ofx_lk_levels")

        eng.check(Lb.ofx_corner_flows((lib.LkDesc * L)(*_corner_descs(lib, pyr, w, h, L, flows)), L, win, lib.MODE_LK_FLOAT, uv.ptr, st), "ofx_corner_flows")
        lk([pyr[1][k].ptr for k in range(L)], 0, with_uv=True)                                        # iteration 1
        sd = [lib.ShiftDesc(pyr[1][k].ptr, shifted[k].ptr, geom[k], uvp(k)) for k in range(L - 1)]
        eng.check(Lb.ofx_shift_levels((lib.ShiftDesc * len(sd))(*sd), len(sd), st), "ofx_shift_levels")
        wsrc = [shifted[k].ptr for k in range(L - 1)] + [pyr[1][L - 1].ptr]                           # (the top level is not shifted)
        wd = [lib.WarpDesc(wsrc[k], warped[0][k].ptr, geom[k], flows[k].ptr, 0, float(K.ITER_SCALE), None, 0) for k in range(L)]
        eng.check(Lb.ofx_warp_levels((lib.WarpDesc * L)(*wd), L, st), "ofx_warp_levels")
        lk([x.ptr for x in warped[0]], 1, wsrc, [x.ptr for x in warped[1]])                           # iteration 2, and the image of iteration 3
        lk([x.ptr for x in warped[1]], 1)                                                             # iteration 3
        torch.cuda.synchronize()
        for k in range(L):
            got, clean = flows[k].host()
            got = got[0].reshape(h >> k, w >> k, 2)
            assert clean, f"level {k} run {run}: bytes around the flow were written"
            same(got, want[k], f"level {k} run {run} against the oracle")
            same(got, session[k], f"level {k} run {run} against engine.flow_pair")
    assert not np.isfinite(want[0]).all(), "the frames were meant to produce non-finite flows"
