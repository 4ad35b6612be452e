"""The stateless launch ABI on caller-owned buffers (include/ofx.h: ofx_lk_levels, ofx_lk_level_sums, ofx_corner_flows,
ofx_shift_levels, ofx_warp_levels, ofx_pyramid_1ch, ofx_downsample_1ch): the case lists of tests/test_gpu_lk_abi.py, their frames and
their expected values.  NumPy only, no GPU; tests/test_lk_abi_ref.py shows on the oracle alone that the cases are what they claim.

Frames come from iter_hard.hard_frames (levels that hold a whole flat block) and synth (the tiny shapes).  Expected values come from
the oracle's functions: level_planes (+ its inline solve) for compat_cpu, lk_iter_level for lk_float, shift_back_pyramid,
warp_bilinear_u8, gauss_pyramid, flow_pair / flow_pair_iter.  The one restatement here is warp_rows: the "nearest row held" rule of
ofx_warp_levels / ofx_lk_desc on a row window, which the oracle does not have; test_lk_abi_ref.py pins it to the oracle's warp on
whole levels."""
from collections import namedtuple

import numpy as np

import iter_hard as ih
from cuda_optical_flow_2_amd import synth

F32 = np.float32
ITER_SCALE = F32(8.0 / 15.0)
MODES = ("compat_cpu", "lk_float", "lk_float_fast")

# ---- geometries -----------------------------------------------------------------------------------------------------------------
PITCH_KINDS = ("tight", "tight+4", "wide")     # (w + 3) & ~3; the same + 4; the session's pitch + 12
PLANE_LEADS = (4, 20, 256)                     # bytes: the plane is 4-byte aligned only; ...; 256-byte aligned
FLOW_LEADS = (2, 4)                            # floats: 8-byte aligned only; 16-byte aligned
FRONT = 256                                    # bytes in front of every lead: an input has at least this much of the test's own memory before it


def pitch_of(kind, w):
    tight = (w + 3) & ~3
    return {"tight": tight, "tight+4": tight + 4, "wide": (w + 63) // 64 * 64 + 12}[kind]


Geo = namedtuple("Geo", "pitch lead flow_lead")


def geo(i):
    """the i-th combination: every pitch kind meets every plane lead within nine cases, every flow lead within two"""
    return Geo(PITCH_KINDS[i % 3], PLANE_LEADS[(i + i // 3) % 3], FLOW_LEADS[i % 2])


# ---- frames ---------------------------------------------------------------------------------------------------------------------
def edge_w(win):
    """two tiles of the level kernel, the second one column wide"""
    return ih.tile_out_w(win >> 1) + 1


def frames(w, h, kind="hard", seed=None):
    """(prev, next) u8 [h, w].  hard: iter_hard.hard_frames with the flat block across the tile seam where the level has one (the
    block is cut to the level); smooth: a small translation; noise: synth.random_pair"""
    if kind == "smooth":
        return synth.smooth_pair(w, h, 0.6, -0.4, seed=w + 3 * h)
    if kind == "noise" or w < 32 or h < 16:
        return synth.random_pair(w, h, seed=(w + 7 * h) if seed is None else seed)
    seam = min(240, w - 1) if w > 200 else None     # (the tiles are 224 .. 248 columns wide: the block, 90 wide, covers every seam)
    p, n = ih.hard_frames(w, h, 2, seed=seed, seam_x=seam, block=(min(40, h // 2), 90), band=min(24, w // 4))
    return p, n


SPECIALS = [(np.nan, 1.5), (np.inf, -np.inf), (1e30, -1e30), (-0.0, -0.0), (-np.inf, 2.0), (3.25, np.nan), (-1e30, 0.0)]


def old_flow(base):
    """the flow an accumulating launch finds in d_flow: `base` (ordinary values: an oracle result) with NaN, +-Inf, +-1e30 and -0.0
    written over pixels spread across the level (every 5th pixel at most; a 1 x 1 level gets the NaN)"""
    f = np.array(base, F32)
    h, w = f.shape[:2]
    flat = f.reshape(-1, 2)
    n = len(flat)
    for i, s in enumerate(SPECIALS[:max(n // 5, 1)]):
        flat[i * max(n // len(SPECIALS), 1)] = s
    return f


def flow_kinds(f):
    """which of the special values a field holds"""
    f = np.asarray(f, F32)
    with np.errstate(invalid="ignore"):
        return {"nan": bool(np.isnan(f).any()), "+inf": bool((f == np.inf).any()), "-inf": bool((f == -np.inf).any()),
                "1e30": bool((np.abs(f) == F32(1e30)).any()), "-0": bool(((f == 0) & np.signbit(f)).any()),
                "ordinary": bool((np.isfinite(f) & (np.abs(f) < 1e6) & (f != 0)).any())}


# ---- expected values, from the oracle ---------------------------------------------------------------------------------------------
# "out": (w + 5, 0), per level.  "right": at w % 4 == 2 and a tight pitch the last lane's shifted dword would start at column w - 1,
# three bytes past the row pitch: the kernels move it back to pitch - 4 (nb = min(nb, pitch - 4))
UV_CASES = {"none": None, "frac": (-2.5, 1.25), "right": (1.5, -0.75), "out": None, "nan": (float("nan"), float("nan"))}


def uv_of(name, w):
    return (float(w + 5), 0.0) if name == "out" else UV_CASES[name]


def shift_ref(orc, img, uv):
    """what a level kernel reads as `next` under the shift vector uv (None: the plane itself): the oracle's shift_back_pyramid with a
    single coarser level whose pixel 0 holds uv / 2 (the halves are exact; 2 * half is uv again)"""
    if uv is None:
        return np.ascontiguousarray(img)
    half = (np.array(uv, F32) / F32(2)).reshape(1, 1, 2)
    return np.ascontiguousarray(orc.shift_back_pyramid(synth.to_3ch(img), 0, 2, [None, half])[:, :, 0])


def level_ref(orc, prev, nxt, win, mode, min_det=0.0):
    """the flow of one level whose next plane is read as it is.  compat_cpu: level_planes' integer sums through the reference's inline
    solve; lk_float (and the value lk_float_fast is held within one ulp of): lk_iter_level's first iteration, exact sums"""
    if mode == "compat_cpu":
        assert min_det == 0.0
        s = orc.level_planes(synth.to_3ch(prev), synth.to_3ch(nxt), win, 0)[3].astype(np.int64).astype(np.int32)
        return orc.inverse_matrix_inline_cpu(*s)
    return orc.lk_iter_level(prev, nxt, win, 1, min_det)[0]


def sums_ref(orc, prev, nxt, win):
    """lk_float: the five exact window sums as float32 (the kernel's are the integers themselves)"""
    return orc.level_planes(synth.to_3ch(prev), synth.to_3ch(nxt), win, 1, exact_sums=True)[3].astype(F32)


def add_ref(old, delta):
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(old, F32) + np.asarray(delta, F32)).astype(F32)


def warp_rows(src, flow, scale, row0=0, row_end=None):
    """orc_warp_bilinear_u8 (oracle/ofx_oracle.c) in float32 NumPy, every operation rounded once, with the row-window rule of
    include/ofx.h: a tap row outside [row0, row_end) is replaced by the nearest row held.  Returns (image, needs): needs marks the
    pixels with a finite flow one of whose tap rows lies outside the window."""
    src = np.asarray(src, np.uint8)
    h, w = src.shape
    row_end = h if row_end is None else row_end
    flow = np.asarray(flow, F32)
    s = F32(scale)
    yy, xx = np.mgrid[0:h, 0:w].astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        sx = (xx + (s * flow[..., 0]).astype(F32)).astype(F32)
        sy = (yy + (s * flow[..., 1]).astype(F32)).astype(F32)
        big = F32(1e9)
        ok = (sx >= -big) & (sx <= big) & (sy >= -big) & (sy <= big)
    sx = np.clip(np.where(ok, sx, xx), 0, F32(w - 1)).astype(F32)
    sy = np.clip(np.where(ok, sy, yy), 0, F32(h - 1)).astype(F32)
    x0, y0 = sx.astype(np.int64), sy.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    fx, fy = (sx - x0.astype(F32)).astype(F32), (sy - y0.astype(F32)).astype(F32)
    needs = ok & ((y0 < row0) | (y1 >= row_end))
    y0c, y1c = np.clip(y0, row0, row_end - 1), np.clip(y1, row0, row_end - 1)
    p = src.astype(F32)
    p00, p01, p10, p11 = p[y0c, x0], p[y0c, x1], p[y1c, x0], p[y1c, x1]
    a = (p00 + (fx * (p01 - p00)).astype(F32)).astype(F32)
    b = (p10 + (fx * (p11 - p10)).astype(F32)).astype(F32)
    v = (a + (fy * (b - a)).astype(F32)).astype(F32)
    out = (v + F32(0.5)).astype(F32).astype(np.int64).astype(np.uint8)
    return np.where(ok, out, src), needs


# ---- a. plain levels --------------------------------------------------------------------------------------------------------------
# rows: (row0, rows held, out_y0, out_y1, flow_row0); None = the whole level
Plain = namedtuple("Plain", "id w h win mode uv rows min_det geo kind")


def _plain():
    out = []
    i = 0

    def add(w, h, win, mode, uv="none", rows=None, min_det=0.0, kind="hard"):
        nonlocal i
        tag = f"{w}x{h}-win{win}-{mode}-uv_{uv}" + ("-rows" if rows else "") + ("-guard" if min_det else "")
        out.append(Plain(tag, w, h, win, mode, uv, rows, min_det, geo(i), kind))
        i += 1

    for mode in MODES:
        wins = (3, 9, 15, 23) + ((25,) if mode == "compat_cpu" else ())
        for win in wins:
            add(edge_w(win), 67, win, mode)
        # the shift fused into the row loads, on the odd widths
        add(250, 19, 9, mode, "frac")
        add(259, 20, 15, mode, "out")
        add(37, 21, 3, mode, "nan")
        add(edge_w(9), 67, 9, mode, "frac")
        add(5, 3, 23, mode)
        add(2, 2, 9, mode, "frac")
        add(1, 1, 3, mode)
        add(250, 19, 9, mode, "right")
        add(2, 2, 3, mode, "right")
        add(5, 3, 9, mode, "right")
        # three tiles: the middle one takes the kernels' interior form, whose flow pieces are 16 bytes at 8-byte aligned addresses
        add(521, 19, 9, mode, "frac")
        add(521, 19, 3, mode)
        # row windows: row0 > 0, rows < h, the out rows a strict subset of the rows held, flow_row0 < out_y0
        add(259, 20, 9, mode, "none", rows=(1, 17, 7, 12, 5))
        add(250, 19, 3, mode, "frac", rows=(3, 14, 6, 11, 2))
    add(edge_w(9), 67, 9, "lk_float", min_det=ih.MIN_DET)
    add(250, 19, 3, "lk_float", "frac", min_det=ih.MIN_DET)
    return out


PLAIN = _plain()
SUMS = Plain("sums-259x20-win9", 259, 20, 9, "lk_float", "none", (1, 17, 7, 12, 5), 0.0, Geo("tight", 4, 2), "hard")

# three descriptors of different sizes in one launch, one of them empty (out_y1 == out_y0); (w, h, rows); the empty one holds its
# whole level and asks for no row
MULTI = [(edge_w(9), 67, None), (37, 21, None), (5, 3, (0, 3, 1, 1, 0))]
MULTI_WIN = 9
MULTI_ORDERS = {"empty-first": (2, 0, 1), "empty-last": (1, 0, 2)}
GUARD_CASE = (edge_w(9), 67, 9)   # the level of MULTI the determinant guard is checked on (test_lk_abi_ref.py: neither empty nor full)


def plain_want(orc, c):
    """(the next plane as the level reads it, the whole level's flow)"""
    p, n = frames(c.w, c.h, c.kind)
    nr = shift_ref(orc, n, uv_of(c.uv, c.w))
    return nr, level_ref(orc, p, nr, c.win, c.mode if c.mode != "lk_float_fast" else "lk_float", c.min_det)


# ---- b. accumulate ----------------------------------------------------------------------------------------------------------------
# compat_cpu with accumulate = 1: the old march's MAY_ACC path, which only a stateless caller reaches
Acc = namedtuple("Acc", "id items win")       # items: (w, h, rows, geo)
ACC_COMPAT = [
    Acc("whole-win9", [(edge_w(9), 67, None, geo(0))], 9),
    Acc("whole-win25", [(edge_w(25), 67, None, geo(4))], 25),
    Acc("whole-250x19-win3", [(250, 19, None, geo(2))], 3),
    Acc("rows-259x20-win9", [(259, 20, (1, 17, 7, 12, 5), geo(1))], 9),
    Acc("two-descriptors-win15", [(37, 21, None, geo(5)), (259, 20, None, geo(3))], 15),
    Acc("tiny-win9", [(5, 3, None, geo(6)), (1, 1, None, geo(7)), (2, 2, None, geo(8))], 9),
    Acc("three-tiles-win9", [(521, 19, None, geo(0))], 9),
]


def acc_compat_want(orc, w, h, win):
    """(old flow, the whole level's flow after the launch) of an accumulating compat_cpu level that reads its next plane as it is"""
    p, n = frames(w, h)
    delta = level_ref(orc, p, n, win, "compat_cpu")
    old = old_flow(level_ref(orc, p, n, 3, "compat_cpu"))
    return old, add_ref(old, delta)


# lk_float / lk_float_fast on the buffer march: kIterAdd, kIterAddWarp, kIterSetWarp on whole levels.  The launch is a real
# refinement iteration: d_next is the oracle's warp of the next frame by the old flow (which is what iter_hard.check_fast_step
# replays for lk_float_fast), d_warp_src the next frame itself.
ITER_VARIANTS = ("add", "add+warp", "set+warp")
ITER_SHAPES = [(edge_w(3), 67, 3), (edge_w(9), 67, 9), (edge_w(15), 67, 15), (edge_w(23), 67, 23), (250, 19, 9), (259, 20, 3), (37, 21, 15),
               (5, 3, 23), (2, 2, 9), (1, 1, 3), (521, 19, 9), (521, 19, 23)]     # the last two: three tiles, the middle one interior
ITER_MODES = ("lk_float", "lk_float_fast")
_iter_cache = {}


def iter_inputs(orc, w, h, win):
    """{prev, next, old, fed (= warp(next, old), what d_next holds), delta (= the exact level of (prev, fed))} of an iteration case"""
    key = (w, h, win)
    if key not in _iter_cache:
        p, n = frames(w, h)
        old = old_flow(orc.lk_iter_level(p, n, win, 1)[0])
        fed = orc.warp_bilinear_u8(n, old)
        d = {"prev": p, "next": n, "old": old, "fed": fed, "delta": orc.lk_iter_level(p, fed, win, 1)[0]}
        for v in d.values():
            v.setflags(write=False)
        _iter_cache[key] = d
    return _iter_cache[key]


# the fused shift on the buffer march (accumulate with d_uv: a stateless caller's combination; a session shifts first), lk_float:
# (w, h, win, uv, with d_warp_out, geo)
ITER_UV = [(250, 19, 9, "right", False, geo(0)), (edge_w(9), 67, 9, "frac", True, geo(4)), (521, 19, 3, "right", True, geo(2)), (37, 21, 15, "nan", False, geo(7)),
           (2, 2, 3, "right", True, geo(6))]


def iter_uv_want(orc, w, h, win, uv):
    """(prev, next, old, the flow the launch leaves) of an accumulating lk_float level that reads next through the shift vector"""
    p, n = frames(w, h)
    old = old_flow(orc.lk_iter_level(p, n, win, 1)[0])
    return p, n, old, add_ref(old, level_ref(orc, p, shift_ref(orc, n, uv_of(uv, w)), win, "lk_float"))


# kIterAddWarpRows: (w, h, win, frames, rows, status bit, bits the status word holds before the launch)
ROWS_NO_MISS = dict(id="no-row-missing", w=259, h=40, win=9, kind="smooth", rows=(4, 28, 12, 22, 10), bit=3, preload=0)
ROWS_MISS = dict(id="row-missing", w=259, h=40, win=3, kind="hard", rows=(10, 14, 12, 22, 10), bit=4, preload=0b100101)
_rows_cache = {}


def rows_inputs(orc, c):
    """an iteration on a row window: as iter_inputs, plus flow (= old + delta on the whole level, exact), warped (the whole-level warp
    of next by flow) and needs (the pixels of the whole level whose taps need a row outside the window)"""
    if c["id"] not in _rows_cache:
        p, n = frames(c["w"], c["h"], c["kind"])
        base = orc.lk_iter_level(p, n, c["win"], 1)[0]
        old = old_flow(base) if c["kind"] == "hard" else np.array(base, F32)
        fed = orc.warp_bilinear_u8(n, old)
        flow = add_ref(old, orc.lk_iter_level(p, fed, c["win"], 1)[0])
        row0, rows = c["rows"][0], c["rows"][1]
        _, needs = warp_rows(n, flow, ITER_SCALE, row0, row0 + rows)
        d = {"prev": p, "next": n, "old": old, "fed": fed, "flow": flow, "warped": orc.warp_bilinear_u8(n, flow), "needs": needs}
        _rows_cache[c["id"]] = d
    return _rows_cache[c["id"]]


# ---- d. the companions ------------------------------------------------------------------------------------------------------------
# ofx_shift_levels: three descriptors, a row window among them: (w, h, uv, rows (as above, flow_row0 unused), geo)
SHIFT = [(250, 19, (1.5, -0.75), None, geo(3)), (edge_w(9), 67, (-2.5, 1.25), None, geo(0)), (37, 21, (float("nan"), 0.5), None, geo(4)), (259, 20, (3.0, -2.0), (2, 15, 7, 12, 0), geo(8)),
         (250, 19, (255.0, 0.0), None, geo(1)), (5, 3, (0.75, -0.75), None, geo(5))]
# ofx_warp_levels: (w, h, win of the flow's level, rows, geo, status bit); the flows are the old_flow fields of hard frames
WARP = [(edge_w(9), 67, 9, None, geo(2), 0), (250, 19, 3, (3, 14, 6, 11, 2), geo(3), 5), (37, 21, 15, None, geo(7), 0), (5, 3, 3, None, geo(6), 0),
        (259, 20, 9, None, geo(1), 0)]
WARP_PRELOAD = 0b1000001
DOWN = dict(w=129, h=10, src_row0=4, src_rows=11, rows=(2, 6, 3, 7), geo=geo(0), src_geo=geo(4))   # rows: (row0, rows held, out_y0, out_y1) of the destination
PYRAMIDS = [(264, 80, 3), (500, 76, 3), (4, 4, 2), (2, 2, 2), (72, 136, 4)]
# ofx_corner_flows: (w, h, levels, window, black corner): with the corner, pixel 0 of levels 1 and 2 has no texture -- a NaN shift
CORNERS = [(264, 80, 3, 9, 48), (264, 80, 3, 9, 0), (250, 36, 2, 3, 0)]


def warp_flow(orc, w, h, win):
    p, n = frames(w, h)
    return n, old_flow(orc.lk_iter_level(p, n, win, 1)[0])


def corner_frames(w, h, corner):
    p, n = ih.hard_frames(w, h, 2, block=(min(40, h // 2), 90), band=min(24, w // 4), corner=corner)
    return p, n


def corner_want(orc, w, h, levels, win, mode, corner):
    """(d_uv as ofx_corner_flows leaves it: 2 floats per level below the top, in float32, coarsest level first; pixel 0 of every level)"""
    p, n = corner_frames(w, h, corner)
    flows = orc.flow_pair(synth.to_3ch(p), synth.to_3ch(n), levels, win, mode, exact_sums=True)[0]
    uv = np.zeros((levels, 2), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(levels - 1):
            u = v = F32(0)
            for j in range(levels - 1, k, -1):
                m = F32(1 << (j - k))
                u = F32(u + F32(m * flows[j][0, 0, 0]))
                v = F32(v + F32(m * flows[j][0, 0, 1]))
            uv[k] = (u, v)
    return uv, np.array([f[0, 0] for f in flows], F32)


# ---- e. a whole pair by stateless calls ---------------------------------------------------------------------------------------------
PAIR = dict(w=264, h=80, levels=3, win=9, iters=3)


def pair_frames():
    return frames(PAIR["w"], PAIR["h"])


# ---- c. refusals ------------------------------------------------------------------------------------------------------------------
OFX_E_INVALID, OFX_E_UNSUPPORTED = 1, 3


def refusals(lib, base):
    """[(what, expected code, a word of the message, call)]: call(L) makes the stateless call on the loaded library L and returns its
    status.  Every case fails a check on the host, before anything is enqueued.  base: an address with 4 MiB behind it, 256-byte
    aligned, from which the planes and fields are carved (a GPU test passes a real allocation, so that a call that is wrongly
    accepted still runs inside it; the host test passes a made-up one)."""
    K64 = 1 << 16
    PREV, NEXT, FLOW, WSRC, WOUT, STATUS, UV, DST = (base + i * 8 * K64 for i in range(8))
    W, H, P = 64, 32, 64

    def lk(n=1, win=9, mode="lk_float", which=0, **kw):
        """n descriptors of a 64 x 32 level; the keywords change descriptor `which`"""
        def one(prev=PREV, nxt=NEXT, w=W, h=H, pitch=P, row0=0, rows=H, y0=0, y1=H, flow=FLOW, f0=0, uv=None, acc=0, min_det=0.0, wsrc=None,
                wout=None, status=None, bit=0):
            return lib.LkDesc(prev, nxt, lib.Geom(w, h, pitch, row0, rows, y0, y1), flow, f0, uv, acc, min_det, wsrc, wout, 0.5, status, bit)
        common = {k: kw.pop(k) for k in list(kw) if k.startswith("all_")}
        descs = [one(**{k[4:]: v for k, v in common.items()}) for _ in range(max(n, 1))]
        descs[which] = one(**{**{k[4:]: v for k, v in common.items()}, **kw})
        arr = (lib.LkDesc * len(descs))(*descs)
        return lambda L: L.ofx_lk_levels(arr, n, win, lib.MODES[mode], None)

    iter_kw = dict(all_acc=1, all_wsrc=WSRC, all_wout=WOUT)
    out = [
        ("d_warp_out with compat_cpu", OFX_E_INVALID, b"lk_float", lk(mode="compat_cpu", **iter_kw)),
        ("iteration 1 with d_warp_out on a row window", OFX_E_INVALID, b"row window", lk(all_wsrc=WSRC, all_wout=WOUT, row0=2, rows=28, y0=8, y1=20)),
        ("accumulate on some descriptors only", OFX_E_INVALID, b"for all descriptors", lk(n=3, which=1, acc=1)),
        ("accumulate missing on the last descriptor", OFX_E_INVALID, b"for all descriptors", lk(n=3, which=2, all_acc=1, acc=0)),
        ("d_warp_out on some descriptors only", OFX_E_INVALID, b"for all descriptors", lk(n=2, which=1, all_acc=1, wsrc=WSRC, wout=WOUT)),
        ("d_warp_out == d_next", OFX_E_INVALID, b"plane of its own", lk(all_acc=1, wsrc=WSRC, wout=NEXT)),
        ("d_warp_out == d_prev", OFX_E_INVALID, b"plane of its own", lk(all_acc=1, wsrc=WSRC, wout=PREV)),
        ("d_warp_out == d_warp_src", OFX_E_INVALID, b"plane of its own", lk(all_acc=1, wsrc=WSRC, wout=WSRC)),
        ("d_warp_out without d_warp_src", OFX_E_INVALID, b"d_warp_src", lk(all_acc=1, wout=WOUT)),
        ("d_prev at lead 2", OFX_E_INVALID, b"4-byte aligned", lk(prev=PREV + 2)),
        ("d_next at lead 2", OFX_E_INVALID, b"4-byte aligned", lk(n=2, which=1, nxt=NEXT + 2)),
        ("d_warp_out at lead 2", OFX_E_INVALID, b"4-byte aligned", lk(all_acc=1, wsrc=WSRC, wout=WOUT + 2)),
        ("d_flow 4-byte aligned only", OFX_E_INVALID, b"8-byte aligned", lk(flow=FLOW + 4)),
        ("d_flow 4-byte aligned only, accumulating", OFX_E_INVALID, b"8-byte aligned", lk(n=2, which=1, flow=FLOW + 12, **iter_kw)),
        ("pitch no multiple of 4", OFX_E_INVALID, b"pitch", lk(pitch=66)),
        ("pitch below w", OFX_E_INVALID, b"pitch", lk(pitch=60)),
        ("a missing halo row above", OFX_E_INVALID, b"halo", lk(row0=4, rows=28, y0=8, y1=20)),
        ("a missing halo row below", OFX_E_INVALID, b"halo", lk(row0=0, rows=24, y0=8, y1=20)),
        ("an even window", OFX_E_INVALID, b"odd", lk(win=8)),
        ("window 1", OFX_E_INVALID, b"odd", lk(win=1)),
        ("window 25 in lk_float", OFX_E_UNSUPPORTED, b"not supported", lk(win=25)),
        ("window 25 in lk_float_fast", OFX_E_UNSUPPORTED, b"not supported", lk(win=25, mode="lk_float_fast")),
        ("window 27 in compat_cpu", OFX_E_UNSUPPORTED, b"not supported", lk(win=27, mode="compat_cpu")),
        ("warp_status_bit 31", OFX_E_INVALID, b"warp_status_bit", lk(status=STATUS, bit=31, **iter_kw)),
        ("warp_status_bit -1", OFX_E_INVALID, b"warp_status_bit", lk(status=STATUS, bit=-1, **iter_kw)),
        ("flow_row0 > out_y0", OFX_E_INVALID, b"flow_row0", lk(y0=4, f0=5)),
        ("n = 0", OFX_E_INVALID, b"descriptor count", lk(n=0)),
        ("a null plane", OFX_E_INVALID, b"null", lk(nxt=None)),
        ("out rows outside the level", OFX_E_INVALID, b"output rows", lk(y1=H + 1)),
    ]

    def shift(**kw):
        def one(src=PREV, dst=DST, pitch=P, uv=UV):
            return lib.ShiftDesc(src, dst, lib.Geom(W, H, pitch, 0, H, 0, H), uv)
        arr = (lib.ShiftDesc * 2)(one(), one(**kw))
        return lambda L: L.ofx_shift_levels(arr, 2, None)

    def warp(**kw):
        def one(src=PREV, dst=DST, pitch=P, flow=FLOW, f0=0):
            return lib.WarpDesc(src, dst, lib.Geom(W, H, pitch, 0, H, 0, H), flow, f0, 0.5, None, 0)
        arr = (lib.WarpDesc * 2)(one(), one(**kw))
        return lambda L: L.ofx_warp_levels(arr, 2, None)

    def pyramid(level0=PREV, pitch0=P, l1=NEXT, p1=32):
        import ctypes as C
        planes = (C.c_void_p * 3)(None, l1, DST)
        pitches = (C.c_int * 3)(0, p1, 16)
        return lambda L: L.ofx_pyramid_1ch(level0, pitch0, W, H, planes, pitches, 3, None)

    def corner(**kw):
        def one(prev=PREV, nxt=NEXT):
            return lib.LkDesc(prev, nxt, lib.Geom(W, H, P, 0, H, 0, H), FLOW, 0, None, 0, 0.0, None, None, 0.0, None, 0)
        arr = (lib.LkDesc * 2)(one(), one(**kw))
        return lambda L: L.ofx_corner_flows(arr, 2, 9, lib.MODE_LK_FLOAT, UV, None)

    out += [
        ("shift: d_dst at lead 2", OFX_E_INVALID, b"4-byte aligned", shift(dst=DST + 2)),
        ("shift: d_src at lead 1", OFX_E_INVALID, b"4-byte aligned", shift(src=PREV + 1)),
        ("shift: pitch 62", OFX_E_INVALID, b"pitch", shift(pitch=62)),
        ("shift in place", OFX_E_INVALID, b"in-place", shift(dst=PREV)),
        ("warp: d_dst at lead 2", OFX_E_INVALID, b"4-byte aligned", warp(dst=DST + 2)),
        ("warp: d_src at lead 3", OFX_E_INVALID, b"4-byte aligned", warp(src=PREV + 3)),
        ("warp: d_flow 4-byte aligned only", OFX_E_INVALID, b"8-byte aligned", warp(flow=FLOW + 4)),
        ("warp: flow_row0 > out_y0", OFX_E_INVALID, b"flow_row0", warp(f0=1)),
        ("pyramid: level 1 at lead 2", OFX_E_INVALID, b"4-byte aligned", pyramid(l1=NEXT + 2)),
        ("pyramid: level 1 pitch 34", OFX_E_INVALID, b"4-byte aligned", pyramid(p1=34)),
        ("pyramid: level 1 pitch below its width", OFX_E_INVALID, b"bad plane", pyramid(p1=28)),
        ("pyramid: level 0 pitch below the width", OFX_E_INVALID, b"level 0", pyramid(pitch0=60)),
        ("pyramid: level 0 at lead 2", OFX_E_INVALID, b"level 0", pyramid(level0=PREV + 2)),
        ("corner: d_next at lead 2", OFX_E_INVALID, b"4-byte aligned", corner(nxt=NEXT + 2)),
    ]
    return out
