"""One recipe per stateless entry point, for the stream contract of include/ofx.h ("Device entry points only enqueue work; they never
synchronise or allocate", host arrays read before the call returns, work buffers that need nothing and keep nothing).  A recipe is
host-only until stage(): its inputs are NumPy arrays and its `want` comes from the referee that the entry point's own GPU test uses.
tests/test_call_order_cases.py checks the recipes on the CPU, tests/test_gpu_call_order.py runs them the hard way.

A recipe has
    want            {name: array} by the referee, in the layout read() returns
    reach           facts about the case that the referee established (tiles, groups, counts), for the CPU test
    stage(torch)    device copies of the clean inputs (`ins`), the buffers the call reads, the outputs (`outs`, test_gpu_interp.Guarded:
                    0x5A all around) and the work / stats / scratch buffers (`works`); share=<a staged recipe> reuses that recipe's
                    work, stats, counter and in-place buffers
    launch(stream)  builds descriptors and tables afresh, calls the library and overwrites every host array it passed with 0xFF
    outputs()       {name: tensor} to snapshot;  read(snapshot) -> {name: array}, having checked the bytes around every output
    branches()      what of `reach` another case of the same row must reach as well

variant(name) is recipe(name) with other device data: the same geometry, pitches, models, parameters, times and seeds -- everything
the host passes is identical --, other frames, fields, points, matches and status arrays.  It is what a captured call may see change
between two replays (tests/test_gpu_graph_capture.py): stage_variant() puts its clean inputs on the device, load_variant() copies
them into the recipe's own staged `clean` buffers, from which every load() -- live or recorded -- fills the buffers the call reads."""
import copy
import ctypes as C
import functools

import numpy as np

import chain_cases as KC
import chain_ref as KR
import consistency_ref as CR
import dense_ref as D
import fit_motion_ref as FR
import homography_cases as HC
import homography_ref as HR
import interp3_ref as I3
import interp_ref as IR
import klt_ref as K
import lk_abi_cases as LK
import median_ref as M
import mosaic_cases as MC
import mosaic_ref as MZ
import motion_ref as MR
import sampled_ref as SR
import temporal_cases as TC
import temporal_ref as TR
import texture_ref as T
import warp_affine_ref as WA
import warp_persp_ref as WP
from cuda_optical_flow_2_amd import lib as L
from cuda_optical_flow_2_amd import synth
from test_gpu_fit_motion import matches as motion_matches
from test_gpu_interp import FILL, Guarded, Plane
from test_gpu_warp_affine import image

F32 = np.float32
NAN = float("nan")
POISON = {np.dtype(np.uint8): 0xEE, np.dtype(np.float32): NAN, np.dtype(np.int32): -1}     # what an input buffer holds outside its window
WORK_FILL = 0xA5
# the tiles of csrc/fit_motion.hip and csrc/fit_homography.hip: matches per score block, hypotheses per score block
FIT_TILE, FIT_GROUP = 1024, 32


@functools.lru_cache(maxsize=None)
def oracle():
    import oracle as orc

    orc.build()
    return orc.Oracle()


def wipe(*host):
    """0xFF over every host array a call was given: a library that reads one after it has returned reads this"""
    for a in host:
        if a is None:
            continue
        if isinstance(a, np.ndarray):
            a.reshape(-1).view(np.uint8)[...] = 0xFF
        else:
            C.memset(C.addressof(a), 0xFF, C.sizeof(a))


def same(got, want, what):
    """by the bits: float32 through dense_ref.same_bits, float64 as int64, integers as they are"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype}{got.shape} vs {want.dtype}{want.shape}"
    if got.dtype == np.float32:
        ok = D.same_bits(got, want)
    elif got.dtype == np.float64:
        ok = got.view(np.int64) == want.view(np.int64)
    else:
        ok = got == want
    if not ok.all():
        bad = np.argwhere(~ok)
        raise AssertionError(f"{what}: {len(bad)}/{got.size} differ, first at {bad[:3].tolist()}: {got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}")


def differs(a, b):
    """whether two referee results (dicts of arrays) differ anywhere"""
    for k in a:
        if k in b and (a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes()):
            return True
    return False


class In:
    """An input on the device: `clean` holds its bytes, `buf` is the buffer the call reads (ptr: the input inside it)."""

    def __init__(self, torch, host, lead=0, tail=16):
        host = np.ascontiguousarray(host).reshape(-1)
        pad = np.frombuffer(b"\xEE" * host.itemsize, host.dtype)[0]
        whole = np.concatenate([np.full(lead, pad, host.dtype), host, np.full(tail, pad, host.dtype)])
        self.clean = torch.from_numpy(whole).cuda()
        self.buf = torch.empty_like(self.clean)
        self.ptr = self.buf.data_ptr() + lead * host.itemsize
        self.poison = POISON[host.dtype]

    @classmethod
    def plane(cls, torch, arr, pitch, lead, around):
        """a u8 plane [h, w] with rows `pitch` apart, `lead` bytes in (test_gpu_interp.Plane's layout)"""
        p = Plane(np.ascontiguousarray(arr), pitch, lead, around)
        self = cls.__new__(cls)
        self.clean, self.buf, self.pitch, self.poison = p.t, torch.empty_like(p.t), pitch, 0xEE
        self.ptr = self.buf.data_ptr() + lead
        return self

    def fill(self):
        self.buf.fill_(self.poison)

    def load(self):
        self.buf.copy_(self.clean)


class InOut:
    """A buffer the call reads and writes in place: a Guarded of one tightly packed slot, loaded with the clean input."""

    def __init__(self, torch, g, host):
        raw = torch.from_numpy(np.ascontiguousarray(host).reshape(-1).view(np.uint8).copy()).cuda()
        o = g.lead * g.size
        self.clean, self.dst = raw, g.flat[o:o + raw.numel()]

    def fill(self):
        pass

    def load(self):
        self.dst.copy_(self.clean)


def host_of(g, flat):
    """Guarded.host() of a snapshot of g.flat"""
    c = copy.copy(g)
    c.flat = flat
    return c.host()


class Recipe:
    name = entry = ""

    def __init__(self):
        self.want, self.reach = {}, {}
        self.ins, self.loads, self.outs, self.works = [], [], {}, []

    def lib(self):
        return L.load()

    def outputs(self):
        return {k: g.flat for k, g in self.outs.items()}

    def read(self, snap):
        out = {}
        for k, g in self.outs.items():
            got, clean = host_of(g, snap[k])
            assert clean, f"{self.name}: bytes around {k} were written"
            out[k] = got.reshape(self.want[k].shape) if k in self.want else got
        return out

    def branches(self):
        return {}

    def want_over(self, prev):
        """`want` of this call made on outputs that hold the results of prev, a recipe of the same geometry"""
        return self.want

    def check(self, snap, what="", want=None):
        got = self.read(snap)
        for k, w in (self.want if want is None else want).items():
            same(got[k], w, f"{what or self.name}: {k}")

    def stage_variant(self, torch, v):
        """after stage(): device copies of the clean inputs of v, a recipe of this one's geometry, and of this one's own (v's buffers
        are dropped)"""
        v.stage(torch)
        mine, theirs = self.ins + self.loads, v.ins + v.loads
        assert len(mine) == len(theirs), (self.name, v.name)
        for a, b in zip(mine, theirs):
            assert a.clean.shape == b.clean.shape and a.clean.dtype == b.clean.dtype, (self.name, v.name)
        self.clean_of = {True: [b.clean for b in theirs], False: [a.clean.clone() for a in mine]}
        v.ins, v.loads, v.outs, v.works = [], [], {}, []

    def load_variant(self, on=True):
        """the variant's clean inputs (on=False: this recipe's own again) into the staged `clean` buffers, which every load() reads --
        a load() recorded in a graph as well: copies on the current stream, nothing is allocated"""
        for a, clean in zip(self.ins + self.loads, self.clean_of[on]):
            a.clean.copy_(clean)


def work(torch, nbytes):
    return torch.full(((nbytes + 7) // 8 * 8 + 256,), WORK_FILL, dtype=torch.uint8, device="cuda")


# ---- camera motion and homography from point matches --------------------------------------------------------------------------------
class Fit(Recipe):
    """ofx_fit_motion (model 0 .. 2) or ofx_fit_homography (model 3) on items (p, q, status or None, pair, (w, h))"""

    def __init__(self, name, model, items, H, thr_q, refits, seed):
        super().__init__()
        self.name, self.model, self.items, self.prm = name, model, items, (H, thr_q, refits, seed)
        self.homography = model == HR.HOMOGRAPHY
        self.entry = "ofx_fit_homography" if self.homography else "ofx_fit_motion"
        self.dim = 9 if self.homography else 6
        res = []
        for p, q, st, pair, size in items:
            if self.homography:
                res.append(HR.fit_homography(p, q, size, st, pair, H, thr_q, refits, seed))
            else:
                res.append(FR.fit_motion(p, q, size, st, pair, model, H, thr_q, refits, seed))
        self.want["model"] = np.stack([r[0] for r in res]).reshape(len(items), 1, self.dim)
        self.want["info"] = np.stack([r[1] for r in res]).reshape(len(items), 1, 8)
        for i, r in enumerate(res):
            self.want[f"mask{i}"] = r[2].reshape(1, 1, -1)
        self.reach = dict(tiles=max(-(-len(it[0]) // FIT_TILE) for it in items), groups=-(-H // FIT_GROUP),
                          info=[r[1].tolist() for r in res], n=[len(it[0]) for it in items], status=[it[2] is not None for it in items])

    def branches(self):
        r = self.reach
        return dict(tiles=r["tiles"], groups=r["groups"], n=r["n"], status=r["status"], code=[i[0] for i in r["info"]], refits=[i[6] for i in r["info"]],
                    usable=[0 < i[1] < n for i, n in zip(r["info"], r["n"])], inliers=[0 < i[5] < i[1] for i in r["info"]],
                    mask=[0 < int(self.want[f"mask{k}"].sum()) < self.want[f"mask{k}"].size for k in range(len(self.items))])

    def work_bytes(self):
        prm = L.FitParams(self.model, *self.prm)
        fn = self.lib().ofx_fit_homography_work_bytes if self.homography else self.lib().ofx_fit_motion_work_bytes
        return int(fn(C.byref(prm)))

    def stage(self, torch, share=None):
        self.ins, self.ptrs = [], []
        for i, (p, q, st, pair, size) in enumerate(self.items):
            tp, tq = In(torch, np.asarray(p, F32), 2 * (i % 2)), In(torch, np.asarray(q, F32), 2)
            ts = None if st is None else In(torch, np.asarray(st, np.int32), 1)
            self.ins += [t for t in (tp, tq, ts) if t is not None]
            self.ptrs.append((tp.ptr, tq.ptr, None if ts is None else ts.ptr))
        n = len(self.items)
        self.outs = {"model": Guarded(np.float64, n, 1, self.dim, self.dim, 1), "info": Guarded(np.int32, n, 1, 8, 8, 3)}
        for i, it in enumerate(self.items):
            self.outs[f"mask{i}"] = Guarded(np.uint8, 1, 1, len(it[0]), len(it[0]), 1 + i)          # (odd addresses)
        nbytes = self.work_bytes()
        assert nbytes > 0
        if share is None:
            self.works = [work(torch, nbytes) for _ in self.items]
        else:
            self.works = share.works[:n]
            assert len(self.works) == n and all(w.numel() >= nbytes for w in self.works)

    def launch(self, stream):
        prm = L.FitParams(self.model, *self.prm)
        descs = (L.FitDesc * len(self.items))()
        for i, (p, q, st, pair, (w, h)) in enumerate(self.items):
            dp, dq, ds = self.ptrs[i]
            descs[i] = L.FitDesc(dp, dq, ds, len(p), pair, w, h, self.outs["model"].slot(i), self.outs["info"].slot(i), self.outs[f"mask{i}"].ptr,
                                 self.works[i].data_ptr())
        fn = self.lib().ofx_fit_homography if self.homography else self.lib().ofx_fit_motion
        rc = fn(descs, len(self.items), C.byref(prm), stream)
        wipe(descs, prm)
        return rc


FIT_SIZE = (192, 128)


def fit_items(homography, seed):
    """the table's two items: n = 1025 (two score tiles) and n = 65 with a status array around pair 5"""
    mk = HC.matches if homography else motion_matches
    a, b = mk(1025, FIT_SIZE, seed), mk(65, (67, 45), seed + 1, status=True)
    return [(a[0], a[1], None, 0, FIT_SIZE), (b[0], b[1], b[2], 5, (67, 45))]


def few_item(usable, n=9, size=(67, 45)):
    """n matches of which `usable` are usable: the others hold a NaN"""
    rng = np.random.RandomState(40 + usable)
    p = np.stack([rng.randint(0, 32 * (size[0] - 1), n), rng.randint(0, 32 * (size[1] - 1), n)], axis=1).astype(F32) / F32(32)
    q = p[::-1].copy()
    p[usable:, 0] = NAN
    return (p, q, None, 0, size)


# ---- affine and perspective warp ----------------------------------------------------------------------------------------------------
WARP_SHAPE = (67, 45, 64, 48)         # (w, h, sw, sh)


def _rot(sw, sh, tail=()):
    c, s = 1.1 * np.cos(0.3), 1.1 * np.sin(0.3)
    return (c, -s, 0.3 * sw, s, c, -0.2 * sh) + tail


class Warp(Recipe):
    """ofx_warp_affine (6 entries per model) or ofx_warp_perspective (9): items (src, (w, h), model, border, fill), each with d_outside"""

    def __init__(self, name, items):
        super().__init__()
        self.name, self.items = name, items
        self.persp = len(items[0][2]) == 9
        self.entry = "ofx_warp_perspective" if self.persp else "ofx_warp_affine"
        outside = []
        for i, (src, size, m, border, fill) in enumerate(items):
            dst, n = (WP.warp_perspective if self.persp else WA.warp_affine)(src, m, size, border, fill)
            self.want[f"dst{i}"] = dst.reshape(1, size[1], -1)
            outside.append(n)
        self.want["outside"] = np.array(outside, np.int64).reshape(len(items), 1, 1)
        self.reach = dict(outside=outside, pixels=[it[1][0] * it[1][1] for it in items], channels=[1 if it[0].ndim == 2 else 3 for it in items])

    def branches(self):
        r = self.reach
        return dict(pixels=r["pixels"], channels=r["channels"], some=[0 < n < px for n, px in zip(r["outside"], r["pixels"])])

    def stage(self, torch, share=None):
        self.ins, self.outs = [], {}
        for i, (src, (w, h), m, border, fill) in enumerate(self.items):
            ch = 3 if src.ndim == 3 else 1
            sh, sw = src.shape[:2]
            self.ins.append(In.plane(torch, src.reshape(sh, ch * sw), ch * sw + 2 * i + 5, 1 + 2 * i, 0xEE))
            self.outs[f"dst{i}"] = Guarded(np.uint8, 1, h, ch * w, ch * w + 3 * i + 7, 1 + 2 * i)
        self.outs["outside"] = Guarded(np.int64, len(self.items), 1, 1, 1, 1) if share is None else share.outs["outside"]
        self.works = []        # (d_outside is an output: it is compared.  Nothing else is kept.)

    def launch(self, stream):
        Desc = L.WarpPerspDesc if self.persp else L.WarpAffineDesc
        descs = (Desc * len(self.items))()
        for i, (src, (w, h), m, border, fill) in enumerate(self.items):
            ch = 3 if src.ndim == 3 else 1
            sh, sw = src.shape[:2]
            dst = self.outs[f"dst{i}"]
            descs[i] = Desc(self.ins[i].ptr, self.ins[i].pitch, sw, sh, dst.ptr, dst.pitch, w, h, ch, WA.BORDERS[border], fill,
                            (C.c_double * len(m))(*m), self.outs["outside"].slot(i))
        fn = self.lib().ofx_warp_perspective if self.persp else self.lib().ofx_warp_affine
        rc = fn(descs, len(self.items), stream)
        wipe(descs)
        return rc


def warp_items(persp, model_c3, model_c1, seed=0):
    w, h, sw, sh = WARP_SHAPE
    tail = lambda m: tuple(m) + ((0.0, 0.0, 1.0) if persp and len(m) == 6 else ())      # noqa: E731
    return [(image(sw, sh, 3, seed), (w, h), tail(model_c3), "constant", 37), (image(sw, sh, 1, seed), (w, h), tail(model_c1), "constant", 201)]


INSIDE = (0.9, 0.0, 0.25, 0.0, 0.9, 0.5)                        # 67 x 45 lands inside 64 x 48: nothing is outside
INSIDE_P = (0.9, 0.0, 0.25, 0.0, 0.9, 0.5, 1e-4, 2e-4, 1.0)
FAR = (1.0, 0.0, 40.0, 0.0, 1.0, 20.0)                          # most of the output is outside


# ---- frame mosaic -----------------------------------------------------------------------------------------------------------------------
# (w, h, channels, sources, border, fill, d_which given, d_counts given): five items, which take the 16-item instance of
# csrc/warp_mosaic.hip, with up to six sources, which take its 9-source instance
MOSAIC_GEOM = [(67, 45, 3, 5, "replicate", 37, True, True), (33, 17, 1, 5, "constant", 201, True, False), (70, 20, 1, 6, "replicate", 0, False, True),
               (9, 8, 3, 2, "constant", 90, False, False), (45, 33, 1, 1, "constant", 5, True, True)]
COUNTS_LEFT = np.frombuffer(bytes([FILL]) * 8, np.int64)[0]        # a d_counts slot of an item that gave NULL


def mosaic_sources(kind, w, h, ch, S, seed):
    """(srcs, models) of one item.  'ladder': mosaic_cases.ladder, its images redrawn from `seed`; 'steps': S sources of the output's
    size, source k 2 (S - k) pixels and a quarter to the right and a pixel and a half up or down, so that each covers two columns more
    than the one before it and together they cover most of the output; 'edge': the same sources far to the right: source k covers the
    output's columns 0 .. k + 1 and nothing else"""
    if kind == "ladder":
        _, srcs, models, _ = MC.ladder(w, h, S, ch)
        return [MC.image(s.shape[1], s.shape[0], ch, seed + 7 * k + S) for k, s in enumerate(srcs)], models
    srcs = [MC.image(w, h, ch, seed + 31 + k) for k in range(S)]
    if kind == "steps":
        turn = [0.003 if k == 3 else 0.0 for k in range(S)]
        models = [(np.cos(a), -np.sin(a), 2.0 * (S - k) + 0.25, np.sin(a), np.cos(a), 1.5 if k % 2 else -1.5, 0.0, 0.0, 1.0) for k, a in enumerate(turn)]
    else:
        models = [(1.0, 0.0, float(w - 2 - k), 0.0, 1.0, 0.25, 0.0, 0.0, 1.0) for k in range(S)]
    return srcs, models


def mosaic_items(kind, seed=0):
    return [mosaic_sources(kind, w, h, ch, S, seed) + ((w, h), border, fill, which, counts) for w, h, ch, S, border, fill, which, counts in MOSAIC_GEOM]


class Mosaic(Recipe):
    """ofx_warp_mosaic on items (srcs, models, (w, h), border, fill, d_which given, d_counts given).  d_counts has a slot per item:
    the slot of an item that gave NULL keeps its 0x5A."""
    entry = "ofx_warp_mosaic"

    def __init__(self, name, items):
        super().__init__()
        self.name, self.items = name, items
        counts = []
        for i, (srcs, models, size, border, fill, which, cnt) in enumerate(items):
            dst, wh, cn = MZ.mosaic(srcs, models, size, border, fill)
            self.want[f"dst{i}"] = dst.reshape(1, size[1], -1)
            if which:
                self.want[f"which{i}"] = wh.reshape(1, size[1], size[0])
            counts.append(cn)
        self.want["counts"] = np.stack([c if it[6] else np.full(10, COUNTS_LEFT, np.int64) for c, it in zip(counts, items)]).reshape(len(items), 1, 10)
        self.reach = dict(counts=[c.tolist() for c in counts], pixels=[it[2][0] * it[2][1] for it in items], sources=[len(it[0]) for it in items],
                          channels=[1 if it[0][0].ndim == 2 else 3 for it in items], which=[it[5] for it in items], given=[it[6] for it in items])

    def branches(self):
        r = self.reach
        return dict(pixels=r["pixels"], sources=r["sources"], channels=r["channels"], which=r["which"], given=r["given"],
                    nobody=[c[9] > 0 for c in r["counts"]], first=[c[0] > 0 for c in r["counts"]], later=[sum(c[1:9]) > 0 for c in r["counts"]])

    def stage(self, torch, share=None):
        self.ins, self.table, self.outs = [], [], {}
        for i, (srcs, models, (w, h), border, fill, which, cnt) in enumerate(self.items):
            ch = 3 if srcs[0].ndim == 3 else 1
            row = [In.plane(torch, s.reshape(s.shape[0], ch * s.shape[1]), ch * s.shape[1] + 2 * (i + k) + 5, 1 + 2 * ((i + k) % 3), 0xEE) for k, s in enumerate(srcs)]
            self.ins += row
            self.table.append(row)
            self.outs[f"dst{i}"] = Guarded(np.uint8, 1, h, ch * w, ch * w + 3 * i + 7, 1 + 2 * (i % 2) + (i % 4 == 3))
            if which:
                self.outs[f"which{i}"] = Guarded(np.uint8, 1, h, w, w + i + 3, 1 + i % 4) if share is None else share.outs[f"which{i}"]
        self.outs["counts"] = Guarded(np.int64, len(self.items), 1, 10, 10, 1) if share is None else share.outs["counts"]
        self.works = []        # (d_which and d_counts are outputs: they are compared)

    def launch(self, stream):
        descs = (L.MosaicDesc * len(self.items))()
        for i, (srcs, models, (w, h), border, fill, which, cnt) in enumerate(self.items):
            d, ch = descs[i], 3 if srcs[0].ndim == 3 else 1
            for k, (src, m) in enumerate(zip(srcs, models)):
                s, p = d.source[k], self.table[i][k]
                s.d_src, s.src_pitch, s.sw, s.sh, s.model = p.ptr, p.pitch, src.shape[1], src.shape[0], (C.c_double * 9)(*m)
            dst = self.outs[f"dst{i}"]
            d.n_sources, d.d_dst, d.dst_pitch, d.w, d.h, d.channels, d.border, d.fill = len(srcs), dst.ptr, dst.pitch, w, h, ch, WP.BORDERS[border], fill
            d.d_which, d.which_pitch = (self.outs[f"which{i}"].ptr, self.outs[f"which{i}"].pitch) if which else (None, -1)
            d.d_counts = self.outs["counts"].slot(i) if cnt else None
        rc = self.lib().ofx_warp_mosaic(descs, len(self.items), stream)
        wipe(descs)
        return rc


# ---- flow median, prolongation --------------------------------------------------------------------------------------------------------
class Median(Recipe):
    entry = "ofx_flow_median"

    def __init__(self, name, items):
        """items: (kind, w, h, radius)"""
        super().__init__()
        self.name, self.items = name, items
        for i, (kind, w, h, r) in enumerate(items):
            self.want[f"field{i}"] = np.array(M.want(kind, w, h, r))
        self.reach = dict(tiles=[(-(-w // 256), -(-h // 16)) for _, w, h, _ in items])

    def branches(self):
        return dict(self.reach, radius=[it[3] for it in self.items])

    def stage(self, torch, share=None):
        self.ins = [In(torch, M.field_case(kind, w, h), 2 + 2 * i, 64) for i, (kind, w, h, r) in enumerate(self.items)]
        self.outs = {f"field{i}": Guarded(np.float32, 1, h, 2 * w, 2 * w, 4 - 2 * i) for i, (kind, w, h, r) in enumerate(self.items)}

    def launch(self, stream):
        descs = (L.MedianDesc * len(self.items))()
        for i, (kind, w, h, r) in enumerate(self.items):
            descs[i] = L.MedianDesc(self.ins[i].ptr, self.outs[f"field{i}"].ptr, w, h, r, float(D.P_SCALE), None, 0, None, 0)
        rc = self.lib().ofx_flow_median(descs, len(self.items), stream)
        wipe(descs)
        return rc


class Prolong(Recipe):
    entry = "ofx_flow_prolong"

    def __init__(self, name, kind, coarse, fine, flip=False):
        super().__init__()
        self.name, self.kind, self.coarse, self.fine = name, kind, coarse, fine
        self.field = D.coarse_case(kind, *coarse)
        if flip:          # the same values, each at the opposite pixel
            self.field = np.ascontiguousarray(self.field[::-1, ::-1])
        self.want["fine"] = D.prolong(self.field, fine[0], fine[1], D.P_SCALE, D.P_MAX_PX)
        self.reach = dict(nonfinite=int((~np.isfinite(self.field)).sum()), huge=int((np.abs(self.field) > 1e6).sum()))

    def branches(self):
        return {k: v > 0 for k, v in self.reach.items()}

    def stage(self, torch, share=None):
        self.ins = [In(torch, self.field, 2, 64)]
        self.outs = {"fine": Guarded(np.float32, 1, self.fine[1], 2 * self.fine[0], 2 * self.fine[0], 2)}

    def launch(self, stream):
        d = (L.ProlongDesc * 1)(L.ProlongDesc(self.ins[0].ptr, self.coarse[0], self.coarse[1], self.outs["fine"].ptr, self.fine[0], self.fine[1],
                                              float(D.P_SCALE), float(D.P_MAX_PX), None, 0, None, 0))
        rc = self.lib().ofx_flow_prolong(d, 1, stream)
        wipe(d)
        return rc


# ---- tracker: ofx_pyramid_1ch per frame, then ofx_track_points ----------------------------------------------------------------------
TRACK_SHAPE = (96, 64, 2)              # (w, h, levels)
TRACK_PRM = K.Params(9, 10, 1, K.lam_for(9), 200 * 81)


def pad4(w):
    return (w + 3) & ~3


class Track(Recipe):
    """frames[f0 : f0 + n_frames] of a clip: their pyramids by ofx_pyramid_1ch, then one ofx_track_points over them, pairs numbered
    from pair0.  start: (points, status) on entry."""
    entry = "ofx_track_points"

    def __init__(self, name, frames, start, pair0, f0=0, n_frames=None):
        super().__init__()
        w, h, self.levels = TRACK_SHAPE
        self.name, self.pair0 = name, pair0
        self.frames = frames[f0:f0 + (n_frames or len(frames))]
        self.start = start
        orc = oracle()
        self.pyr = [[np.ascontiguousarray(x[:, :, 0]) for x in orc.gauss_pyramid(synth.to_3ch(f), self.levels)] for f in self.frames]
        pts, status, hist, sad, stats = K.track_chain(self.pyr, start[0], start[1], pair0, TRACK_PRM)
        self.end = (pts, status)
        self.want = dict(points=pts, status=status, history=hist, sad=sad, stats=stats)
        for f in range(len(self.frames)):
            for k in range(1, self.levels):
                self.want[f"plane{f}_{k}"] = self.pyr[f][k]
        alive = start[1] == 0
        self.reach = dict(tracked=int((status[alive] == 0).sum()), lost=int((status[alive] != 0).sum()), n=len(pts))

    def branches(self):
        r = self.reach
        return dict(n=r["n"], tracked=r["tracked"] > 0, lost=r["lost"] > 0, frozen=int((self.start[1] != 0).sum()) > 0,
                    sad=[bool((self.want["sad"] >= 0).any()), bool((self.want["sad"] == -1).any())], alive_at_the_end=bool(self.want["stats"][-1, 0] > 0))

    def stage(self, torch, share=None):
        w, h, levels = TRACK_SHAPE
        n, pairs = len(self.start[0]), len(self.frames) - 1
        self.ins = [In.plane(torch, f, pad4(w) + 4, 4 + 4 * i, 0xEE) for i, f in enumerate(self.frames)]      # (one pitch per level for the clip)
        if share is None:
            self.outs = dict(points=Guarded(np.float32, 1, 1, 2 * n, 2 * n, 2), status=Guarded(np.int32, 1, 1, n, n, 1),
                             history=Guarded(np.float32, 1, pairs, 2 * n, 2 * n, 4), sad=Guarded(np.int32, 1, pairs, n, n, 3),
                             stats=Guarded(np.int64, 1, pairs, 7, 7, 1))
            self.loads = [InOut(torch, self.outs["points"], self.start[0]), InOut(torch, self.outs["status"], self.start[1])]
        else:      # the chain goes on in place: nothing is loaded, the first call's buffers hold the state
            self.outs = {k: share.outs[k] for k in ("points", "status", "history", "sad", "stats")}
            self.loads = []
        for f in range(len(self.frames)):
            for k in range(1, levels):
                self.outs[f"plane{f}_{k}"] = Guarded(np.uint8, 1, h >> k, w >> k, pad4(w >> k) + 4, 4 * (1 + k + f))

    def launch(self, stream):
        w, h, levels = TRACK_SHAPE
        lib = self.lib()
        nf = len(self.frames)
        for f in range(nf):
            planes = (C.c_void_p * levels)(None, *[self.outs[f"plane{f}_{k}"].ptr for k in range(1, levels)])
            pitches = (C.c_int * levels)(0, *[self.outs[f"plane{f}_{k}"].pitch for k in range(1, levels)])
            rc = lib.ofx_pyramid_1ch(self.ins[f].ptr, self.ins[f].pitch, w, h, planes, pitches, levels, stream)
            wipe(planes, pitches)
            if rc:
                return rc
        table = (C.c_void_p * (nf * levels))(*[self.ins[f].ptr if k == 0 else self.outs[f"plane{f}_{k}"].ptr for f in range(nf) for k in range(levels)])
        pitches = (C.c_int * levels)(self.ins[0].pitch, *[self.outs[f"plane0_{k}"].pitch for k in range(1, levels)])
        clip = L.TrackClip(w, h, levels, nf, table, pitches)
        prm = L.TrackParams(TRACK_PRM.window, TRACK_PRM.max_iters, TRACK_PRM.eps_q, TRACK_PRM.max_sad, TRACK_PRM.min_lambda)
        o = self.outs
        rc = lib.ofx_track_points(C.byref(clip), C.byref(prm), self.pair0, o["points"].ptr, o["status"].ptr, len(self.start[0]), o["history"].ptr,
                                  o["sad"].ptr, o["stats"].ptr, stream)
        wipe(table, pitches, clip, prm)
        return rc


# ---- texture strength, selection, compaction ------------------------------------------------------------------------------------------
FEAT_WIN, FEAT_CELL = 5, 16
FILL_F32 = np.frombuffer(bytes([FILL]) * 4, F32)[0]


class Features(Recipe):
    """ofx_texture_features (strength, cells, cell strengths, stats) then ofx_compact_features of its cells.  over=<a Features>: this
    call writes into that one's buffers, which are larger: what lies past this image's extent keeps that call's values."""
    entry = "ofx_texture_features"

    def __init__(self, name, img, over=None):
        super().__init__()
        self.name, self.img, self.over = name, img, over
        h, w = img.shape
        self.w, self.h = w, h
        self.ncx, self.ncy = T.grid(w, h, FEAT_CELL)
        self.border = T.default_border(FEAT_WIN)
        R = T.strength(oracle(), img, FEAT_WIN)
        cells, cs, stats = T.select(R, FEAT_CELL, self.border, 0.0)
        pts, occupied = T.compact(cells)
        first = over or self
        self.max_points = first.ncx * first.ncy
        if over is None:
            points = np.full((self.max_points, 2), FILL_F32, F32)
            want = dict(strength=R, cells=cells, cell_strength=cs)
        else:
            points = over.want["points"].copy()
            want = {k: over.want[k].copy() for k in ("strength", "cells", "cell_strength")}
            want["strength"][:h, :w] = R
            want["cells"].reshape(-1)[:cells.size] = cells.reshape(-1)
            want["cell_strength"].reshape(-1)[:cs.size] = cs.reshape(-1)
        points[:occupied] = pts
        self.want = dict(want, stats=stats, points=points, count=np.array([occupied], np.int32))
        self.reach = dict(cells=int(stats[0]), occupied=int(stats[1]), blocks=(-(-w // (256 - 2 * (FEAT_WIN // 2))), -(-h // T.STRIP)))

    def branches(self):
        r = self.reach
        return dict(cells=r["cells"], blocks=r["blocks"], some=0 < r["occupied"] < r["cells"])

    def want_over(self, prev):
        points = prev.want["points"].copy()          # entries beyond the count are left alone: they keep prev's
        points[:self.reach["occupied"]] = self.want["points"][:self.reach["occupied"]]
        return dict(self.want, points=points)

    def stage(self, torch, share=None):
        assert (share is None) == (self.over is None)
        self.ins = [In.plane(torch, self.img, pad4(self.w) + 4, 8, 0xEE)]
        if share is None:
            w, h = self.w, self.h
            self.sp = w + 3
            self.outs = dict(strength=Guarded(np.float32, 1, h, w, self.sp, 4), cells=Guarded(np.int32, 1, self.ncy, 2 * self.ncx, 2 * self.ncx, 2),
                             cell_strength=Guarded(np.float32, 1, self.ncy, self.ncx, self.ncx, 3), stats=Guarded(np.int64, 1, 1, 4, 4, 1),
                             points=Guarded(np.float32, 1, 1, 2 * self.max_points, 2 * self.max_points, 2), count=Guarded(np.int32, 1, 1, 1, 1, 1))
        else:
            self.sp, self.outs = share.sp, dict(share.outs)

    def launch(self, stream):
        o = self.outs
        d = (L.TextureDesc * 1)(L.TextureDesc(self.ins[0].ptr, self.ins[0].pitch, self.w, self.h, o["strength"].ptr, self.sp, o["cells"].ptr,
                                              o["cell_strength"].ptr, o["stats"].ptr, FEAT_CELL, self.border, 0.0))
        rc = self.lib().ofx_texture_features(d, 1, FEAT_WIN, stream)
        wipe(d)
        if rc:
            return rc
        return self.lib().ofx_compact_features(o["cells"].ptr, self.ncx * self.ncy, self.max_points, o["points"].ptr, o["count"].ptr, stream)


# ---- pixel displacement, frame interpolation, consistency, motion compensation --------------------------------------------------------
UV = (3.7, -2.2)


class Displacement(Recipe):
    entry = "ofx_flow_displacement"

    def __init__(self, name, w, h, kind="nonfinite", flip=False):
        super().__init__()
        self.name, self.w, self.h = name, w, h
        self.flow = IR.flow_case(kind, w, h)
        if flip:          # the same values, each at the opposite pixel
            self.flow = np.ascontiguousarray(self.flow[::-1, ::-1])
        self.want["disp"] = IR.displacement(self.flow, UV, IR.ITER_SCALE)
        self.reach = dict(nonfinite=int((~np.isfinite(self.flow)).sum()), huge=int((np.abs(self.flow) > 1e6).sum()),
                          nonfinite_out=int((~np.isfinite(self.want["disp"])).sum()))

    def branches(self):
        return {k: v > 0 for k, v in self.reach.items()}

    def stage(self, torch, share=None):
        self.ins = [In(torch, self.flow, 2, 64), In(torch, np.array(UV, F32), 1)]
        self.outs = {"disp": Guarded(np.float32, 1, self.h, 2 * self.w, 2 * self.w, 2)}

    def launch(self, stream):
        return self.lib().ofx_flow_displacement(self.ins[0].ptr, self.w, self.h, self.ins[1].ptr, float(IR.ITER_SCALE), self.outs["disp"].ptr, stream)


class Interp(Recipe):
    """ofx_interpolate_frames_batch, or with colour ofx_interpolate_frames_3ch_batch: pairs (kind, seed) at TIME_SETS[1], stats given"""

    def __init__(self, name, w, h, pairs, colour):
        super().__init__()
        self.name, self.w, self.h, self.pairs, self.colour = name, w, h, pairs, colour
        self.entry = "ofx_interpolate_frames_3ch_batch" if colour else "ofx_interpolate_frames_batch"
        self.times = np.array(IR.TIME_SETS[1], F32)
        ref = [(I3.reference3 if colour else IR.reference)(kind, w, h, 1, seed) for kind, seed in pairs]
        self.want["frames"] = np.concatenate([r[0] for r in ref]).reshape(len(pairs) * len(self.times), h, -1)
        self.want["stats"] = np.stack([r[1] for r in ref]).reshape(len(pairs), 1, -1)
        self.reach = dict(classes=self.want["stats"].reshape(-1, 4)[:, 1:].sum(0).tolist())

    def branches(self):
        return dict(classes=[c > 0 for c in self.reach["classes"]], pairs=len(self.pairs), times=self.times.tolist())

    def stage(self, torch, share=None):
        w, h, c = self.w, self.h, 3 if self.colour else 1
        n, T_ = len(self.pairs), len(self.times)
        self.ins, self.table = [], []
        for i, (kind, seed) in enumerate(self.pairs):
            a, b = (I3.planes3 if self.colour else IR.planes)(w, h, seed)
            dab, dba = IR.field_case(kind, w, h, seed)
            row = [In.plane(torch, a.reshape(h, c * w), c * w + 5 + i, 3 + i, 0xEE), In.plane(torch, b.reshape(h, c * w), c * w + 2 * i, 1, 0xEE),
                   In(torch, dab, 2, 64), In(torch, dba, 4, 64)]
            self.ins += row
            self.table.append(row)
        self.outs = {"frames": Guarded(np.uint8, n * T_, h, c * w, c * w + 9, 3)}
        self.outs["stats"] = Guarded(np.int64, n, 1, 4 * T_, 4 * T_, 1) if share is None else share.outs["stats"]

    def launch(self, stream):
        n, T_ = len(self.pairs), len(self.times)
        ptrs = lambda f: (C.c_void_p * n)(*[f(i) for i in range(n)])            # noqa: E731
        ints = lambda f: (C.c_int * n)(*[f(i) for i in range(n)])               # noqa: E731
        t = self.times.copy()
        fr, st = self.outs["frames"], self.outs["stats"]
        host = [ptrs(lambda i: self.table[i][0].ptr), ints(lambda i: self.table[i][0].pitch), ptrs(lambda i: self.table[i][1].ptr),
                ints(lambda i: self.table[i][1].pitch), ptrs(lambda i: self.table[i][2].ptr), ptrs(lambda i: self.table[i][3].ptr),
                ptrs(lambda i: fr.slot(i * T_)), ptrs(lambda i: st.slot(i))]
        fn = self.lib().ofx_interpolate_frames_3ch_batch if self.colour else self.lib().ofx_interpolate_frames_batch
        rc = fn(host[0], host[1], host[2], host[3], n, self.w, self.h, host[4], host[5], t.ctypes.data_as(C.POINTER(C.c_float)), T_, host[6], fr.pitch,
                fr.stride, host[7], stream)
        wipe(t, *host)
        return rc


class Consistency(Recipe):
    entry = "ofx_flow_consistency_batch"

    def __init__(self, name, w, h, pairs):
        super().__init__()
        self.name, self.w, self.h, self.pairs = name, w, h, pairs
        self.fields = [CR.field_case(kind, w, h, seed) for kind, seed in pairs]
        self.scale = self.fields[0][2]
        assert all(f[2] == self.scale for f in self.fields)
        self.alpha, self.beta = CR.tolerances(self.scale)[0]
        ref = [CR.reference(kind, w, h, 0, seed) for kind, seed in pairs]
        self.want = dict(mask=np.stack([r[0] for r in ref]), err=np.stack([r[1] for r in ref]), stats=np.stack([r[2] for r in ref]).reshape(len(pairs), 1, 4))
        self.reach = dict(classes=self.want["stats"].reshape(-1, 4)[:, 1:].sum(0).tolist())

    def branches(self):
        return dict(classes=[c > 0 for c in self.reach["classes"]], pairs=len(self.pairs), host=(float(self.scale), float(self.alpha), float(self.beta)))

    def stage(self, torch, share=None):
        n, w, h = len(self.pairs), self.w, self.h
        self.ins = [In(torch, f[j], 2 + 2 * j, 64) for f in self.fields for j in (0, 1)]
        self.outs = dict(mask=Guarded(np.uint8, n, h, w, w + 6, 3), err=Guarded(np.float32, n, h, w, w, 1))
        self.outs["stats"] = Guarded(np.int64, n, 1, 4, 4, 1) if share is None else share.outs["stats"]

    def launch(self, stream):
        n = len(self.pairs)
        o = self.outs
        host = [(C.c_void_p * n)(*[self.ins[2 * i].ptr for i in range(n)]), (C.c_void_p * n)(*[self.ins[2 * i + 1].ptr for i in range(n)])]
        host += [(C.c_void_p * n)(*[o[k].slot(i) for i in range(n)]) for k in ("mask", "err", "stats")]
        rc = self.lib().ofx_flow_consistency_batch(host[0], host[1], n, self.w, self.h, float(self.scale), float(self.alpha), float(self.beta), host[2],
                                                   o["mask"].pitch, host[3], host[4], stream)
        wipe(*host)
        return rc


class Motion(Recipe):
    entry = "ofx_motion_compensate"

    def __init__(self, name, w, h, seed, kind="nonfinite"):
        super().__init__()
        self.name, self.w, self.h = name, w, h
        self.prev, self.next = MR.planes(w, h, seed)
        self.flow, self.scale = MR.flow_case(kind, w, h, seed)
        mc, stats = MR.motion(self.prev, self.next, self.flow, UV, self.scale)
        self.want = dict(mc=mc.reshape(1, h, w), stats=stats.reshape(1, 1, 4))
        self.reach = dict(not_warped=int(stats[3]))

    def branches(self):
        return dict(some=0 < self.reach["not_warped"] < self.w * self.h, host=float(self.scale))

    def stage(self, torch, share=None):
        w, h = self.w, self.h
        self.ins = [In.plane(torch, self.prev, w + 11, 5, 0xEE), In.plane(torch, self.next, w + 22, 3, 0xEE), In(torch, self.flow, 2, 64),
                    In(torch, np.array(UV, F32), 1)]
        self.outs = {"mc": Guarded(np.uint8, 1, h, w, w + 9, 61)}
        self.outs["stats"] = Guarded(np.int64, 1, 1, 4, 4, 1) if share is None else share.outs["stats"]

    def launch(self, stream):
        i, o = self.ins, self.outs
        return self.lib().ofx_motion_compensate(i[0].ptr, i[0].pitch, i[1].ptr, i[1].pitch, self.w, self.h, i[2].ptr, i[3].ptr, float(self.scale), o["mc"].ptr,
                                                o["mc"].pitch, o["stats"].ptr, stream)


# ---- the composed field, its arrows, points moved through it --------------------------------------------------------------------------
SAMPLED = (96, 64, 3, 0)           # (W, H, levels, level)
ARROW_RES = 12


class Sampled(Recipe):
    """ofx_compose_flow, ofx_sample_arrows and ofx_advect_points on one flow pyramid; start: (points, status) on entry"""
    entry = "ofx_advect_points"

    def __init__(self, name, seed, start, pair):
        super().__init__()
        W, H, Lv, lv = SAMPLED
        self.name, self.pair, self.start = name, pair, start
        self.pyr = SR.synth_pyramid(W, H, Lv, lv, seed, 0.04 * W)
        Cf = SR.compose(self.pyr, Lv, lv)
        pts, st = SR.advect(Cf, start[0], start[1], pair)
        self.end = (pts, st)
        self.want = dict(composed=Cf, arrows=SR.arrows(Cf, ARROW_RES), points=pts, status=st)
        alive = start[1] == 0
        self.reach = dict(moved=int((st[alive] == 0).sum()), lost=int((st[alive] != 0).sum()))

    def branches(self):
        return dict(moved=self.reach["moved"] > 0, lost=self.reach["lost"] > 0, n=len(self.start[0]), frozen=int((self.start[1] != 0).sum()),
                    not_drawn=bool((self.want["arrows"][..., 2] == -1).any()))

    def stage(self, torch, share=None):
        W, H, Lv, lv = SAMPLED
        n = len(self.start[0])
        _, ny, nx = SR.arrow_grid(W, H, ARROW_RES)
        self.ins = [In(torch, f, 2, 64) for f in self.pyr]
        self.outs = dict(composed=Guarded(np.float32, 1, H, 2 * W, 2 * W, 2), arrows=Guarded(np.int32, 1, ny, 4 * nx, 4 * nx, 4))
        if share is None:
            self.outs.update(points=Guarded(np.float32, 1, 1, 2 * n, 2 * n, 2), status=Guarded(np.int32, 1, 1, n, n, 1))
            self.loads = [InOut(torch, self.outs["points"], self.start[0]), InOut(torch, self.outs["status"], self.start[1])]
        else:
            self.outs.update(points=share.outs["points"], status=share.outs["status"])
            self.loads = []

    def launch(self, stream):
        W, H, Lv, lv = SAMPLED
        lib, o = self.lib(), self.outs
        table = lambda: (C.c_void_p * Lv)(*[i.ptr for i in self.ins])          # noqa: E731
        for call in (lambda t: lib.ofx_compose_flow(t, W, H, Lv, lv, o["composed"].ptr, stream),
                     lambda t: lib.ofx_sample_arrows(t, W, H, Lv, lv, ARROW_RES, o["arrows"].ptr, stream),
                     lambda t: lib.ofx_advect_points(t, W, H, Lv, lv, self.pair, o["points"].ptr, o["status"].ptr, len(self.start[0]), stream)):
            t = table()
            rc = call(t)
            wipe(t)
            if rc:
                return rc
        return 0


def sampled_start(n=40, seed=5):
    W, H, _, _ = SAMPLED
    pts = SR.synth_points(W, H, n, seed)
    st = np.zeros(n, np.int32)
    st[[n // 2, n - 1]] = (7, -3)
    return pts, st


# ---- a whole pair by the LK calls (tests/test_gpu_lk_abi.py: test_a_whole_pair_by_stateless_calls) -------------------------------------
class LkPair(Recipe):
    """lk_float: two ofx_pyramid_1ch, ofx_corner_flows, ofx_lk_levels with d_uv, then ofx_shift_levels, ofx_warp_levels, ofx_lk_levels with
    accumulate and d_warp_out, ofx_lk_levels with accumulate (three iterations, against Oracle.flow_pair_iter).  compat_cpu has no
    refinement iterations: the chain ends after the first ofx_lk_levels (against Oracle.flow_pair)."""
    entry = "ofx_lk_levels"

    def __init__(self, name, mode, swap=False):
        super().__init__()
        c = LK.PAIR
        self.name, self.mode = name, mode
        self.w, self.h, self.L, self.win = c["w"], c["h"], c["levels"], c["win"]
        p, n = LK.pair_frames()
        self.frames = (n, p) if swap else (p, n)
        orc = oracle()
        if mode == "lk_float":
            flows = orc.flow_pair_iter(self.frames[0], self.frames[1], self.L, self.win, c["iters"])
        else:
            flows = orc.flow_pair(synth.to_3ch(self.frames[0]), synth.to_3ch(self.frames[1]), self.L, self.win, mode, exact_sums=True)[0]
        self.want = {f"flow{k}": np.ascontiguousarray(flows[k], F32) for k in range(self.L)}
        self.reach = dict(nonfinite=int(sum((~np.isfinite(f)).sum() for f in flows)))

    def branches(self):
        return dict(nonfinite=self.reach["nonfinite"] > 0)

    def stage(self, torch, share=None):
        w, h, Lv = self.w, self.h, self.L
        self.ins = [In.plane(torch, f, pad4(w), 4, 0xEE) for f in self.frames]
        self.outs = {f"flow{k}": Guarded(np.float32, 1, h >> k, 2 * (w >> k), 2 * (w >> k), 2) for k in range(Lv)}
        if share is None:
            plane = lambda k: work(torch, (h >> k) * pad4(w >> k))               # noqa: E731
            self.pyr = [[None] + [plane(k) for k in range(1, Lv)] for _ in (0, 1)]
            self.uv = work(torch, 8 * Lv)
            self.shifted = [plane(k) for k in range(Lv)]
            self.warped = [[plane(k) for k in range(Lv)] for _ in (0, 1)]
            self.works = [t for fr in self.pyr for t in fr[1:]] + [self.uv] + self.shifted + self.warped[0] + self.warped[1]
        else:
            self.pyr, self.uv, self.shifted, self.warped, self.works = share.pyr, share.uv, share.shifted, share.warped, share.works

    def launch(self, stream):
        w, h, Lv, win = self.w, self.h, self.L, self.win
        lib, mode = self.lib(), L.MODES[self.mode]
        scale = float(LK.ITER_SCALE)
        for f in (0, 1):
            planes = (C.c_void_p * Lv)(None, *[t.data_ptr() for t in self.pyr[f][1:]])
            pitches = (C.c_int * Lv)(0, *[pad4(w >> k) for k in range(1, Lv)])
            rc = lib.ofx_pyramid_1ch(self.ins[f].ptr, self.ins[f].pitch, w, h, planes, pitches, Lv, stream)
            wipe(planes, pitches)
            if rc:
                return rc
        pl = [[self.ins[f].ptr] + [t.data_ptr() for t in self.pyr[f][1:]] for f in (0, 1)]
        geom = lambda k: L.Geom.full(w >> k, h >> k, pad4(w >> k))              # noqa: E731
        flow = [self.outs[f"flow{k}"].ptr for k in range(Lv)]
        uvp = lambda k: None if k == Lv - 1 else self.uv.data_ptr() + 8 * k      # noqa: E731

        def lk(nxt, acc, wsrc=None, wout=None, with_uv=False):
            d = (L.LkDesc * Lv)(*[L.LkDesc(pl[0][k], nxt[k], geom(k), flow[k], 0, uvp(k) if with_uv else None, acc, 0.0, wsrc and wsrc[k], wout and wout[k],
                                           scale, None, 0) for k in range(Lv - 1, -1, -1)])
            rc = lib.ofx_lk_levels(d, Lv, win, mode, stream)
            wipe(d)
            return rc

        d = (L.LkDesc * Lv)(*[L.LkDesc(pl[0][k], pl[1][k], geom(k), flow[k], 0, None, 0, 0.0, None, None, 0.0, None, 0) for k in range(Lv)])
        rc = lib.ofx_corner_flows(d, Lv, win, mode, self.uv.data_ptr(), stream)
        wipe(d)
        rc = rc or lk(pl[1], 0, with_uv=True)
        if rc or self.mode != "lk_float":
            return rc
        sd = (L.ShiftDesc * (Lv - 1))(*[L.ShiftDesc(pl[1][k], self.shifted[k].data_ptr(), geom(k), uvp(k)) for k in range(Lv - 1)])
        rc = lib.ofx_shift_levels(sd, Lv - 1, stream)
        wipe(sd)
        if rc:
            return rc
        wsrc = [self.shifted[k].data_ptr() for k in range(Lv - 1)] + [pl[1][Lv - 1]]
        w0, w1 = ([t.data_ptr() for t in self.warped[j]] for j in (0, 1))
        wd = (L.WarpDesc * Lv)(*[L.WarpDesc(wsrc[k], w0[k], geom(k), flow[k], 0, scale, None, 0) for k in range(Lv)])
        rc = lib.ofx_warp_levels(wd, Lv, stream)
        wipe(wd)
        return rc or lk(w0, 1, wsrc, w1) or lk(w1, 1)


# ---- the colour front end -------------------------------------------------------------------------------------------------------------
GREY, BILATERAL = 1, 2


class Frontend(Recipe):
    entry = "ofx_frontend_1ch"

    def __init__(self, name, w, h, seed):
        super().__init__()
        self.name, self.w, self.h, self.win = name, w, h, 5
        rng = np.random.default_rng(seed)
        self.imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in (0, 1)]
        self.modes = [GREY, BILATERAL]
        orc = oracle()
        for i, (img, mode) in enumerate(zip(self.imgs, self.modes)):
            g = orc.grayscale_avg(img)
            self.want[f"plane{i}"] = np.ascontiguousarray((g if mode == GREY else orc.bilateral_3ch(g, g, self.win, self.win, 2.0, 10.0))[:, :, 0]).reshape(1, h, w)

    def stage(self, torch, share=None):
        w, h = self.w, self.h
        self.ins = [In.plane(torch, img.reshape(h, 3 * w), 3 * w + 4 * i + 3, 4 + 4 * i, 0xEE) for i, img in enumerate(self.imgs)]
        self.outs = {f"plane{i}": Guarded(np.uint8, 1, h, w, w + 7 * i, 1 + i) for i in range(2)}

    def launch(self, stream):
        n = 2
        host = [(C.c_void_p * n)(*[i.ptr for i in self.ins]), (C.c_int * n)(*[i.pitch for i in self.ins]),
                (C.c_void_p * n)(*[self.outs[f"plane{i}"].ptr for i in range(n)]), (C.c_int * n)(*[self.outs[f"plane{i}"].pitch for i in range(n)]),
                (C.c_int * n)(*self.modes)]
        rc = self.lib().ofx_frontend_1ch(host[0], host[1], 0, host[2], host[3], 0, n, self.w, self.h, host[4], 0, self.win, 2.0, 10.0, stream)
        wipe(*host)
        return rc


# ---- displacement chain ---------------------------------------------------------------------------------------------------------------
# (w, h, links, mask: None / "loose" / "odd", d_stats given, in place): six items, ONE launch of the batched grid
CHAIN_GEOM = [(257, 40, 3, "odd", True, False), (67, 33, 2, "loose", False, True), (130, 9, 4, None, True, False), (5, 3, 2, "odd", True, True),
              (1, 1, 2, None, False, False), (67, 33, 4, "loose", True, False)]
CHAIN_KINDS = ["borders", "nonfinite", "edge", "inverse", "integers", "overflow"]


def chain_items(seed=0, turn=0):
    """the table's items (links, mask, stats given, in place), item i with kind i + turn"""
    return [(KC.links(CHAIN_KINDS[(i + turn) % len(CHAIN_KINDS)], w, h, n, seed), mask, given, there) for i, (w, h, n, mask, given, there) in enumerate(CHAIN_GEOM)]


class Chain(Recipe):
    """ofx_displacement_chain on items (links, mask, stats given, in place).  The stats slots are consecutive in memory (ONE Guarded
    without a gap between its slots), item i at slot slots[i]: zero_stats merges slots that follow one another into one launch, and
    the slot of an item that gave NULL keeps its 0x5A.  An in-place item has ONE Guarded that is link 0 and d_dst, loaded with
    link 0 through InOut; with carried, nothing is loaded: link 0 is what the call before left there.
    The table's 1 x 1 item leaves the frame whatever the seed (only a link 0 of exactly zero stays): its dst is the dead vector in the
    row, the variant and the second instance alike, so it never tells the three apart in a replay or between two calls in flight.
    What it holds is the store of a one-pixel item (the guard bytes around it) and its stats slot, which was not given and keeps
    its 0x5A; tests/test_call_order_cases.py asserts that it is the dead vector in all three."""
    entry = "ofx_displacement_chain"

    def __init__(self, name, items, slots=None, carried=False):
        super().__init__()
        self.name, self.items, self.carried = name, items, carried
        self.slots = list(range(len(items))) if slots is None else list(slots)
        res = [KR.chain(list(links)) for links, _, _, _ in items]
        stats = np.full((len(items), 1, 4), COUNTS_LEFT, np.int64)
        for i, ((links, mask, given, there), (dst, cls, st)) in enumerate(zip(items, res)):
            h, w, _ = links[0].shape
            self.want[f"dst{i}"] = dst.reshape(1, h, 2 * w)
            if mask is not None:
                self.want[f"mask{i}"] = cls.reshape(1, h, w)
            if given:
                stats[self.slots[i], 0] = st
        self.want["stats"] = stats
        self.end = res[0][0]
        self.reach = dict(sizes=[it[0][0].shape[1::-1] for it in items], links=[len(it[0]) for it in items], masks=[it[1] for it in items],
                          given=[it[2] for it in items], there=[it[3] for it in items], stats=[r[2].tolist() for r in res])

    def branches(self):
        r = self.reach
        return dict(sizes=r["sizes"], links=r["links"], masks=r["masks"], given=r["given"], there=r["there"], slots=self.slots,
                    classes=[[c > 0 for c in s[1:]] for s in r["stats"]])

    def stage(self, torch, share=None):
        self.ins, self.loads, self.rows, self.outs = [], [], [], {}
        for i, (links, mask, given, there) in enumerate(self.items):
            h, w, _ = links[0].shape
            row = [None if there and k == 0 else In(torch, f, 2 if (i + k) % 3 else 6) for k, f in enumerate(links)]     # 8 or 24 bytes in: never 16
            self.ins += [t for t in row if t is not None]
            self.rows.append(row)
            if share is None:
                self.outs[f"dst{i}"] = Guarded(np.float32, 1, h, 2 * w, 2 * w, 2 + 4 * (i % 2))
                if mask is not None:
                    self.outs[f"mask{i}"] = Guarded(np.uint8, 1, h, w, (w + 11) & ~3, 4) if mask == "loose" else Guarded(np.uint8, 1, h, w, (w + 5) | 1, 1 + 2 * (i % 2))
            else:
                self.outs.update({k: share.outs[k] for k in (f"dst{i}", f"mask{i}") if k in self.want})
            if there and not self.carried:
                self.loads.append(InOut(torch, self.outs[f"dst{i}"], links[0]))
        self.outs["stats"] = Guarded(np.int64, len(self.items), 1, 4, 4, 1, 4) if share is None else share.outs["stats"]
        self.works = []

    def launch(self, stream):
        descs = (L.ChainDesc * len(self.items))()
        for i, (links, mask, given, there) in enumerate(self.items):
            d, dst = descs[i], self.outs[f"dst{i}"]
            h, w, _ = links[0].shape
            for k, t in enumerate(self.rows[i]):
                d.d_link[k] = dst.ptr if t is None else t.ptr
            d.n_links, d.w, d.h, d.d_dst = len(links), w, h, dst.ptr
            d.d_mask, d.mask_pitch = (self.outs[f"mask{i}"].ptr, self.outs[f"mask{i}"].pitch) if mask is not None else (None, -1)
            d.d_stats = self.outs["stats"].slot(self.slots[i]) if given else None
        rc = self.lib().ofx_displacement_chain(descs, len(self.items), stream)
        wipe(descs)
        return rc


# ---- temporal noise filter ------------------------------------------------------------------------------------------------------------
# (w, h, channels, neighbours, field kind, same, own, d_stats given): six items, which take the 16-item instance of csrc/temporal.hip
TEMPORAL_GEOM = [(131, 9, 1, 4, "special", False, False, True), (67, 9, 3, 2, "ramp", False, False, True), (5, 3, 1, 1, "edge", False, False, False),
                 (67, 9, 1, 3, "random", True, False, True), (3, 2, 3, 2, "whole", False, True, False), (131, 9, 3, 3, "random", False, False, True)]


def temporal_items(table, wc, base=0, rows=range(len(TEMPORAL_GEOM))):
    """temporal_cases.case(...) + (stats given,) of the table's rows, the item at position i of the call with seed base + 2 i"""
    out = []
    for pos, row in enumerate(rows):
        w, h, ch, S, kind, same_, own, given = TEMPORAL_GEOM[row]
        out.append(TC.case(w, h, ch, S, kind, table, wc, seed=base + 2 * pos, same=same_, own=own) + (given,))
    return out


class Temporal(Recipe):
    """ofx_temporal_filter on items (name, centre, planes, fields, table, centre weight, stats given), one table for the call.  A plane
    that IS the centre or an earlier plane (the same array) is staged once.  Pitches are odd, so that the rows of a plane start at
    every address mod 4.  The stats slot of an item that gave NULL keeps its 0x5A."""
    entry = "ofx_temporal_filter"

    def __init__(self, name, items):
        super().__init__()
        self.name, self.items = name, items
        self.weights, self.wc = np.asarray(items[0][4]), int(items[0][5])
        with np.errstate(all="ignore"):
            res = [TR.temporal_filter(c, planes, fields, self.weights, self.wc) for _, c, planes, fields, _, _, _ in items]
        stats = np.full((len(items), 1, 8), COUNTS_LEFT, np.int64)
        for i, (it, (out, st)) in enumerate(zip(items, res)):
            self.want[f"dst{i}"] = out.reshape(1, out.shape[0], -1)
            if it[6]:
                stats[i, 0] = st
        self.want["stats"] = stats
        self.reach = dict(sizes=[it[1].shape[1::-1] for it in items], channels=[3 if it[1].ndim == 3 else 1 for it in items], neighbours=[len(it[2]) for it in items],
                          given=[it[6] for it in items], stats=[r[1].tolist() for r in res], same=[len(it[2]) > 1 and it[2][1] is it[2][0] for it in items],
                          own=[it[2][0] is it[1] for it in items])

    def branches(self):
        r = self.reach
        px = [w * h for w, h in r["sizes"]]
        return dict(sizes=r["sizes"], channels=r["channels"], neighbours=r["neighbours"], given=r["given"], same=r["same"], own=r["own"],
                    table=self.weights.tolist(), wc=self.wc, instance=1 if len(self.items) == 1 else 16,
                    some=[[0 < u < p for u in s[1:1 + S]] for s, p, S in zip(r["stats"], px, r["neighbours"])], filled=[[v > 0 for v in s[5:]] for s in r["stats"]])

    def stage(self, torch, share=None):
        self.ins, self.staged, self.outs = [], [], {}
        for i, (_, centre, planes, fields, _, _, given) in enumerate(self.items):
            h, w = centre.shape[:2]
            ch = 3 if centre.ndim == 3 else 1
            made = {}

            def plane_of(a, k):
                if id(a) not in made:
                    made[id(a)] = In.plane(torch, a.reshape(h, ch * w), (ch * w + 4 + 2 * ((i + k) % 3)) | 1, 1 + (i + k) % 4, 0xEE)
                    self.ins.append(made[id(a)])
                return made[id(a)]

            cen = plane_of(centre, 0)
            nbs = [plane_of(p, 1 + k) for k, p in enumerate(planes)]
            flds = [In(torch, f, 2 if (i + k) % 3 else 6) for k, f in enumerate(fields)]
            self.ins += flds
            self.staged.append((cen, nbs, flds))
            self.outs[f"dst{i}"] = Guarded(np.uint8, 1, h, ch * w, ch * w + 3 * i + 7, 1 + 2 * (i % 2) + (i % 4 == 3)) if share is None else share.outs[f"dst{i}"]
        self.outs["stats"] = Guarded(np.int64, len(self.items), 1, 8, 8, 1) if share is None else share.outs["stats"]
        self.works = []

    def launch(self, stream):
        descs = (L.TemporalDesc * len(self.items))()
        for i, (_, centre, planes, fields, _, _, given) in enumerate(self.items):
            d, (cen, nbs, flds), dst = descs[i], self.staged[i], self.outs[f"dst{i}"]
            for k, (p, f) in enumerate(zip(nbs, flds)):
                s = d.neighbour[k]
                s.d_plane, s.pitch, s.pad, s.d_field = p.ptr, p.pitch, 0, f.ptr
            d.n_neighbours, d.w, d.h, d.channels = len(planes), centre.shape[1], centre.shape[0], 3 if centre.ndim == 3 else 1
            d.d_centre, d.centre_pitch, d.d_dst, d.dst_pitch = cen.ptr, cen.pitch, dst.ptr, dst.pitch
            d.d_stats = self.outs["stats"].slot(i) if given else None
        prm = temporal_params(self.weights, self.wc)
        rc = self.lib().ofx_temporal_filter(descs, len(self.items), C.byref(prm), stream)
        wipe(descs, prm)
        return rc


def temporal_params(table, wc):
    prm = L.TemporalParams()
    prm.weights = (C.c_uint16 * 256)(*[int(v) for v in table])
    prm.centre_weight, prm.reserved = int(wc), 0
    return prm


# ---- the two together: engine.denoise_rings(reach=2) by ABI calls -------------------------------------------------------------------------
DENOISE = (5, 67, 33, 10)           # (frames, w, h, sigma of the noise)


def denoise_rings(seed):
    """(fwd, bwd) float32 [4, h, w, 2] of the pan of temporal_cases.pan_clip (frame p shows the texture 3 p to the right and 2 p down:
    a pixel of frame p is found (3, 2) to the left and up in frame p + 1, and as far to the right and down in frame p - 1) plus
    N(0, 0.3); NaN in 3 % of fwd[1], +Inf in 3 % of bwd[2]: every two-link chain through them has vectors that are not defined"""
    N, w, h, _ = DENOISE
    rng = np.random.default_rng(900 + seed)
    fwd = (np.array([-3.0, -2.0]) + rng.normal(0.0, 0.3, (N - 1, h, w, 2))).astype(F32)
    bwd = (np.array([3.0, 2.0]) + rng.normal(0.0, 0.3, (N - 1, h, w, 2))).astype(F32)
    fwd[1][rng.random((h, w, 2)) < 0.03] = np.nan
    bwd[2][rng.random((h, w, 2)) < 0.03] = np.inf
    return fwd, bwd


class Denoise(Recipe):
    """engine.denoise_rings(reach=2) on a five-frame clip by ABI calls: ONE ofx_displacement_chain of six two-link items, which read
    their links in place out of the two rings and write fwd2[0 .. 2] and bwd2[0 .. 2], then ONE ofx_temporal_filter of the five
    frames, each with its neighbours in the engine's order (f - 1, f + 1, f - 2, f + 2, what lies outside the clip skipped), the far
    fields pointing into the slots the chain is still writing when the filter is enqueued."""
    entry = "ofx_temporal_filter"

    def __init__(self, name, channels, seed, table=None, wc=256):
        super().__init__()
        N, w, h, sigma = DENOISE
        self.name, self.channels, self.wc = name, channels, wc
        self.weights = TR.weights_for(float(sigma)) if table is None else np.asarray(table)
        self.frames = TC.pan_clip(N, w, h, channels, sigma, seed)[0]
        self.fwd, self.bwd = denoise_rings(seed)
        with np.errstate(all="ignore"):
            res = KR.denoise_rings(self.frames, self.fwd, self.bwd, self.weights, 2, wc)
        self.want = dict(fwd2=KR.chain_ring(self.fwd, 2).reshape(N - 2, h, 2 * w), bwd2=KR.chain_ring(self.bwd, 2).reshape(N - 2, h, 2 * w),
                         frames=np.stack([r[0] for r in res]).reshape(N, h, channels * w), stats=np.stack([r[1] for r in res]).reshape(N, 1, 8))
        self.reach = dict(stats=[r[1].tolist() for r in res], chains=[KR.chain([ring[p], ring[p + 1]])[2].tolist() for ring in (self.fwd, self.bwd) for p in range(N - 2)])

    def branches(self):
        r = self.reach
        return dict(channels=self.channels, table=self.weights.tolist(), wc=self.wc, neighbours=[[v > 0 for v in s[1:5]] for s in r["stats"]],
                    filled=[[v > 0 for v in s[5:]] for s in r["stats"]], chains=[[v > 0 for v in c[1:]] for c in r["chains"]])

    def stage(self, torch, share=None):
        N, w, h, _ = DENOISE
        row = self.channels * w
        self.planes = [In.plane(torch, f.reshape(h, row), (row + 4 + 2 * (i % 3)) | 1, 1 + i % 4, 0xEE) for i, f in enumerate(self.frames)]
        self.rings = [In(torch, self.fwd, 2), In(torch, self.bwd, 6)]
        self.ins = self.planes + self.rings
        if share is None:
            self.outs = dict(fwd2=Guarded(np.float32, N - 2, h, 2 * w, 2 * w, 2), bwd2=Guarded(np.float32, N - 2, h, 2 * w, 2 * w, 2),
                             frames=Guarded(np.uint8, N, h, row, row + 9, 3), stats=Guarded(np.int64, N, 1, 8, 8, 1))
        else:
            self.outs = dict(share.outs)
        self.works = []

    def launch(self, stream):
        N, w, h, _ = DENOISE
        o, field = self.outs, 8 * w * h
        chains = (L.ChainDesc * (2 * (N - 2)))()
        for j, (ring, out) in enumerate(zip(self.rings, (o["fwd2"], o["bwd2"]))):
            for p in range(N - 2):
                d = chains[(N - 2) * j + p]
                d.d_link[0], d.d_link[1] = ring.ptr + p * field, ring.ptr + (p + 1) * field
                d.n_links, d.w, d.h, d.mask_pitch, d.d_dst, d.d_mask, d.d_stats = 2, w, h, -1, out.slot(p), None, None
        rc = self.lib().ofx_displacement_chain(chains, len(chains), stream)
        wipe(chains)
        if rc:
            return rc
        fwd, bwd = (r.ptr for r in self.rings)
        descs = (L.TemporalDesc * N)()
        for f in range(N):
            near = ([(f - 1, bwd + (N - 1 - f) * field)] if f >= 1 else []) + ([(f + 1, fwd + f * field)] if f + 1 < N else []) + \
                   ([(f - 2, o["bwd2"].slot(N - 1 - f))] if f >= 2 else []) + ([(f + 2, o["fwd2"].slot(f))] if f + 2 < N else [])
            d = descs[f]
            for k, (g, at) in enumerate(near):
                s = d.neighbour[k]
                s.d_plane, s.pitch, s.pad, s.d_field = self.planes[g].ptr, self.planes[g].pitch, 0, at
            d.n_neighbours, d.w, d.h, d.channels = len(near), w, h, self.channels
            d.d_centre, d.centre_pitch, d.d_dst, d.dst_pitch, d.d_stats = self.planes[f].ptr, self.planes[f].pitch, o["frames"].slot(f), o["frames"].pitch, o["stats"].slot(f)
        prm = temporal_params(self.weights, self.wc)
        rc = self.lib().ofx_temporal_filter(descs, N, C.byref(prm), stream)
        wipe(descs, prm)
        return rc


# ---- the registry -----------------------------------------------------------------------------------------------------------------------
SIZE = (67, 45)
MODELS = ("translation", "similarity", "affine")


def track_frames(seed=17):
    w, h, _ = TRACK_SHAPE
    return [K.cosine_texture(w, h, sx, sy, seed=seed) for sx, sy in ((0.0, 0.0), (1.4, -0.8), (2.1, 0.3))]


def track_start(seed=0):
    w, h, _ = TRACK_SHAPE
    return K.points_for(w, h, 40, seed=seed)


def _fit(model, seed=9, H=33, refits=2, item_seed=1):
    hom = model == "homography"
    return Fit(f"fit-{model}", HR.HOMOGRAPHY if hom else FR.MODELS[model], fit_items(hom, item_seed), H, 32, refits, seed)


MAKERS = {
    "fit-translation": lambda: _fit("translation"),
    "fit-similarity": lambda: _fit("similarity"),
    "fit-affine": lambda: _fit("affine"),
    "fit-homography": lambda: _fit("homography"),
    "warp-affine": lambda: Warp("warp-affine", warp_items(False, _rot(64, 48), (1.0, 0.0, -33 / 32, 0.0, 1.0, -31 / 32))),
    "warp-perspective": lambda: Warp("warp-perspective", warp_items(True, _rot(64, 48, (1e-3, -5e-4, 1.0)), (1.0, 0.0, -33 / 32, 0.0, 1.0, -31 / 32))),
    "tracker": lambda: Track("tracker", track_frames(), track_start(), 1),
    "features": lambda: Features("features", T.make_input("hard", 97, 61)),
    "median": lambda: Median("median", [("salted", 67, 45, 2), ("ties", 67, 45, 2)]),
    "prolong": lambda: Prolong("prolong", "salted", (33, 17), (67, 35)),
    "displacement": lambda: Displacement("displacement", *SIZE),
    "interp": lambda: Interp("interp", *SIZE, [("borders", 0), ("nonfinite", 1)], False),
    "interp-colour": lambda: Interp("interp-colour", *SIZE, [("borders", 0), ("nonfinite", 1)], True),
    "consistency": lambda: Consistency("consistency", *SIZE, [("borders", 0), ("nonfinite", 1)]),
    "motion": lambda: Motion("motion", *SIZE, 3),
    "sampled": lambda: Sampled("sampled", 11, sampled_start(), 3),
    "lk-pair-lk_float": lambda: LkPair("lk-pair-lk_float", "lk_float"),
    "lk-pair-compat_cpu": lambda: LkPair("lk-pair-compat_cpu", "compat_cpu"),
    "frontend": lambda: Frontend("frontend", *SIZE, 21),
    "mosaic": lambda: Mosaic("mosaic", mosaic_items("ladder")),
    "chain": lambda: Chain("chain", chain_items()),
    "temporal": lambda: Temporal("temporal", temporal_items("random", 37)),
    "temporal-one": lambda: Temporal("temporal-one", temporal_items("random", 37, rows=[0])),
    "denoise-reach2": lambda: Denoise("denoise-reach2", 1, 0),
}
NAMES = list(MAKERS)

# recipe(name) on other device data: everything the host passes is the same
VARIANTS = {
    "fit-translation": lambda: _fit("translation", item_seed=7),
    "fit-similarity": lambda: _fit("similarity", item_seed=7),
    "fit-affine": lambda: _fit("affine", item_seed=7),
    "fit-homography": lambda: _fit("homography", item_seed=7),
    "warp-affine": lambda: Warp("warp-affine", warp_items(False, _rot(64, 48), (1.0, 0.0, -33 / 32, 0.0, 1.0, -31 / 32), seed=3)),
    "warp-perspective": lambda: Warp("warp-perspective", warp_items(True, _rot(64, 48, (1e-3, -5e-4, 1.0)), (1.0, 0.0, -33 / 32, 0.0, 1.0, -31 / 32), seed=3)),
    "tracker": lambda: Track("tracker", track_frames(seed=5)[::-1], track_start(seed=3), 1),
    "features": lambda: Features("features", T.make_input("noise", 97, 61)),
    "median": lambda: Median("median", [("ties", 67, 45, 2), ("salted", 67, 45, 2)]),
    "prolong": lambda: Prolong("prolong", "salted", (33, 17), (67, 35), flip=True),
    "displacement": lambda: Displacement("displacement", *SIZE, flip=True),
    "interp": lambda: Interp("interp", *SIZE, [("borders", 4), ("nonfinite", 5)], False),
    "interp-colour": lambda: Interp("interp-colour", *SIZE, [("borders", 4), ("nonfinite", 5)], True),
    "consistency": lambda: Consistency("consistency", *SIZE, [("borders", 4), ("nonfinite", 5)]),
    "motion": lambda: Motion("motion", *SIZE, 5),
    "sampled": lambda: Sampled("sampled", 12, sampled_start(seed=6), 3),
    "lk-pair-lk_float": lambda: LkPair("lk-pair-lk_float", "lk_float", swap=True),
    "lk-pair-compat_cpu": lambda: LkPair("lk-pair-compat_cpu", "compat_cpu", swap=True),
    "frontend": lambda: Frontend("frontend", *SIZE, 22),
    "mosaic": lambda: Mosaic("mosaic", mosaic_items("ladder", seed=100)),
    "chain": lambda: Chain("chain", chain_items(seed=1)),
    "temporal": lambda: Temporal("temporal", temporal_items("random", 37, base=50)),
    "temporal-one": lambda: Temporal("temporal-one", temporal_items("random", 37, base=50, rows=[0])),
    "denoise-reach2": lambda: Denoise("denoise-reach2", 1, 1),
}
assert list(VARIANTS) == NAMES


@functools.lru_cache(maxsize=None)
def variant(name):
    """the variant of the table's row, its referee's answer computed once"""
    v = VARIANTS[name]()
    v.name = name + " (variant)"
    return v


@functools.lru_cache(maxsize=None)
def recipe(name):
    """the recipe of the table's row, its referee's answer computed once"""
    return MAKERS[name]()


# a second instance of the same entry point, for two calls in flight (the first is recipe(name))
OTHERS = {
    "fit-similarity": lambda: Fit("fit-similarity-b", FR.MODELS["similarity"], fit_items(False, 7), 40, 16, 1, 77),
    "fit-homography": lambda: Fit("fit-homography-b", HR.HOMOGRAPHY, fit_items(True, 7), 40, 16, 1, 77),
    "warp-affine": lambda: Warp("warp-affine-b", warp_items(False, (0.9, 0.35, -1.7, -0.2, 1.05, 0.6), _rot(64, 48), seed=3)),
    "warp-perspective": lambda: Warp("warp-perspective-b", warp_items(True, (0.9, 0.35, -1.7, -0.2, 1.05, 0.6, -2e-3, 1e-3, 1.0), _rot(64, 48), seed=3)),
    "tracker": lambda: Track("tracker-b", track_frames(seed=5)[::-1], track_start(seed=3), 4),
    "median": lambda: Median("median-b", [("noise", 67, 45, 1), ("smooth", 67, 45, 2)]),
    "mosaic": lambda: Mosaic("mosaic-b", mosaic_items("steps", seed=50)),
    # the stats slots in descending order: no two follow one another, every slot is a zeroing launch of its own
    "chain": lambda: Chain("chain-b", chain_items(seed=3, turn=1), slots=range(len(CHAIN_GEOM) - 1, -1, -1)),
    "temporal": lambda: Temporal("temporal-b", temporal_items("sigma 10", 256, base=20)),
    "denoise-reach2": lambda: Denoise("denoise-reach2-b", 3, 2),
}


@functools.lru_cache(maxsize=None)
def other(name):
    return OTHERS[name]()


# ---- buffers reused: calls back to back that share their work, stats, counter or in-place buffers ----------------------------------------
def _fit_chain(model):
    hom = model == "homography"
    code = HR.HOMOGRAPHY if hom else FR.MODELS[model]
    mk = HC.matches if hom else motion_matches
    a, b = mk(4099, FIT_SIZE, 2), mk(65, (67, 45), 3, status=True)
    K_ = code + 1
    chain = [Fit(f"reuse-{model}-1", code, [(a[0], a[1], None, 0, FIT_SIZE)], 256, 32, 3, 9),
             Fit(f"reuse-{model}-2", code, [(b[0], b[1], b[2], 5, (67, 45))], 33, 32, 0, 1234),
             Fit(f"reuse-{model}-3", code, [few_item(3)], 33, 32, 2, 5)]
    if K_ <= 3:       # (three usable matches are few for a homography only: the other models get an item that is few for them as well)
        chain.append(Fit(f"reuse-{model}-4", code, [few_item(K_ - 1)], 33, 32, 2, 5))
    return chain


def _track_chain():
    frames, start = track_frames(), track_start()
    first = Track("reuse-tracker-1", frames, start, 1, 0, 2)
    return [first, Track("reuse-tracker-2", frames, first.end, 2, 1, 2)]


def _sampled_chain():
    first = Sampled("reuse-sampled-1", 11, sampled_start(), 3)
    return [first, Sampled("reuse-sampled-2", 12, first.end, 4)]


def _features_chain():
    first = Features("reuse-features-1", T.make_input("hard", 97, 61))
    return [first, Features("reuse-features-2", T.make_input("noise", 49, 33), over=first)]


def _chain_fold():
    """the left fold of four links, in place: the first call chains links 0 and 1 on the shared buffer, which it loads with link 0;
    the next two chain what the buffer holds with links 2 and 3.  One mask and one stats slot for all three."""
    links = KC.links("borders", 257, 40, 4)
    fold = [Chain("reuse-chain-1", [(links[:2], "odd", True, True)])]
    for j in (2, 3):
        h, w, _ = links[0].shape
        fold.append(Chain(f"reuse-chain-{j}", [((fold[-1].end.reshape(h, w, 2), links[j]), "odd", True, True)], carried=True))
    return fold


TEMPORAL_REUSE = [("all 256", 1, 0), ("all 0", 256, 7), ("sigma 10", 256, 13)]        # (table, centre weight, base seed) of the three calls


CHAINS = {
    "fit-translation": lambda: _fit_chain("translation"),
    "fit-similarity": lambda: _fit_chain("similarity"),
    "fit-affine": lambda: _fit_chain("affine"),
    "fit-homography": lambda: _fit_chain("homography"),
    "warp-affine": lambda: [Warp("reuse-warp-affine-1", warp_items(False, FAR, FAR)), Warp("reuse-warp-affine-2", warp_items(False, INSIDE, INSIDE, seed=3))],
    "warp-perspective": lambda: [Warp("reuse-warp-perspective-1", warp_items(True, FAR, FAR)),
                                 Warp("reuse-warp-perspective-2", warp_items(True, INSIDE_P, INSIDE_P, seed=3))],
    "tracker": _track_chain,
    "features": _features_chain,
    "interp": lambda: [Interp("reuse-interp-1", *SIZE, [("borders", 0), ("nonfinite", 1)], False), Interp("reuse-interp-2", *SIZE, [("inverse", 2), ("borders", 3)], False)],
    "interp-colour": lambda: [Interp("reuse-interp-colour-1", *SIZE, [("borders", 0), ("nonfinite", 1)], True),
                              Interp("reuse-interp-colour-2", *SIZE, [("inverse", 2), ("borders", 3)], True)],
    "consistency": lambda: [Consistency("reuse-consistency-1", *SIZE, [("borders", 0), ("nonfinite", 1)]),
                            Consistency("reuse-consistency-2", *SIZE, [("inverse", 2), ("borders", 3)])],
    "motion": lambda: [Motion("reuse-motion-1", *SIZE, 3), Motion("reuse-motion-2", *SIZE, 4, "borders")],
    "sampled": _sampled_chain,
    "lk-pair-lk_float": lambda: [LkPair("reuse-lk-pair-1", "lk_float"), LkPair("reuse-lk-pair-2", "lk_float", swap=True)],
    # the d_counts slots and the d_which planes shared: few pixels covered, then most
    "mosaic": lambda: [Mosaic("reuse-mosaic-1", mosaic_items("edge")), Mosaic("reuse-mosaic-2", mosaic_items("steps", seed=3))],
    "chain": _chain_fold,
    # rows 0, 3 and 5 of the table: destination planes and stats slots shared; full weight, no weight at all, a sigma's table
    "temporal": lambda: [Temporal(f"reuse-temporal-{j + 1}", temporal_items(table, wc, base=base, rows=[0, 3, 5])) for j, (table, wc, base) in enumerate(TEMPORAL_REUSE)],
    "denoise-reach2": lambda: [Denoise("reuse-denoise-1", 1, 0), Denoise("reuse-denoise-2", 1, 1, TC.tables()["random"], 37)],
}


@functools.lru_cache(maxsize=None)
def chain(name):
    return CHAINS[name]()
