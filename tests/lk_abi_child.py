"""ofx_lk_levels on caller-owned buffers: the buffers and the launches of tests/test_gpu_lk_abi.py, and the child process that runs
its accumulating lk_float cases once more in the deep-fetch form.  Not a test module and not a conftest.

    OFX_ITER_DMA=1 python tests/lk_abi_child.py OUT.npz

OFX_ITER_DMA is read once per process, at the first LK launch (csrc/lk_level.hip, lk_switches), so the deep form of the iteration
kernels is reached at these small shapes only by a process STARTED with it (tests/deep_child.py has the same reason).  The child
refuses to start otherwise, runs run_iter_cases on the GPU, stores every array under a readable key in OUT.npz and prints
"lk abi ok".  It compares nothing: the parent does, on the CPU.  The oracle is called for the INPUTS only (the old flow and the warped
next plane an iteration reads).  The first exception ends it with a non-zero status.

Buffer discipline (tests/test_gpu_interp.py: Plane, Field, Guarded): every input lies inside one larger allocation with at least
256 bytes before it and max(256, 2 * pitch) after it, all of it -- the pad columns too -- holding the run's surroundings; every
output is a window of a buffer of 0x5A."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import lk_abi_cases as K   # noqa: E402

F32 = np.float32
FILL = 0x5A
RUNS = (0, 1, 2)           # the three surroundings (test_gpu_interp.AROUND_P / AROUND_F)


def key(*parts):
    return "/".join(str(p) for p in parts)


# ---- buffers --------------------------------------------------------------------------------------------------------------------

def in_plane(arr, g, run):
    """an input plane [rows, w] at the geometry g, its surroundings and pad columns holding the run's byte"""
    from test_gpu_interp import AROUND_P, Plane

    pitch = K.pitch_of(g.pitch, arr.shape[1])
    return Plane(np.ascontiguousarray(arr), pitch, K.FRONT + g.lead, AROUND_P[run], trail=max(256, 2 * pitch))


def in_floats(values, run, lead=2):
    """a few floats (a shift vector) inside a larger buffer of the run's bit pattern; lead in floats behind 256 bytes"""
    from test_gpu_interp import AROUND_F, Field

    return Field(np.asarray(values, F32).reshape(1, -1, 2), 64 + lead, AROUND_F[run])


def in_field(arr, run, lead):
    from test_gpu_interp import AROUND_F, Field

    return Field(arr, 64 + lead, AROUND_F[run])


def out_flow(rows, w, flow_lead):
    from test_gpu_interp import Guarded

    return Guarded(np.float32, 1, rows, 2 * w, 2 * w, 64 + flow_lead)


def out_plane(rows, pitch, lead):
    """an output plane, pad columns included in what host() returns"""
    from test_gpu_interp import Guarded

    return Guarded(np.uint8, 1, rows, pitch, pitch, K.FRONT + lead)


def out_words(dtype, n, lead=64):
    from test_gpu_interp import Guarded

    return Guarded(dtype, 1, 1, n, n, lead)


def put(g, arr, row=0):
    """writes arr [r, items] into rows row .. row + r of slot 0 of a Guarded buffer"""
    import torch

    arr = np.ascontiguousarray(arr, g.dtype)
    raw = g.flat.cpu().numpy()
    view = np.lib.stride_tricks.as_strided(raw.view(g.dtype)[g.lead:], (g.rows, g.w), (g.pitch * g.size, g.size))
    view[row:row + arr.shape[0], :arr.shape[1]] = arr
    g.flat.copy_(torch.from_numpy(raw))


# ---- one descriptor of an ofx_lk_levels launch ------------------------------------------------------------------------------------

class Item:
    """The buffers of one ofx_lk_desc.  prev / nxt / warp_src: whole-level arrays, of which the planes hold the rows of `rows`
    = (row0, rows held, out_y0, out_y1, flow_row0) (None: the whole level).  old: the flow d_flow holds before the launch (whole
    level; its out rows are written into the buffer, every other row stays 0x5A).  status: the word *d_warp_status holds before
    the launch (None: no status word)."""
    EXTRA = 2   # flow rows behind out_y1, which no launch may touch

    def __init__(self, prev, nxt, g, run, rows=None, uv=None, old=None, accumulate=None, min_det=0.0, warp_src=None, warp_scale=K.ITER_SCALE,
                 status=None, bit=0):
        h, w = prev.shape
        self.w, self.h, self.g = w, h, g
        self.row0, self.nrows, self.y0, self.y1, self.f0 = rows if rows is not None else (0, h, 0, h, 0)
        held = slice(self.row0, self.row0 + self.nrows)
        self.prev, self.next = in_plane(prev[held], g, run), in_plane(nxt[held], g, (run + 1) % 3)
        self.pitch = self.prev.pitch
        self.uv = None if uv is None else in_floats(uv, run, lead=2 if g.flow_lead == 4 else 4)
        self.flow = out_flow(self.y1 - self.f0 + self.EXTRA, w, g.flow_lead)
        self.accumulate = (old is not None) if accumulate is None else accumulate
        if old is not None and self.y1 > self.y0:
            put(self.flow, np.asarray(old, F32)[self.y0:self.y1].reshape(self.y1 - self.y0, 2 * w), self.y0 - self.f0)
        self.min_det = float(min_det)
        self.wsrc = self.wout = self.status = None
        self.warp_scale, self.bit = float(warp_scale), bit
        if warp_src is not None:
            self.wsrc = in_plane(warp_src[held], g, (run + 2) % 3)
            self.wout = out_plane(self.nrows, self.pitch, g.lead)
        if status is not None:
            self.status = out_words(np.int32, 1)
            put(self.status, np.array([[status]], np.int32))

    def desc(self, lib):
        return lib.LkDesc(self.prev.ptr, self.next.ptr, lib.Geom(self.w, self.h, self.pitch, self.row0, self.nrows, self.y0, self.y1), self.flow.ptr,
                          self.f0, None if self.uv is None else self.uv.ptr, int(self.accumulate), self.min_det,
                          None if self.wsrc is None else self.wsrc.ptr, None if self.wout is None else self.wout.ptr, self.warp_scale,
                          None if self.status is None else self.status.ptr, self.bit)

    def result(self):
        """{flow: the out rows [y1 - y0, w, 2]; clean: 1 when every other byte of the flow buffer -- the rows before out_y0 and
        behind out_y1 too -- still holds 0x5A; warp: the whole d_warp_out buffer [rows held, pitch]; warp_clean; status}"""
        got, clean = self.flow.host()
        rows = got[0].view(np.uint32)
        lo, hi = self.y0 - self.f0, self.y1 - self.f0
        outside = np.concatenate([rows[:lo].ravel(), rows[hi:].ravel()])
        out = {"flow": got[0][lo:hi].reshape(hi - lo, self.w, 2).copy(), "clean": np.int64(clean and bool((outside == 0x5A5A5A5A).all()))}
        if self.wout is not None:
            wgot, wclean = self.wout.host()
            out["warp"], out["warp_clean"] = wgot[0].copy(), np.int64(wclean)
        if self.status is not None:
            out["status"] = np.int64(self.status.host()[0][0, 0, 0])
        return out


def launch_lk(eng, items, win, mode):
    lib = eng._lib
    arr = (lib.LkDesc * len(items))(*[it.desc(lib) for it in items])
    eng.check(lib.load().ofx_lk_levels(arr, len(items), win, lib.MODES[mode], eng._stream_ptr()), "ofx_lk_levels")


def results(items):
    import torch

    torch.cuda.synchronize()
    return [it.result() for it in items]


# ---- the accumulating lk_float launches (the buffer march: lk_iter_kernel) ----------------------------------------------------------

def run_iter_cases(eng, orc, out, runs=RUNS):
    """kIterAdd, kIterAddWarp, kIterSetWarp on whole levels and kIterAddWarpRows on the two row windows, both modes, every run: the
    arrays of Item.result under variant/shape/mode/runN/name"""
    for mode in K.ITER_MODES:
        for si, (w, h, win) in enumerate(K.ITER_SHAPES):
            d = K.iter_inputs(orc, w, h, win)
            for vi, variant in enumerate(K.ITER_VARIANTS):
                for run in runs:
                    it = Item(d["prev"], d["fed"], K.geo(si + vi), run, old=d["old"] if variant != "set+warp" else None,
                              warp_src=d["next"] if variant != "add" else None)
                    launch_lk(eng, [it], win, mode)
                    for name, v in results([it])[0].items():
                        out[key(variant, f"{w}x{h}-win{win}", mode, f"run{run}", name)] = v
        for c in (K.ROWS_NO_MISS, K.ROWS_MISS):
            d = K.rows_inputs(orc, c)
            for run in runs:
                whole = Item(d["prev"], d["fed"], K.geo(run), run, old=d["old"], warp_src=d["next"])
                part = Item(d["prev"], d["fed"], K.geo(run + 4), run, rows=c["rows"], old=d["old"], warp_src=d["next"], status=c["preload"], bit=c["bit"])
                launch_lk(eng, [whole], c["win"], mode)
                launch_lk(eng, [part], c["win"], mode)
                for tag, r in zip(("whole", "window"), results([whole, part])):
                    for name, v in r.items():
                        out[key("rows", c["id"], mode, f"run{run}", tag, name)] = v
    return out


def main(argv):
    if len(argv) != 2:
        sys.exit(f"usage: OFX_ITER_DMA=1 python {argv[0]} OUT.npz")
    if os.environ.get("OFX_ITER_DMA") != "1" or "OFX_LK_DMA" in os.environ:
        sys.exit("lk_abi_child: start me with OFX_ITER_DMA=1 and without OFX_LK_DMA (both are read once per process)")
    import torch

    assert torch.cuda.is_available(), "these runs need the MI355X"
    from cuda_optical_flow_2_amd import engine
    import oracle

    oracle.build()
    out = run_iter_cases(engine, oracle.Oracle(), {})
    np.savez(argv[1], **out)
    print("lk abi ok")


if __name__ == "__main__":
    main(sys.argv)
