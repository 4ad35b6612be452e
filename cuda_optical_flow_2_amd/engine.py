"""Host-side mirror of the engine's C ABI (include/ofx.h) for Python callers.

PyTorch is used only as plumbing: device memory (``torch.empty(..., device='cuda')``), streams and, in
``parallel.py``, ``torch.distributed``.  All arithmetic runs in libofx_hip.so; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import numpy as np

from . import lib as _lib
from .lib import Geom, MODES, OfxError, Params, check

_vp = C.c_void_p


def _stream_ptr(stream=None) -> Optional[int]:
    """hipStream_t of a torch stream (None -> torch's current stream)."""
    import torch

    st = stream if stream is not None else torch.cuda.current_stream()
    return st.cuda_stream or None


def pitch_for(w: int) -> int:
    return (w + 63) // 64 * 64


class DeviceView:
    """Zero-copy torch view of a device range owned by the C session (via __cuda_array_interface__)."""

    def __init__(self, ptr: int, shape, typestr: str, strides=None):
        self.__cuda_array_interface__ = {"data": (int(ptr), False), "shape": tuple(shape), "typestr": typestr,
                                         "strides": strides, "version": 2}

    def tensor(self):
        import torch

        return torch.as_tensor(self, device="cuda")


class FrameGroup:
    """Consecutive frames of a stream as one argument block for Session.stream_submit_frames (keeps the tensors alive)."""

    def __init__(self, tensors):
        self.tensors = list(tensors)
        self.n = len(self.tensors)
        assert self.n >= 1 and all(t.is_cuda and t.dtype.itemsize == 1 and t.stride(0) == self.tensors[0].stride(0) for t in self.tensors)
        self.pitch = int(self.tensors[0].stride(0))
        self.ptrs = (_vp * self.n)(*[t.data_ptr() for t in self.tensors])


def suggest_stream_batch(width: int, height: int, levels: int, shard=None, borrow_frames: bool = False, two_stage: bool = False) -> int:
    """Frames per launch (ofx_params.stream_batch) for a throughput-bound stream on MI355X: the largest B in {16, 8, 4} the
    launch can carry (OFX_MAX_LK_ITEMS = 80 (pair, level) items) whose cyclic working set stays inside the 256 MB Infinity
    Cache, else 2.  The working set is what lives between a frame's arrival and its last use, d = 3 ticks later (2 with
    two_stage = ofx_params.stream_two_stage): the session's dB+2 image sets (the whole pyramid, or levels >= 1 only with
    borrow_frames) plus the caller's ring of frames (borrow_frames needs at least dB+1 buffers -- include/ofx.h states the
    lifetime rule: frame f's buffer is read until the launch enqueued by the submit of frame f+dB has run --; the estimate
    assumes the ring bench.py uses, dB+4 rounded up to a multiple of four).  Measured: the fused level
    kernel runs ~25 % slower when its image rows come from HBM instead of that cache -- 4K, copied frames: 2 / 4 frames per
    launch = 222k / 197k Mpix/s; borrowed frames in three stages: 4 / 8 = 251-264k / 219k, in two stages: 8 = 274-280k; 1080p
    takes 16 (8 / 16 frames per launch = 227k-247k / 258k-267k), the ranks of a sharded pair 8 (sixteen measured no better
    there: tools/shard_sim.py)."""
    rows = [(height >> k) if shard is None else (shard.buf[k][1] - shard.buf[k][0]) for k in range(levels)]
    level_bytes = [(width >> k) * rows[k] for k in range(levels)]
    depth = 2 if two_stage else 3   # ticks a frame stays in use (ofx_params.stream_two_stage)
    for b in ((16, 8, 4) if shard is None else (8, 4)):  # (a rank of a sharded pair gains nothing from sixteen: measured)
        ring = (depth * max(b, 4) + 4 + 3) // 4 * 4
        working_set = (depth * b + 2) * sum(level_bytes[1 if borrow_frames else 0:]) + ring * level_bytes[0]
        if b * levels <= 80 and working_set <= 230e6:
            return b
    return 2


class Session:
    """Device-resident frame loop (main.cu:192-272): ofx_session_* behind a small object."""

    def __init__(self, width: int, height: int, levels: int, window: int, mode: str = "lk_float", device: int = 0,
                 shard=None, iters: int = 1, local_corner: bool = False, patch_size: int = 0, stream_batch: int = 1, borrow_frames: bool = False,
                 min_det: float = 0.0, two_stage: bool = False, strict: bool = True, frames_partial: bool = False, deep_fetch: int = 0):
        """strict: stream_drain() raises OfxError when the pipeline has drained and the session's status word is not 0 -- a pair
        whose result is NOT the reference's (a corner shift that left the patch of a session that cannot repair it, a shift or
        warp beyond a shard's halo; include/ofx.h, ofx_session_corner_status).  strict=False: poll corner_status() yourself."""
        self.L = _lib.load()
        self.strict = bool(strict)
        self._status = 0
        self.width, self.height, self.levels, self.window, self.mode = width, height, levels, window, mode
        self.device, self._median_scratch = device, None
        p = Params()
        p.width, p.height, p.levels, p.window, p.mode, p.device = width, height, levels, window, MODES[mode], device
        p.iters = iters
        p.local_corner, p.patch_size = int(bool(local_corner)), int(patch_size)
        p.stream_batch = int(stream_batch)
        p.borrow_frames = int(bool(borrow_frames))
        p.min_det = float(min_det)
        p.stream_two_stage = int(bool(two_stage))
        p.frames_partial = int(bool(frames_partial))   # (ofx_params.frames_partial: only the plan's rows + the patch were ever written)
        # ofx_params.deep_fetch: +1 = the frames handed to the stream pipeline are cold (last touched more than an Infinity Cache of
        # traffic ago), -1 = warm, 0 = decide by level size.  Speed only; the bits are the same.
        p.deep_fetch = int(deep_fetch)
        self.shard = shard
        if shard is not None:
            p.sharded = 1
            for k in range(levels):
                p.own_y0[k], p.own_y1[k] = shard.own[k]
                p.buf_y0[k], p.buf_y1[k] = shard.buf[k]
                p.comp_y0[k], p.comp_y1[k] = shard.comp[k]
        self._h = _vp()
        check(self.L.ofx_session_create(C.byref(p), C.byref(self._h)), "ofx_session_create")
        self._keep = []
        self._ring, self._ring_level = None, 0
        self._arrows = self._tracks = self._motion = self._disp = None

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            check(self.L.ofx_session_destroy(self._h), "ofx_session_destroy")
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- frames
    def set_frame_host(self, gray1: np.ndarray, stream=None):
        gray1 = np.ascontiguousarray(gray1, dtype=np.uint8)
        assert gray1.shape == (self.height, self.width), gray1.shape
        self._keep = [gray1]
        check(self.L.ofx_session_set_frame_host(self._h, gray1.ctypes.data, _stream_ptr(stream)), "set_frame_host")

    def set_frame_host_3ch(self, img3: np.ndarray, stream=None):
        img3 = np.ascontiguousarray(img3, dtype=np.uint8)
        assert img3.shape == (self.height, self.width, 3), img3.shape
        self._keep = [img3]
        check(self.L.ofx_session_set_frame_host_3ch(self._h, img3.ctypes.data, _stream_ptr(stream)), "set_frame_host_3ch")

    def set_frame_device(self, t, stream=None):
        """t: torch uint8 CUDA tensor (height, width), row stride = t.stride(0)."""
        assert t.is_cuda and t.dtype.itemsize == 1 and tuple(t.shape) == (self.height, self.width)
        check(self.L.ofx_session_set_frame_device(self._h, t.data_ptr(), int(t.stride(0)), _stream_ptr(stream)),
              "set_frame_device")

    # ---- steps
    def build_pyramid(self, stream=None):
        check(self.L.ofx_session_build_pyramid(self._h, _stream_ptr(stream)), "build_pyramid")

    def downsample_level(self, level: int, stream=None):
        check(self.L.ofx_session_downsample_level(self._h, level, _stream_ptr(stream)), "downsample_level")

    def run_flow(self, stream=None):
        check(self.L.ofx_session_run_flow(self._h, _stream_ptr(stream)), "run_flow")

    def run_flow_dense(self, max_px: Optional[float] = None, stream=None, median: int = 0):
        """ofx_session_run_flow_dense: the pair's dense flow of "coarse-to-fine propagation" in include/ofx.h, in run_flow's place
        -- every level below the top starts from the prolonged flow of the level above instead of one global shift.  max_px: a
        coarse vector longer than this many pixels (of its own level) is dropped; None: the window size, 0: no limit.
        median: 0, or the radius (1: 3x3, 2: 5x5) of the median that filters the flow after the top level and after every
        iteration below it (ofx_session_run_flow_dense_median, "flow median" in include/ofx.h); the session object then keeps a
        second flow pyramid as a torch tensor, made at the first such call."""
        max_px = float(self.window) if max_px is None else float(max_px)
        if not median:
            check(self.L.ofx_session_run_flow_dense(self._h, max_px, _stream_ptr(stream)), "run_flow_dense")
            return
        if self._median_scratch is None:
            import torch

            n = C.c_size_t()
            check(self.L.ofx_session_dense_median_scratch_bytes(self._h, C.byref(n)), "dense_median_scratch_bytes")
            self._median_scratch = torch.empty(n.value // 4, dtype=torch.float32, device=f"cuda:{self.device}")
        t = self._median_scratch
        check(self.L.ofx_session_run_flow_dense_median(self._h, max_px, int(median), t.data_ptr(), t.numel() * 4, _stream_ptr(stream)),
              "run_flow_dense_median")

    def run_flow_sequential(self, stream=None):
        check(self.L.ofx_session_run_flow_sequential(self._h, _stream_ptr(stream)), "run_flow_sequential")

    def corner_flows(self, stream=None):
        check(self.L.ofx_session_corner_flows(self._h, _stream_ptr(stream)), "corner_flows")

    def run_levels(self, stream=None):
        check(self.L.ofx_session_run_levels(self._h, _stream_ptr(stream)), "run_levels")

    def compute_uv(self, level: int, stream=None):
        check(self.L.ofx_session_compute_uv(self._h, level, _stream_ptr(stream)), "compute_uv")

    def run_level(self, level: int, stream=None):
        check(self.L.ofx_session_run_level(self._h, level, _stream_ptr(stream)), "run_level")

    def swap(self):
        check(self.L.ofx_session_swap(self._h), "swap")

    # ---- pipelined pair: staging on the session's aux stream under the previous pair's LK launch
    def submit_device(self, t, stream=None):
        assert t.is_cuda and t.dtype.itemsize == 1 and tuple(t.shape) == (self.height, self.width)
        check(self.L.ofx_session_submit_device(self._h, t.data_ptr(), int(t.stride(0)), _stream_ptr(stream)), "submit_device")

    def stage_frame(self, t, aux=None):
        check(self.L.ofx_session_stage_frame(self._h, t.data_ptr(), int(t.stride(0)), aux), "stage_frame")

    def stage_shift(self, aux=None):
        check(self.L.ofx_session_stage_shift(self._h, aux), "stage_shift")

    def solve_staged(self, stream=None):
        check(self.L.ofx_session_solve_staged(self._h, _stream_ptr(stream)), "solve_staged")

    def aux_stream_ptr(self) -> int:
        p = _vp()
        check(self.L.ofx_session_aux_stream(self._h, C.byref(p)), "aux_stream")
        return p.value

    # ---- stream pipeline: one launch per frame, flow of pair p ready after frame p+3
    def corner_status(self, stream=None) -> int:
        """local_corner sessions: OR of the "shift left the patch at level k" bits since the last call (0 = all exact)."""
        st = C.c_int(0)
        check(self.L.ofx_session_corner_status(self._h, C.byref(st), _stream_ptr(stream)), "corner_status")
        word, self._status = int(st.value) | self._status, 0
        return word

    STATUS_REPAIRED = 1 << 24   # OFX_STATUS_REPAIRED

    def pair_status(self, pair: int, stream=None) -> int:
        """Status word of ONE pair of the stream pipeline (ofx_session_pair_status): the error bits that pair raised, plus
        STATUS_REPAIRED when its shifted corner left the top-left patch and was read through a relocated one (exact all the same)."""
        st = C.c_int(0)
        check(self.L.ofx_session_pair_status(self._h, pair, C.byref(st), _stream_ptr(stream)), "pair_status")
        return int(st.value)

    def stream_begin(self):
        check(self.L.ofx_session_stream_begin(self._h), "stream_begin")

    def stream_submit(self, t, stream=None) -> int:
        assert t.is_cuda and t.dtype.itemsize == 1 and tuple(t.shape) == (self.height, self.width)
        done = C.c_int(-1)
        check(self.L.ofx_session_stream_submit(self._h, t.data_ptr(), int(t.stride(0)), _stream_ptr(stream), C.byref(done)),
              "stream_submit")
        return done.value

    def stream_submit_frames(self, frames, stream=None) -> int:
        """Several consecutive frames in one call (ofx_session_stream_submit_frames): one FFI crossing per group instead of
        one per frame.  `frames`: a sequence of device tensors of equal pitch, or a FrameGroup packed once for a ring that is
        reused.  Returns the highest pair complete after the call, or -1."""
        g = frames if isinstance(frames, FrameGroup) else FrameGroup(frames)
        done = C.c_int(-1)
        check(self.L.ofx_session_stream_submit_frames(self._h, g.ptrs, None, g.pitch, g.n, _stream_ptr(stream), C.byref(done)),
              "stream_submit_frames")
        return done.value

    FRONTEND_MODES = {"off": 0, "grey": 1, "bilateral": 2}   # OFX_FRONTEND_OFF / _GREY / _BILATERAL

    def stream_frontend(self, mode="bilateral", window: int = 9, sigma_s: float = 2.0, sigma_b: float = 10.0, fast: bool = False,
                        first_grey: bool = False):
        """The stream pipeline's colour front end (ofx_session_stream_frontend): every tick's colour frames (stream_submit_3ch)
        are averaged to grey and, with mode "bilateral", filtered (square odd window 3 .. 13, main.cu:240: 9, 2.0, 10.0) by one
        launch that writes the planes the tick reads.  fast: the +-1 LSB filter.  first_grey: frame 0 of every stream is averaged
        only (main.cu:198-209).  mode "off" or None turns it off.  Only before the first frame of a stream."""
        m = self.FRONTEND_MODES["off" if mode is None else mode]
        flags = (1 if fast else 0) | (2 if first_grey else 0)   # OFX_FRONTEND_FLAG_FAST / _FIRST_GREY
        check(self.L.ofx_session_stream_frontend(self._h, m, int(window), float(sigma_s), float(sigma_b), flags), "stream_frontend")

    def _check_3ch(self, t):
        assert t.is_cuda and t.dtype.itemsize == 1 and tuple(t.shape) == (self.height, self.width, 3), "colour frame: uint8 CUDA [H, W, 3]"
        assert t.stride(2) == 1 and t.stride(1) == 3, "colour frame: interleaved channels (stride(2) == 1, stride(1) == 3)"

    def stream_submit_3ch(self, t, stream=None) -> int:
        """stream_submit for a colour frame [H, W, 3] (ofx_session_stream_submit_3ch): the front end must be set.  The tensor is
        read by the front-end launch of the call that launches its tick and must stay unmodified until that launch has run."""
        self._check_3ch(t)
        done = C.c_int(-1)
        check(self.L.ofx_session_stream_submit_3ch(self._h, t.data_ptr(), int(t.stride(0)), _stream_ptr(stream), C.byref(done)),
              "stream_submit_3ch")
        return done.value

    def stream_submit_frames_3ch(self, frames, stream=None) -> int:
        """stream_submit_frames for colour frames (ofx_session_stream_submit_frames_3ch); a FrameGroup of them may be reused."""
        g = frames if isinstance(frames, FrameGroup) else FrameGroup(frames)
        for t in g.tensors:
            self._check_3ch(t)
        done = C.c_int(-1)
        check(self.L.ofx_session_stream_submit_frames_3ch(self._h, g.ptrs, None, g.pitch, g.n, _stream_ptr(stream), C.byref(done)),
              "stream_submit_frames_3ch")
        return done.value

    def stream_drain(self, stream=None) -> int:
        done = C.c_int(-1)
        check(self.L.ofx_session_stream_drain(self._h, _stream_ptr(stream), C.byref(done)), "stream_drain")
        if done.value == -2 and self.strict:
            # the pipeline is empty: every pair it produced must have been the reference's (one synchronising read per drained
            # stream, not per frame).  The word is kept for corner_status() when the caller wants to look at it.
            st = C.c_int(0)
            check(self.L.ofx_session_corner_status(self._h, C.byref(st), _stream_ptr(stream)), "corner_status")
            self._status |= int(st.value)
            if self._status:
                word, self._status = self._status, 0
                raise _lib.OfxError(f"stream pipeline: status word {word:#x} -- bit k: level k's corner shift left the patch and could not be "
                                    "repaired; bit 8+k / 16+k: a shift / warp reached beyond this shard's halo: those pairs are not the "
                                    "reference's result (include/ofx.h, ofx_session_corner_status)")
        return done.value

    def push_frame_host(self, gray1: np.ndarray, stream=None):
        """Load a frame, build its pyramid and make it the previous frame (priming step of main.cu:203-209)."""
        self.set_frame_host(gray1, stream)
        self.build_pyramid(stream)
        self.swap()

    # ---- timing of the level-0 fused kernel (HIP events on the launch stream)
    def timing(self, max_launches: int):
        check(self.L.ofx_session_timing(self._h, max_launches), "session_timing")

    def timing_read(self):
        avg, mn, n = C.c_double(), C.c_double(), C.c_int()
        check(self.L.ofx_session_timing_read(self._h, C.byref(avg), C.byref(mn), C.byref(n)), "session_timing_read")
        return avg.value, mn.value, n.value

    TIME_KINDS = {"lk": 0, "lk_acc": 1, "warp": 2, "stream": 3, "shift": 4, "corner": 5, "pyramid": 6, "lk_acc_warp": 7,
                  "compose": 8}   # OFX_TIME_*

    def timing_read_kind(self, kind: str):
        """(average us, minimum us, launches) of one kind of launch; call before timing_read, which re-arms."""
        avg, mn, n = C.c_double(), C.c_double(), C.c_int()
        check(self.L.ofx_session_timing_read_kind(self._h, self.TIME_KINDS[kind], C.byref(avg), C.byref(mn), C.byref(n)),
              "session_timing_read_kind")
        return avg.value, mn.value, n.value

    # ---- buffers
    def plane(self, which: int, level: int):
        """(torch uint8 view [rows, pitch], Geom) of plane 0=prev 1=next 2=shifted."""
        ptr, g = _vp(), Geom()
        check(self.L.ofx_session_plane(self._h, which, level, C.byref(ptr), C.byref(g)), "session_plane")
        return DeviceView(ptr.value, (g.rows, g.pitch), "|u1").tensor(), g

    def flow(self, level: int):
        """torch float32 view [own_rows, w, 2] of the level's flow, and the global index of its first row."""
        ptr, r0, rows = _vp(), C.c_int(), C.c_int()
        check(self.L.ofx_session_flow(self._h, level, C.byref(ptr), C.byref(r0), C.byref(rows)), "session_flow")
        w = self.width >> level
        return DeviceView(ptr.value, (rows.value, w, 2), "<f4").tensor(), r0.value

    def flow_of(self, pair: int, level: int):
        """As flow(), for one of the newest completed pairs of the stream pipeline (two of them with stream_batch = 2)."""
        ptr, r0, rows = _vp(), C.c_int(), C.c_int()
        check(self.L.ofx_session_flow_of(self._h, pair, level, C.byref(ptr), C.byref(r0), C.byref(rows)), "session_flow_of")
        w = self.width >> level
        return DeviceView(ptr.value, (rows.value, w, 2), "<f4").tensor(), r0.value

    def stream_compose(self, ring, level: int = 0):
        """The stream pipeline's output stage (ofx_session_stream_compose): every pair it completes is composed at `level`
        (main.cu:138-147, the reference's dense field, bit for bit) into slot (p - 1) mod n_slots of `ring`, by one more launch
        per completing call on that call's stream.  ring: float32 CUDA tensor [n_slots, rows, width >> level, 2] (rows = the
        level's own rows), rows tightly packed, the slot stride (stride(0)) free as long as it is 16-byte aligned; n_slots >=
        stream_batch.  None turns it off.  Only before the first frame of a stream; stays in effect for later streams."""
        if ring is None:
            check(self.L.ofx_session_stream_compose(self._h, 0, None, 0, 0), "stream_compose")
            self._ring = None
            return
        import torch

        w = self.width >> level
        rows = (self.height >> level) if self.shard is None else self.shard.own[level][1] - self.shard.own[level][0]
        assert ring.is_cuda and ring.dtype == torch.float32 and ring.dim() == 4, "ring: float32 CUDA tensor [n_slots, rows, w, 2]"
        assert tuple(ring.shape[1:]) == (rows, w, 2), f"ring slots must be [{rows}, {w}, 2], got {tuple(ring.shape[1:])}"
        assert ring.stride()[1:] == (2 * w, 2, 1), "ring: the rows of a slot must be tightly packed"
        check(self.L.ofx_session_stream_compose(self._h, level, ring.data_ptr(), 4 * int(ring.stride(0)), int(ring.shape[0])),
              "stream_compose")
        self._ring = ring
        self._ring_level = level
        self._keep.append(ring)

    def composed_of(self, pair: int):
        """torch float32 view [rows, width >> level, 2] of `pair`'s slot in the ring (ofx_session_composed_of), while it is one
        of the newest n_slots composed pairs; valid once the launch of the call that reported the pair has run."""
        ptr, r0, rows = _vp(), C.c_int(), C.c_int()
        check(self.L.ofx_session_composed_of(self._h, pair, C.byref(ptr), C.byref(r0), C.byref(rows)), "session_composed_of")
        w = self.width >> self._ring_level
        return DeviceView(ptr.value, (rows.value, w, 2), "<f4").tensor()

    def stream_arrows(self, ring, level: int = 0, arrow_res: int = 30):
        """The stream pipeline's sampled output stage, arrows (ofx_session_stream_arrows): the arrow field of main.cu:123-169 of
        every pair it completes -- the composed field at `level` read at the grid points i, j = 0, offset, 2 offset, .. with
        offset = (width >> level) // arrow_res, clamped to +-offset, added to the point and truncated -- into slot (p - 1) mod n_slots
        of `ring`: int32 CUDA tensor [n_slots, ny, nx, 4] of (x0, y0, x1, y1) in the level's pixels, x1 = y1 = -1 for an arrow the
        reference does not draw; (offset, ny, nx) = arrow_grid(width >> level, height >> level, arrow_res).  Slots tightly packed,
        the slot stride free as long as it is a multiple of 16 bytes; n_slots >= stream_batch.  One launch per completing call,
        shared with stream_tracks; no dense ring needed.  None turns it off.  Only before the first frame of a stream."""
        if ring is None:
            check(self.L.ofx_session_stream_arrows(self._h, 0, 1, None, 0, 0), "stream_arrows")
            self._arrows = None
            return
        import torch

        _, ny, nx = arrow_grid(self.width >> level, self.height >> level, arrow_res)
        assert ring.is_cuda and ring.dtype == torch.int32 and ring.dim() == 4, "ring: int32 CUDA tensor [n_slots, ny, nx, 4]"
        assert tuple(ring.shape[1:]) == (ny, nx, 4), f"ring slots must be [{ny}, {nx}, 4], got {tuple(ring.shape[1:])}"
        assert ring.stride()[1:] == (4 * nx, 4, 1), "ring: the arrows of a slot must be tightly packed"
        check(self.L.ofx_session_stream_arrows(self._h, level, arrow_res, ring.data_ptr(), 4 * int(ring.stride(0)), int(ring.shape[0])),
              "stream_arrows")
        self._arrows = ring

    def arrows_of(self, pair: int):
        """torch int32 view [ny, nx, 4] of `pair`'s slot in the arrow ring (ofx_session_arrows_of), while it is one of the newest
        n_slots sampled pairs; valid once the launch of the call that reported the pair has run."""
        ptr, ny, nx = _vp(), C.c_int(), C.c_int()
        check(self.L.ofx_session_arrows_of(self._h, pair, C.byref(ptr), C.byref(ny), C.byref(nx)), "session_arrows_of")
        return DeviceView(ptr.value, (ny.value, nx.value, 4), "<i4").tensor()

    def stream_tracks(self, points, status, history=None, level: int = 0):
        """The stream pipeline's sampled output stage, tracks (ofx_session_stream_tracks): `points` (float32 CUDA [n, 2] of (x, y)
        in the pixels of `level`) are moved through every completed pair in order by the composed flow at the pixel they are in;
        `status` (int32 CUDA [n], 0 = alive) receives the pair at which a point left the level or met a non-finite flow -- such a
        point keeps its position from then on.  After the launch of the call that completes pair p, `points` holds the positions
        in frame p.  history: float32 CUDA [n_slots, n, 2] (slot stride a multiple of 16 bytes, n_slots >= stream_batch), slot
        (p - 1) mod n_slots receives the positions after pair p.  The caller initialises points and status; the result does not
        depend on stream_batch.  points = None turns it off.  Only before the first frame of a stream."""
        if points is None:
            check(self.L.ofx_session_stream_tracks(self._h, 0, None, None, 0, None, 0, 0), "stream_tracks")
            self._tracks = None
            return
        import torch

        n = int(points.shape[0])
        assert points.is_cuda and points.dtype == torch.float32 and tuple(points.shape) == (n, 2) and points.is_contiguous(), "points: float32 CUDA [n, 2]"
        assert status.is_cuda and status.dtype == torch.int32 and tuple(status.shape) == (n,) and status.is_contiguous(), "status: int32 CUDA [n]"
        hp, hs, hn = None, 0, 0
        if history is not None:
            assert history.is_cuda and history.dtype == torch.float32 and history.dim() == 3 and tuple(history.shape[1:]) == (n, 2), \
                f"history: float32 CUDA [n_slots, {n}, 2]"
            assert history.stride()[1:] == (2, 1), "history: the points of a slot must be tightly packed"
            hp, hs, hn = history.data_ptr(), 4 * int(history.stride(0)), int(history.shape[0])
        check(self.L.ofx_session_stream_tracks(self._h, level, points.data_ptr(), status.data_ptr(), n, hp, hs, hn), "stream_tracks")
        self._tracks = (points, status, history)   # (kept alive while the pipeline may write them; replaces the previous ones)

    def stream_motion(self, ring=None, stats=None, level: int = 0, scale: float = None):
        """The stream pipeline's motion-compensation stage (ofx_session_stream_motion; the definition: "motion compensation" in
        include/ofx.h): for every pair it completes, the next image of `level` pulled back onto the previous one by the pair's
        shift and flow -- bit for bit shift_1ch then warp_u8 -- into slot (p - 1) mod n_slots of `ring`, and (w*h, sum |prev - next|,
        sum |prev - mc|, pixels not warped) into slot (p - 1) mod n_slots of `stats`, by one more launch per completing call.
        ring: uint8 CUDA tensor [n_slots, rows, width >> level], unit column stride, row stride a multiple of 4, slot stride a
        multiple of 16 bytes (row padding is left untouched); stats: int64 CUDA tensor [n_slots, 4], contiguous; n_slots >=
        stream_batch.  Either may be None (image only / stats only); both None turns the stage off.  Only before the first frame
        of a stream; stays in effect for later streams."""
        if ring is None and stats is None:
            check(self.L.ofx_session_stream_motion(self._h, 0, 0.0, None, 0, 0, 0, None), "stream_motion")
            self._motion = None
            return
        import torch

        w, rows = self.width >> level, self.height >> level
        n_slots = int((ring if ring is not None else stats).shape[0])
        rp, pitch, stride = None, 0, 0
        if ring is not None:
            assert ring.is_cuda and ring.dtype == torch.uint8 and ring.dim() == 3, "ring: uint8 CUDA tensor [n_slots, rows, w]"
            assert tuple(ring.shape[1:]) == (rows, w) and ring.stride(2) == 1, f"ring slots must be [{rows}, {w}] with unit column stride"
            rp, pitch, stride = ring.data_ptr(), int(ring.stride(1)), int(ring.stride(0))
        sp = None
        if stats is not None:
            assert stats.is_cuda and stats.dtype == torch.int64 and tuple(stats.shape) == (n_slots, 4) and stats.is_contiguous(), \
                f"stats: contiguous int64 CUDA tensor [{n_slots}, 4]"
            sp = stats.data_ptr()
        check(self.L.ofx_session_stream_motion(self._h, level, ITER_SCALE if scale is None else float(scale), rp, pitch, stride, n_slots, sp),
              "stream_motion")
        self._motion = (ring, stats, level)   # (kept alive while the pipeline may write them)

    def motion_of(self, pair: int):
        """(torch uint8 view [rows, width >> level] or None, torch int64 view [4] or None) of `pair`'s slots in the motion stage's
        rings (ofx_session_motion_of), while it is one of the newest n_slots pairs; valid once the launch of the call that
        reported the pair has run."""
        ptr, pitch, st = _vp(), C.c_int(), _vp()
        check(self.L.ofx_session_motion_of(self._h, pair, C.byref(ptr), C.byref(pitch), C.byref(st)), "session_motion_of")
        level = self._motion[2]
        w, rows = self.width >> level, self.height >> level
        img = DeviceView(ptr.value, (rows, pitch.value), "|u1").tensor()[:, :w] if ptr.value else None
        return img, (DeviceView(st.value, (4,), "<i8").tensor() if st.value else None)

    def stream_displacement(self, ring, level: int = 0, scale: float = None):
        """The stream pipeline's displacement stage (ofx_session_stream_displacement; the definition: "pixel displacement" in
        include/ofx.h): for every pair it completes, the motion IN PIXELS the pipeline applied at `level` -- floor(the level's shift)
        + scale * the level's flow -- into slot (p - 1) mod n_slots of `ring`, by one more launch per completing call.  ring:
        float32 CUDA tensor [n_slots, rows, width >> level, 2], rows tightly packed, 16-byte aligned, the slot stride a multiple
        of 16 bytes; n_slots >= stream_batch.  scale: ITER_SCALE when None.  None for ring turns the stage off.  Only before the
        first frame of a stream; stays in effect for later streams."""
        if ring is None:
            check(self.L.ofx_session_stream_displacement(self._h, 0, 0.0, None, 0, 0), "stream_displacement")
            self._disp = None
            return
        import torch

        w, rows = self.width >> level, self.height >> level
        assert ring.is_cuda and ring.dtype == torch.float32 and ring.dim() == 4, "ring: float32 CUDA tensor [n_slots, rows, w, 2]"
        assert tuple(ring.shape[1:]) == (rows, w, 2), f"ring slots must be [{rows}, {w}, 2], got {tuple(ring.shape[1:])}"
        assert ring.stride()[1:] == (2 * w, 2, 1), "ring: the rows of a slot must be tightly packed"
        check(self.L.ofx_session_stream_displacement(self._h, level, ITER_SCALE if scale is None else float(scale), ring.data_ptr(),
                                                     4 * int(ring.stride(0)), int(ring.shape[0])), "stream_displacement")
        self._disp = (ring, level)   # (kept alive while the pipeline may write it)

    def displacement_of(self, pair: int):
        """torch float32 view [rows, width >> level, 2] of `pair`'s slot in the displacement ring (ofx_session_displacement_of),
        while it is one of the newest n_slots pairs; valid once the launch of the call that reported the pair has run."""
        ptr = _vp()
        check(self.L.ofx_session_displacement_of(self._h, pair, C.byref(ptr)), "session_displacement_of")
        level = self._disp[1]
        return DeviceView(ptr.value, (self.height >> level, self.width >> level, 2), "<f4").tensor()

    def uv(self, level: int):
        """Shift vector of `level` for the pair in progress (the slot alternates per pair: query after every swap)."""
        ptr = _vp()
        check(self.L.ofx_session_shift_uv(self._h, level, C.byref(ptr)), "session_shift_uv")
        return DeviceView(ptr.value, (2,), "<f4").tensor()

    def flow_host(self, level: int, stream=None) -> np.ndarray:
        ptr, r0, rows = _vp(), C.c_int(), C.c_int()
        check(self.L.ofx_session_flow(self._h, level, C.byref(ptr), C.byref(r0), C.byref(rows)), "session_flow")
        out = np.empty((rows.value, self.width >> level, 2), np.float32)
        check(self.L.ofx_session_get_flow_host(self._h, level, out.ctypes.data, _stream_ptr(stream)), "get_flow_host")
        return out


# ---- stateless device-pointer calls on torch tensors -------------------------------------------------------------

def _u8_plane(arr: np.ndarray):
    """Upload an (h, w) u8 array into a pitched CUDA tensor; returns (tensor[h, pitch], pitch)."""
    import torch

    h, w = arr.shape
    pitch = pitch_for(w)
    t = torch.zeros((h, pitch), dtype=torch.uint8, device="cuda")
    t[:, :w] = torch.from_numpy(np.ascontiguousarray(arr)).cuda()
    return t, pitch


def lk_level(prev1: np.ndarray, next1: np.ndarray, window: int, mode: str, want_sums: bool = False,
             rows: Optional[Sequence[int]] = None, buf_rows: Optional[Sequence[int]] = None):
    """One fused LK level on host arrays (upload, ofx_lk_level[_sums], download).

    rows=(y0,y1) restricts the produced rows; buf_rows=(r0,r1) uploads only those rows (shard emulation)."""
    import torch

    L = _lib.load()
    h, w = prev1.shape
    r0, r1 = buf_rows if buf_rows is not None else (0, h)
    y0, y1 = rows if rows is not None else (0, h)
    tp, pitch = _u8_plane(prev1[r0:r1])
    tn, _ = _u8_plane(next1[r0:r1])
    g = Geom(w, h, pitch, r0, r1 - r0, y0, y1)
    st = _stream_ptr()
    if want_sums:
        out = torch.zeros((5, y1 - y0, w), dtype=torch.int32, device="cuda")
        check(L.ofx_lk_level_sums(tp.data_ptr(), tn.data_ptr(), C.byref(g), window, MODES[mode], out.data_ptr(), y0, st),
              "ofx_lk_level_sums")
    else:
        out = torch.zeros((y1 - y0, w, 2), dtype=torch.float32, device="cuda")
        check(L.ofx_lk_level(tp.data_ptr(), tn.data_ptr(), C.byref(g), window, MODES[mode], out.data_ptr(), y0, st),
              "ofx_lk_level")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def downsample_1ch(src1: np.ndarray) -> np.ndarray:
    import torch

    L = _lib.load()
    sh, sw = src1.shape
    h, w = sh >> 1, sw >> 1
    ts, sp = _u8_plane(src1)
    dp = pitch_for(w)
    td = torch.zeros((h, dp), dtype=torch.uint8, device="cuda")
    g = Geom.full(w, h, dp)
    check(L.ofx_downsample_1ch(ts.data_ptr(), sp, 0, sh, td.data_ptr(), C.byref(g), _stream_ptr()), "ofx_downsample_1ch")
    torch.cuda.synchronize()
    return td[:, :w].cpu().numpy()


def shift_1ch(src1: np.ndarray, uv) -> np.ndarray:
    import torch

    L = _lib.load()
    h, w = src1.shape
    ts, pitch = _u8_plane(src1)
    td = torch.zeros_like(ts)
    tuv = torch.tensor(list(uv), dtype=torch.float32, device="cuda")
    g = Geom.full(w, h, pitch)
    check(L.ofx_shift_1ch(ts.data_ptr(), td.data_ptr(), C.byref(g), tuv.data_ptr(), _stream_ptr()), "ofx_shift_1ch")
    torch.cuda.synchronize()
    return td[:, :w].cpu().numpy()


def shift_vector(flow_levels: List[Optional[np.ndarray]], level: int, max_level: int) -> np.ndarray:
    import torch

    L = _lib.load()
    keep, ptrs = [], (_vp * _lib.OFX_MAX_LEVELS)()
    for k in range(level + 1, max_level):
        t = torch.from_numpy(np.ascontiguousarray(flow_levels[k], dtype=np.float32)).cuda()
        keep.append(t)
        ptrs[k] = t.data_ptr()
    out = torch.zeros(2, dtype=torch.float32, device="cuda")
    check(L.ofx_shift_vector(ptrs, level, max_level, out.data_ptr(), _stream_ptr()), "ofx_shift_vector")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def compose_flow(flow_levels: List[np.ndarray], levels: int, level: int) -> np.ndarray:
    import torch

    L = _lib.load()
    keep, ptrs = [], (_vp * _lib.OFX_MAX_LEVELS)()
    for k in range(level, levels):
        t = torch.from_numpy(np.ascontiguousarray(flow_levels[k], dtype=np.float32)).cuda()
        keep.append(t)
        ptrs[k] = t.data_ptr()
    h, w, _ = flow_levels[level].shape
    out = torch.zeros((h, w, 2), dtype=torch.float32, device="cuda")
    check(L.ofx_compose_flow(ptrs, w, h, levels, level, out.data_ptr(), _stream_ptr()), "ofx_compose_flow")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def warp_u8(src1: np.ndarray, flow: np.ndarray, scale: float) -> np.ndarray:
    import torch
    from .lib import WarpDesc

    L = _lib.load()
    h, w = src1.shape
    ts, pitch = _u8_plane(src1)
    td = torch.zeros_like(ts)
    tf = torch.from_numpy(np.ascontiguousarray(flow, dtype=np.float32)).cuda()
    d = WarpDesc(ts.data_ptr(), td.data_ptr(), Geom.full(w, h, pitch), tf.data_ptr(), 0, scale, None, 0)
    check(L.ofx_warp_levels(C.byref(d), 1, _stream_ptr()), "ofx_warp_levels")
    torch.cuda.synchronize()
    return td[:, :w].cpu().numpy()


ITER_SCALE = float(np.float32(8.0 / 15.0))   # OFX_ITER_SCALE: the reference's flow units -> pixels


def motion_compensate(prev1: np.ndarray, next1: np.ndarray, flow: np.ndarray, uv=None, scale: float = ITER_SCALE):
    """ofx_motion_compensate on host arrays: (mc uint8 [h, w], stats int64 [4]) of "motion compensation" in include/ofx.h --
    next1 shifted by uv (None: not shifted) and warped by scale * flow, and (w*h, sum |prev1 - next1|, sum |prev1 - mc|, pixels
    not warped)."""
    import torch

    L = _lib.load()
    h, w = prev1.shape
    assert next1.shape == (h, w) and tuple(flow.shape) == (h, w, 2)
    tp, pp = _u8_plane(prev1)
    tn, pn = _u8_plane(next1)
    td = torch.zeros_like(tp)
    tf = torch.from_numpy(np.ascontiguousarray(flow, dtype=np.float32)).cuda()
    tuv = None if uv is None else torch.tensor(list(uv), dtype=torch.float32, device="cuda")
    ts = torch.zeros(4, dtype=torch.int64, device="cuda")
    check(L.ofx_motion_compensate(tp.data_ptr(), pp, tn.data_ptr(), pn, w, h, tf.data_ptr(), None if tuv is None else tuv.data_ptr(),
                                  float(scale), td.data_ptr(), pp, ts.data_ptr(), _stream_ptr()), "ofx_motion_compensate")
    torch.cuda.synchronize()
    return td[:, :w].cpu().numpy(), ts.cpu().numpy()


def flow_pair(prev1: np.ndarray, next1: np.ndarray, levels: int, window: int, mode: str, iters: int = 1, min_det: float = 0.0) -> List[np.ndarray]:
    """Whole pair through a Session: returns the flow pyramid as host arrays."""
    import torch

    h, w = prev1.shape
    s = Session(w, h, levels, window, mode, iters=iters, min_det=min_det)
    try:
        s.push_frame_host(prev1)
        s.set_frame_host(next1)
        s.build_pyramid()
        s.run_flow()
        torch.cuda.synchronize()
        return [s.flow_host(k) for k in range(levels)]
    finally:
        s.close()


def video_flow(frames, levels: int, window: int, mode: str = "lk_float", level: int = 0, iters: int = 1, min_det: float = 0.0,
               batch: Optional[int] = None, out=None, frontend: Optional[str] = None, bilateral=(9, 2.0, 10.0), fast: bool = False):
    """Dense flow of every consecutive pair of a clip, in one call: the field of main.cu:138-147 -- sum over k >= level of
    2^(k-level) * flow_k(y >> (k-level), x >> (k-level)), the reference's only definition of the final result -- composed
    at `level` by the stream pipeline's output stage, bit for bit the reference's (ofx_compose_flow of the pair's flow pyramid).

    frames: uint8 CUDA tensor [N, H, W], N >= 2, unit column stride (rows and frames may be strided).  Returns float32
    [N-1, H >> level, W >> level, 2]: out[p-1] is the flow of frame p-1 -> frame p.  The result tensor itself is the ring the
    pipeline writes (no copies); `out` may supply it (same shape, tightly packed rows, 16-byte aligned slots).  Frames are
    read in place when their pitch and alignment allow it (with iters > 1: a pitch of the width rounded up to 64), otherwise
    through copies.  stream_batch: `batch`, or suggest_stream_batch, at most N-1.  Work is enqueued on the current torch stream;
    the call returns once the pipeline has drained, and raises when a pair is not the reference's result (strict).

    A colour clip, uint8 [N, H, W, 3] with interleaved channels, goes through the pipeline's front end (Session.stream_frontend):
    frontend="main_cu" (the default for colour) is main.cu:198-240 exactly -- frame 0 averaged to grey only, every later frame
    averaged and then bilateral-filtered with `bilateral` = (window, sigma_s, sigma_b), 9x9 (2, 10) as there; "bilateral" filters
    every frame, "grey" filters none.  fast: the +-1 LSB filter.  A grey clip ignores these three."""
    N, H, W = _clip_shape(frames)
    assert 0 <= level < levels
    out = _ring_for(N, H, W, level, frames.device, out)
    _run_clip(frames, levels, window, mode, iters, min_det, batch, frontend, bilateral, fast, lambda s: s.stream_compose(out, level))
    return out


def _clip_shape(frames):
    import torch

    assert frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() in (3, 4), "frames: uint8 CUDA tensor [N, H, W] or [N, H, W, 3]"
    if frames.dim() == 4:
        assert int(frames.shape[3]) == 3, "frames: [N, H, W, 3]"
    N, H, W = (int(v) for v in frames.shape[:3])
    assert N >= 2, "frames: at least two"
    return N, H, W


def _ring_for(N, H, W, level, device, out):
    import torch

    hl, wl = H >> level, W >> level
    stride = (hl * wl * 2 + 3) // 4 * 4   # floats from slot to slot: a multiple of 16 bytes
    if out is None:
        flat = torch.empty((N - 1) * stride, dtype=torch.float32, device=device)
        return flat.as_strided((N - 1, hl, wl, 2), (stride, 2 * wl, 2, 1))
    assert out.dtype == torch.float32 and tuple(out.shape) == (N - 1, hl, wl, 2), f"out must be float32 [{N - 1}, {hl}, {wl}, 2]"
    return out


def _run_clip(frames, levels, window, mode, iters, min_det, batch, frontend, bilateral, fast, attach, order=None):
    """What video_flow, video_arrows and video_tracks share: the clip (grey [N, H, W] or colour [N, H, W, 3]) through the stream
    pipeline, in the configuration video_flow documents; attach(session) sets the output stages before the stream begins.
    order: the frame indices in the order they are submitted (a permutation of range(N); None = range(N)) -- the frames
    themselves are not moved.
    Grey frames are read in place when their pitch and alignment allow it, otherwise through copies.  A colour clip's front end
    writes the session's own planes, so the pipeline always runs in its fast configuration (borrowed planes, two stages)
    whatever the clip's layout; only the colour frames' own alignment matters."""
    import torch

    N, H, W = _clip_shape(frames)
    assert order is None or sorted(order) == list(range(N)), "order: every frame index once"
    colour = frames.dim() == 4
    if colour:
        frontend = frontend or "main_cu"
        assert frontend in ("main_cu", "bilateral", "grey"), f"frontend: 'main_cu', 'bilateral' or 'grey', not {frontend!r}"
        ptr, fstride, pitch = frames.data_ptr(), int(frames.stride(0)), int(frames.stride(1))
        if not (frames.stride(3) == 1 and frames.stride(2) == 3 and ptr % 4 == 0 and fstride % 4 == 0 and pitch >= 3 * W):
            # (every frame's base 4-byte aligned: rows padded to a multiple of four bytes)
            padded = torch.empty((N, H, 3 * W + (-3 * W) % 4), dtype=torch.uint8, device=frames.device)
            padded[:, :, :3 * W] = frames.reshape(N, H, 3 * W)
            frames = padded[:, :, :3 * W].unflatten(2, (W, 3))
        borrow = True
    else:
        assert frames.stride(2) == 1, "frames: unit column stride"
        pitch, fstride, ptr = int(frames.stride(1)), int(frames.stride(0)), frames.data_ptr()
        aligned = pitch % 4 == 0 and fstride % 4 == 0 and ptr % 4 == 0 and pitch >= W
        # (the kernels read a borrowed frame's rows in 4-byte groups: the last row's pitch must lie inside the tensor's storage)
        st = frames.untyped_storage()
        inside = ptr + (N - 1) * fstride + H * pitch <= st.data_ptr() + st.nbytes()
        if aligned and inside:
            borrow = iters <= 1 or pitch == pitch_for(W)   # (else the session copies every frame into its own planes)
        else:
            padded = torch.empty((N, H, pitch_for(W)), dtype=torch.uint8, device=frames.device)
            padded[:, :, :W] = frames
            frames, borrow = padded[:, :, :W], True
    B = batch if batch is not None else suggest_stream_batch(W, H, levels, borrow_frames=borrow, two_stage=borrow)
    B = max(1, min(int(B), N - 1))
    s = Session(W, H, levels, window, mode, iters=iters, min_det=min_det, stream_batch=B, borrow_frames=borrow, two_stage=borrow,
                strict=True)
    try:
        if colour:
            win, ss, sb = bilateral
            s.stream_frontend("grey" if frontend == "grey" else "bilateral", int(win), float(ss), float(sb), fast=fast,
                              first_grey=frontend == "main_cu")
        attach(s)
        s.stream_begin()
        submit = s.stream_submit_3ch if colour else s.stream_submit
        for i in (range(N) if order is None else order):
            submit(frames[i])
        while s.stream_drain() != -2:
            pass
    finally:
        s.close()


def arrow_grid(w: int, h: int, arrow_res: int):
    """(offset, ny, nx) of the arrow field of a w x h level (main.cu:125-131): grid step offset = w // arrow_res, arrows at
    i = 0, offset, .. < h and j = 0, offset, .. < w."""
    assert w > 0 and h > 0 and arrow_res >= 1
    offset = w // arrow_res
    assert offset >= 1, f"arrow_res {arrow_res} is more than the level's width {w}"
    return offset, -(-h // offset), -(-w // offset)


def video_arrows(frames, levels: int, window: int, mode: str = "lk_float", level: int = 0, arrow_res: int = 30, iters: int = 1,
                 min_det: float = 0.0, batch: Optional[int] = None, out=None, frontend: Optional[str] = None, bilateral=(9, 2.0, 10.0),
                 fast: bool = False):
    """The arrow field the reference program shows (main.cu:123-169) for every consecutive pair of a clip, sampled from the pairs'
    flow pyramids by the pipeline's sampled output stage (Session.stream_arrows) -- no dense field is composed.  frames and the
    other arguments as video_flow.  Returns int32 [N-1, ny, nx, 4]: out[p-1] holds (x0, y0, x1, y1) of pair p's arrows in the
    pixels of `level`, x1 = y1 = -1 for an arrow the reference skips; (offset, ny, nx) = arrow_grid(W >> level, H >> level,
    arrow_res).  `out` may supply the tensor (that shape, contiguous)."""
    import torch

    N, H, W = _clip_shape(frames)
    assert 0 <= level < levels
    _, ny, nx = arrow_grid(W >> level, H >> level, arrow_res)
    if out is None:
        out = torch.empty((N - 1, ny, nx, 4), dtype=torch.int32, device=frames.device)
    else:
        assert out.dtype == torch.int32 and tuple(out.shape) == (N - 1, ny, nx, 4) and out.is_contiguous(), f"out must be int32 [{N - 1}, {ny}, {nx}, 4]"
    _run_clip(frames, levels, window, mode, iters, min_det, batch, frontend, bilateral, fast, lambda s: s.stream_arrows(out, level, arrow_res))
    return out


def video_tracks(frames, points, levels: int, window: int, mode: str = "lk_float", level: int = 0, iters: int = 1, min_det: float = 0.0,
                 batch: Optional[int] = None, frontend: Optional[str] = None, bilateral=(9, 2.0, 10.0), fast: bool = False):
    """Points tracked through a clip by the pipeline's sampled output stage (Session.stream_tracks).  points: float32 [n, 2] of
    (x, y) in the pixels of `level` in frame 0 (CUDA tensor or array; not modified).  Returns (positions float32 [N, n, 2],
    status int32 [n]): positions[0] are the input points, positions[p] the positions in frame p; status is 0 for a point alive
    at the end, else the pair at which it left the level or met a non-finite flow (it keeps its position from then on).  The
    other arguments as video_flow."""
    import torch

    N, H, W = _clip_shape(frames)
    assert 0 <= level < levels
    pts = torch.as_tensor(points, dtype=torch.float32, device=frames.device)
    assert pts.dim() == 2 and pts.shape[1] == 2 and pts.shape[0] >= 1, "points: [n, 2]"
    n = int(pts.shape[0])
    stride = (2 * n + 3) // 4 * 4     # floats from frame to frame: a multiple of 16 bytes
    flat = torch.empty(N * stride, dtype=torch.float32, device=frames.device)
    positions = flat.as_strided((N, n, 2), (stride, 2, 1))
    positions[0] = pts
    state = pts.clone().contiguous()
    status = torch.zeros(n, dtype=torch.int32, device=frames.device)
    _run_clip(frames, levels, window, mode, iters, min_det, batch, frontend, bilateral, fast,
              lambda s: s.stream_tracks(state, status, positions[1:], level))
    return positions, status


def video_motion(frames, levels: int, window: int, mode: str = "lk_float", level: int = 0, iters: int = 1, min_det: float = 0.0,
                 batch: Optional[int] = None, scale: float = ITER_SCALE, frontend: Optional[str] = None, bilateral=(9, 2.0, 10.0),
                 fast: bool = False):
    """Every frame of a clip pulled back onto its predecessor by the pair's flow, and the pair's quality sums, by the pipeline's
    motion-compensation stage (Session.stream_motion).  frames and the other arguments as video_flow.  Returns (uint8
    [N-1, H >> level, W >> level], int64 [N-1, 4]): out[p-1] is frame p of `level` motion-compensated onto frame p-1, stats[p-1] =
    (pixels, sum |prev - next|, sum |prev - mc|, pixels not warped) of pair p."""
    import torch

    N, H, W = _clip_shape(frames)
    assert 0 <= level < levels
    hl, wl = H >> level, W >> level
    pitch = (wl + 3) // 4 * 4
    stride = (hl * pitch + 15) // 16 * 16     # bytes from slot to slot
    flat = torch.zeros((N - 1) * stride, dtype=torch.uint8, device=frames.device)
    ring = flat.as_strided((N - 1, hl, wl), (stride, pitch, 1))
    stats = torch.zeros((N - 1, 4), dtype=torch.int64, device=frames.device)
    _run_clip(frames, levels, window, mode, iters, min_det, batch, frontend, bilateral, fast,
              lambda s: s.stream_motion(ring, stats, level, scale))
    return ring, stats


def _beta(beta_px2: float, scale: float) -> float:
    """beta of "forward-backward consistency" from a floor in pixels^2: beta_px2 / scale^2 in float64, rounded once to float32"""
    return float(np.float32(np.float64(beta_px2) / (np.float64(np.float32(scale)) * np.float64(np.float32(scale)))))


def flow_consistency(fwd: np.ndarray, bwd: np.ndarray, scale: float = ITER_SCALE, alpha: float = 0.01, beta_px2: float = 0.5,
                     want_err: bool = False):
    """ofx_flow_consistency on host arrays [h, w, 2]: the forward-backward check of include/ofx.h ("forward-backward
    consistency") of fwd (frame a -> b) against bwd (frame b -> a).  Returns (mask uint8 [h, w], stats int64 [4]) -- the class of
    every pixel (0 consistent, 1 inconsistent, 2 leaves the frame, 3 undefined) and (w*h, pixels of class 1, 2, 3) -- and, with
    want_err, err float32 [h, w] as well: the squared round-trip error in field units, +Inf for classes 2 and 3.  The
    tolerance is alpha * (|fwd|^2 + |bwd there|^2) + beta_px2 / scale^2."""
    import torch

    L = _lib.load()
    h, w, _ = fwd.shape
    assert tuple(fwd.shape) == (h, w, 2) and tuple(bwd.shape) == (h, w, 2)
    tf = torch.from_numpy(np.array(fwd, dtype=np.float32, order="C")).cuda()    # (a copy: the caller's array may be read-only)
    tb = torch.from_numpy(np.array(bwd, dtype=np.float32, order="C")).cuda()
    tm = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    ts = torch.zeros(4, dtype=torch.int64, device="cuda")
    te = torch.zeros((h, w), dtype=torch.float32, device="cuda") if want_err else None
    check(L.ofx_flow_consistency(tf.data_ptr(), tb.data_ptr(), w, h, float(scale), float(alpha), _beta(beta_px2, scale), tm.data_ptr(), w,
                                 te.data_ptr() if want_err else None, ts.data_ptr(), _stream_ptr()), "ofx_flow_consistency")
    torch.cuda.synchronize()
    out = (tm.cpu().numpy(), ts.cpu().numpy())
    return out + (te.cpu().numpy(),) if want_err else out


def _slot_ptrs(ring):
    return [ring.data_ptr() + p * int(ring.stride(0)) * ring.element_size() for p in range(int(ring.shape[0]))]


def _consistency_pairs(fwd_ptrs, bwd_ptrs, h, w, device, scale, alpha, beta):
    """ofx_flow_consistency_batch over P pairs of device fields [h, w, 2] given by their addresses (fwd_ptrs[i] against
    bwd_ptrs[i]), up to OFX_STREAM_MAX_BATCH pairs per launch: (mask uint8 [P, h, w], stats int64 [P, 4])."""
    import torch

    L = _lib.load()
    P = len(fwd_ptrs)
    mask = torch.empty((P, h, w), dtype=torch.uint8, device=device)
    stats = torch.empty((P, 4), dtype=torch.int64, device=device)
    mp, sp = _slot_ptrs(mask), _slot_ptrs(stats)
    for p0 in range(0, P, 16):
        n = min(16, P - p0)
        arr = [(_vp * n)(*ptrs[p0:p0 + n]) for ptrs in (fwd_ptrs, bwd_ptrs, mp, sp)]
        check(L.ofx_flow_consistency_batch(arr[0], arr[1], n, w, h, scale, alpha, beta, arr[2], w, None, arr[3], _stream_ptr()),
              "ofx_flow_consistency_batch")
    return mask, stats


def video_consistency(frames, levels: int, window: int, mode: str = "lk_float", level: int = 0, iters: int = 1, min_det: float = 0.0,
                      batch: Optional[int] = None, alpha: float = 0.01, beta_px2: float = 0.5, both: bool = False,
                      return_flows: bool = False, frontend: Optional[str] = None, bilateral=(9, 2.0, 10.0), fast: bool = False):
    """Which pixels of every pair's flow can be trusted: the forward-backward check of include/ofx.h ("forward-backward
    consistency") for every consecutive pair of a clip.  The clip goes through the stream pipeline twice with a compose ring at
    `level` -- once as it is, once in reverse frame order (the frames are not copied) -- and the pairs then go through
    ofx_flow_consistency_batch, up to 16 per launch, straight out of the two rings.  frames and the other arguments as
    video_flow; the tolerance is alpha * (|fwd|^2 + |bwd there|^2) + beta_px2 / OFX_ITER_SCALE^2.

    Returns (mask uint8 [N-1, H >> level, W >> level], stats int64 [N-1, 4]): mask[p] holds the class of every pixel of the flow
    frame p -> frame p+1 (0 consistent, 1 inconsistent, 2 leaves the frame, 3 undefined), stats[p] = (pixels, pixels of class
    1, 2, 3).  both=True appends (mask_b, stats_b), the same for the backward direction (the flow frame p+1 -> frame p checked
    against the forward one: occlusion as seen from frame p+1).  return_flows=True appends the two rings, float32
    [N-1, H >> level, W >> level, 2]: fwd[p] is the flow frame p -> p+1, and bwd, in the REVERSED run's order, holds the flow
    frame p+1 -> p in bwd[N-2-p].

    Memory: the two rings take 2 * (N-1) * h * w * 8 bytes (h, w of `level`) whether they are returned or not.

    A colour clip's default front end here is "bilateral": "main_cu" treats the first frame of a run differently from the
    others, so the reversed run would see other images than the forward one, and it is refused."""
    N, H, W = _clip_shape(frames)
    assert 0 <= level < levels
    if frames.dim() == 4:
        frontend = frontend or "bilateral"
        assert frontend != "main_cu", ("video_consistency: frontend 'main_cu' filters every frame but a run's first, and the reversed run starts "
                                       "at the other end of the clip: use 'bilateral' or 'grey'")
    rings = []
    for order in (None, range(N - 1, -1, -1)):
        ring = _ring_for(N, H, W, level, frames.device, None)
        _run_clip(frames, levels, window, mode, iters, min_det, batch, frontend, bilateral, fast,
                  lambda s, ring=ring: s.stream_compose(ring, level), order=order)
        rings.append(ring)
    fwd, bwd = rings
    beta, hl, wl = _beta(beta_px2, ITER_SCALE), H >> level, W >> level
    fp, bp = _slot_ptrs(fwd), _slot_ptrs(bwd)[::-1]    # the backward field of forward pair p is slot N-2-p of the reversed run's ring
    out = _consistency_pairs(fp, bp, hl, wl, frames.device, ITER_SCALE, float(alpha), beta)
    if both:
        out += _consistency_pairs(bp, fp, hl, wl, frames.device, ITER_SCALE, float(alpha), beta)
    return out + (fwd, bwd) if return_flows else out


# ---- pixel displacement and frame interpolation ---------------------------------------------------------------------------------

INTERP_MAX_TIMES = 8    # OFX_INTERP_MAX_TIMES


def flow_displacement(flow: np.ndarray, uv=None, scale: float = ITER_SCALE) -> np.ndarray:
    """ofx_flow_displacement on a host array [h, w, 2]: D of "pixel displacement" in include/ofx.h -- (floor(uv[0]) + scale * u,
    floor(uv[1]) + scale * v), the motion in pixels the pipeline applies at a level whose shift is uv (None: none) and whose flow
    is `flow`.  (compose_flow is the reference's display quantity, not a displacement.)"""
    import torch

    L = _lib.load()
    h, w, _ = flow.shape
    assert tuple(flow.shape) == (h, w, 2)
    tf = torch.from_numpy(np.array(flow, dtype=np.float32, order="C")).cuda()
    tuv = None if uv is None else torch.tensor([float(uv[0]), float(uv[1])], dtype=torch.float32, device="cuda")
    td = torch.empty_like(tf)
    check(L.ofx_flow_displacement(tf.data_ptr(), w, h, None if tuv is None else tuv.data_ptr(), float(scale), td.data_ptr(), _stream_ptr()),
          "ofx_flow_displacement")
    torch.cuda.synchronize()
    return td.cpu().numpy()


def _times(times):
    t = np.ascontiguousarray(times, dtype=np.float32).reshape(-1)
    assert 1 <= t.size <= INTERP_MAX_TIMES, f"times: 1 to {INTERP_MAX_TIMES} of them"
    return t, t.ctypes.data_as(C.POINTER(C.c_float))


def interpolate_frames(a: np.ndarray, b: np.ndarray, disp_ab: np.ndarray, disp_ba: np.ndarray, times):
    """ofx_interpolate_frames on host arrays: the in-between frames of the pair (a, b) at `times` (each in (0, 1), at most 8) of
    "frame interpolation" in include/ofx.h, from the two displacement fields in pixels, disp_ab (a -> b) and disp_ba (b -> a),
    both [h, w, 2].  Returns (frames uint8 [T, h, w], stats int64 [T, 4]): stats[k] = (w*h, pixels taken from a only, from b
    only, with neither source inside its frame)."""
    import torch

    L = _lib.load()
    h, w = a.shape
    assert b.shape == (h, w) and tuple(disp_ab.shape) == (h, w, 2) and tuple(disp_ba.shape) == (h, w, 2)
    t, tp = _times(times)
    ta, pa = _u8_plane(np.array(a, dtype=np.uint8))    # (copies: the caller's arrays may be read-only)
    tb, pb = _u8_plane(np.array(b, dtype=np.uint8))
    tab = torch.from_numpy(np.array(disp_ab, dtype=np.float32, order="C")).cuda()
    tba = torch.from_numpy(np.array(disp_ba, dtype=np.float32, order="C")).cuda()
    td = torch.zeros((t.size, h, w), dtype=torch.uint8, device="cuda")
    ts = torch.zeros((t.size, 4), dtype=torch.int64, device="cuda")
    check(L.ofx_interpolate_frames(ta.data_ptr(), pa, tb.data_ptr(), pb, w, h, tab.data_ptr(), tba.data_ptr(), tp, int(t.size), td.data_ptr(), w,
                                   h * w, ts.data_ptr(), _stream_ptr()), "ofx_interpolate_frames")
    torch.cuda.synchronize()
    return td.cpu().numpy(), ts.cpu().numpy()


def video_displacement(frames, levels: int, window: int, mode: str = "lk_float", level: int = 0, iters: int = 1, min_det: float = 0.0,
                       batch: Optional[int] = None, frontend: Optional[str] = None, bilateral=(9, 2.0, 10.0), fast: bool = False, out=None):
    """The motion in pixels of every consecutive pair of a clip at `level`: D of "pixel displacement" in include/ofx.h -- the
    level's global shift, floored, plus OFX_ITER_SCALE times the level's flow -- by the pipeline's displacement stage
    (Session.stream_displacement).  This is what the pipeline applied to frame p to match frame p-1; video_flow's composed field is
    the reference's display quantity and is no displacement.  frames and the other arguments as video_flow.  Returns float32
    [N-1, H >> level, W >> level, 2]: out[p-1] is the displacement frame p-1 -> frame p; `out` may supply the tensor."""
    N, H, W = _clip_shape(frames)
    assert 0 <= level < levels
    out = _ring_for(N, H, W, level, frames.device, out)
    _run_clip(frames, levels, window, mode, iters, min_det, batch, frontend, bilateral, fast, lambda s: s.stream_displacement(out, level))
    return out


def video_interpolate(frames, levels: int, window: int, mode: str = "lk_float", factor: int = 2, iters: int = 1, min_det: float = 0.0,
                      batch: Optional[int] = None, return_stats: bool = False, return_displacements: bool = False):
    """Frame-rate up-conversion of a grey clip: the factor - 1 in-between frames of every consecutive pair, at the times
    float32(k / factor), k = 1 .. factor - 1, by "frame interpolation" of include/ofx.h.  The clip goes through the stream pipeline
    twice with a level-0 displacement ring -- once as it is, once in reverse frame order (the frames are not copied) -- and the
    pairs then go through ofx_interpolate_frames_batch, up to 16 per launch, frames read in place and fields straight out of the
    two rings: one launch writes all in-between frames of its pairs.

    frames: uint8 CUDA tensor [N, H, W], N >= 2, unit column stride (a colour clip is refused); factor: 2 .. 9.  Returns uint8
    [N-1, factor-1, H, W]: out[p, k-1] lies between frame p and frame p+1 at time k / factor.  return_stats=True appends int64
    [N-1, factor-1, 4]: (pixels, pixels taken from frame p only, from frame p+1 only, with neither source inside its frame).
    return_displacements=True appends the two rings, float32 [N-1, H, W, 2]: fwd[p] is the displacement frame p -> p+1, and bwd,
    in the REVERSED run's order, holds frame p+1 -> p in bwd[N-2-p].

    Memory: the two rings take 2 * (N-1) * H * W * 8 bytes whether they are returned or not."""
    frames, N, H, W = _interp_clip(frames, factor)
    rings = []
    for order in (None, range(N - 1, -1, -1)):
        ring = _ring_for(N, H, W, 0, frames.device, None)
        _run_clip(frames, levels, window, mode, iters, min_det, batch, None, None, False,
                  lambda s, ring=ring: s.stream_displacement(ring, 0), order=order)
        rings.append(ring)
    return _interpolate_rings(frames, rings[0], rings[1], factor, return_stats, return_displacements)


def _interp_clip(frames, factor):
    """what video_interpolate and video_interpolate_dense require of their clip: (the clip with usable strides, N, H, W)"""
    assert frames.dim() == 3, ("video_interpolate: grey clips only, uint8 [N, H, W] (a colour clip [N, H, W, 3] goes through "
                               "video_interpolate_colour / video_interpolate_colour_dense)")
    N, H, W = _clip_shape(frames)
    assert isinstance(factor, int) and 2 <= factor <= INTERP_MAX_TIMES + 1, f"factor: an integer 2 .. {INTERP_MAX_TIMES + 1}, not {factor!r}"
    assert frames.stride(2) == 1, "frames: unit column stride"
    if frames.stride(1) < W or frames.stride(0) < 0:
        frames = frames.contiguous()
    return frames, N, H, W


def _interpolate_rings(frames, fwd, bwd, factor, return_stats, return_displacements):
    """The in-between frames of every pair of a clip from its two level-0 displacement rings, float32 [N-1, H, W, 2]: fwd[p] is the
    displacement frame p -> p+1, and bwd, in the REVERSED run's order, holds frame p+1 -> p in bwd[N-2-p].  The pairs go through
    ofx_interpolate_frames_batch (a colour clip [N, H, W, 3]: ofx_interpolate_frames_3ch_batch), up to 16 per launch, frames read in
    place and fields straight out of the two rings."""
    import torch

    N, H, W = _clip_shape(frames)
    T = factor - 1
    t, tp = _times([np.float32(k / factor) for k in range(1, factor)])
    L = _lib.load()
    colour = frames.dim() == 4
    row = 3 * W if colour else W    # bytes
    name = "ofx_interpolate_frames_3ch_batch" if colour else "ofx_interpolate_frames_batch"
    out = torch.empty((N - 1, T, H, W) + ((3,) if colour else ()), dtype=torch.uint8, device=frames.device)
    stats = torch.empty((N - 1, T, 4), dtype=torch.int64, device=frames.device) if return_stats else None
    pitch = int(frames.stride(1))
    ap = [frames.data_ptr() + p * int(frames.stride(0)) for p in range(N)]
    fp, bp = _slot_ptrs(fwd), _slot_ptrs(bwd)[::-1]    # the backward field of forward pair p is slot N-2-p of the reversed run's ring
    op, sp = _slot_ptrs(out), _slot_ptrs(stats) if return_stats else []
    for p0 in range(0, N - 1, 16):
        n = min(16, N - 1 - p0)
        ptrs = [(_vp * n)(*v[p0:p0 + n]) for v in (ap, ap[1:], fp, bp, op, sp)]
        pitches = (C.c_int * n)(*([pitch] * n))
        check(getattr(L, name)(ptrs[0], pitches, ptrs[1], pitches, n, W, H, ptrs[2], ptrs[3], tp, T, ptrs[4], row, H * row,
                               ptrs[5] if return_stats else None, _stream_ptr()), name)
    res = (out,)
    if return_stats:
        res += (stats,)
    if return_displacements:
        res += (fwd, bwd)
    return res[0] if len(res) == 1 else res


# ---- coarse-to-fine dense flow ----------------------------------------------------------------------------------------------------

def flow_median(field: np.ndarray, radius: int = 2, src: Optional[np.ndarray] = None, scale: float = ITER_SCALE):
    """ofx_flow_median on host arrays ("flow median" in include/ofx.h): the 3x3 (radius 1) or 5x5 (radius 2) median of a flow
    field float32 [h, w, 2], per component, border replicated, a vector that is not finite read as (0, 0).  With src (uint8
    [h, w]) returns (filtered field, src warped by scale * the filtered field) from the one fused launch."""
    import torch
    from .lib import MedianDesc

    L = _lib.load()
    h, w, two = field.shape
    assert two == 2 and (src is None or src.shape == (h, w))
    tf = torch.from_numpy(np.array(field, dtype=np.float32, order="C")).cuda()    # (copies: the caller's array may be read-only)
    to = torch.zeros_like(tf)
    d = MedianDesc(tf.data_ptr(), to.data_ptr(), w, h, int(radius), float(scale), None, 0, None, 0)
    if src is not None:
        ts, pitch = _u8_plane(src)
        td = torch.zeros_like(ts)
        d.d_src, d.src_pitch, d.d_dst, d.dst_pitch = ts.data_ptr(), pitch, td.data_ptr(), pitch
    check(L.ofx_flow_median(C.byref(d), 1, _stream_ptr()), "ofx_flow_median")
    torch.cuda.synchronize()
    return to.cpu().numpy() if src is None else (to.cpu().numpy(), td[:, :w].cpu().numpy())


def flow_pair_dense(prev1: np.ndarray, next1: np.ndarray, levels: int, window: int, iters: int = 3, min_det: float = 1.0,
                    max_px: Optional[float] = None, mode: str = "lk_float", median: int = 0) -> List[np.ndarray]:
    """Whole pair through a Session's run_flow_dense: the dense flow pyramid as host arrays.  OFX_ITER_SCALE * flow[k] is level
    k's motion in pixels.  median: Session.run_flow_dense's (0: none; 1, 2: the radius of the flow median after every iteration)."""
    import torch

    h, w = prev1.shape
    s = Session(w, h, levels, window, mode, iters=iters, min_det=min_det)
    try:
        s.push_frame_host(prev1)
        s.set_frame_host(next1)
        s.build_pyramid()
        s.run_flow_dense(max_px, median=median)
        torch.cuda.synchronize()
        return [s.flow_host(k) for k in range(levels)]
    finally:
        s.close()


def _dense_ring(frames, order, levels, window, iters, min_det, max_px, level, mode, out, median=0):
    """the displacement at `level` of every consecutive pair of the clip, its frames taken in `order`, pair at a time: set_frame_device /
    build_pyramid / run_flow_dense / ofx_flow_displacement (no global shift) into the pair's slot / swap, all on the current stream"""
    import torch

    N, H, W = _clip_shape(frames)
    assert frames.dim() == 3, "grey clips only, uint8 [N, H, W]"
    assert 0 <= level < levels
    assert frames.stride(2) == 1, "frames: unit column stride"
    if frames.stride(1) < W:
        frames = frames.contiguous()
    out = _ring_for(N, H, W, level, frames.device, out)
    assert out.stride(3) == 1 and out.stride(2) == 2 and out.stride(1) == 2 * (W >> level) and out.data_ptr() % 8 == 0 and (out.stride(0) * 4) % 8 == 0, \
        "out: tightly packed rows, 8-byte aligned slots"
    s = Session(W, H, levels, window, mode, iters=iters, min_det=min_det)
    try:
        L, st = s.L, _stream_ptr()
        s.set_frame_device(frames[order[0]])
        s.build_pyramid()
        s.swap()
        for p in range(1, N):
            s.set_frame_device(frames[order[p]])
            s.build_pyramid()
            s.run_flow_dense(max_px, median=median)
            flow, _ = s.flow(level)
            check(L.ofx_flow_displacement(flow.data_ptr(), W >> level, H >> level, None, ITER_SCALE, out[p - 1].data_ptr(), st), "ofx_flow_displacement")
            s.swap()
        torch.cuda.current_stream().synchronize()   # (the session's buffers go with it)
    finally:
        s.close()
    return out


def video_displacement_dense(frames, levels: int, window: int, iters: int = 3, min_det: float = 1.0, max_px: Optional[float] = None,
                             level: int = 0, out=None, mode: str = "lk_float", median: int = 0):
    """The motion in pixels of every consecutive pair of a grey clip at `level`, by the coarse-to-fine dense flow
    (Session.run_flow_dense; "coarse-to-fine propagation" in include/ofx.h): OFX_ITER_SCALE times the level's flow, every level
    started from the whole flow of the level above.  Unlike video_displacement it follows motions of many pixels per frame and
    several motions in one scene; it runs pair at a time, levels one after the other.  frames: uint8 CUDA tensor [N, H, W], N >= 2,
    unit column stride.  Returns float32 [N-1, H >> level, W >> level, 2]: out[p-1] is the displacement frame p-1 -> frame p; `out`
    may supply the tensor.  mode: "lk_float" or "lk_float_fast".  median: 0, or the radius (1, 2) of the flow median that filters
    every level's flow after every iteration ("flow median" in include/ofx.h): isolated wrong vectors go, motion edges stay."""
    N = _clip_shape(frames)[0]
    return _dense_ring(frames, list(range(N)), levels, window, iters, min_det, max_px, level, mode, out, median)


def video_interpolate_dense(frames, levels: int, window: int, factor: int = 2, iters: int = 3, min_det: float = 1.0,
                            max_px: Optional[float] = None, return_stats: bool = False, return_displacements: bool = False,
                            mode: str = "lk_float", median: int = 0):
    """video_interpolate with the displacements of the coarse-to-fine dense flow: the clip goes through _dense_ring at level 0 as it
    is and in reverse frame order (the frames are not copied), and the two rings then go through ofx_interpolate_frames_batch as
    video_interpolate's do.  Arguments and results as there; median as video_displacement_dense's."""
    frames, N, H, W = _interp_clip(frames, factor)
    fwd = _dense_ring(frames, list(range(N)), levels, window, iters, min_det, max_px, 0, mode, None, median)
    bwd = _dense_ring(frames, list(range(N - 1, -1, -1)), levels, window, iters, min_det, max_px, 0, mode, None, median)
    return _interpolate_rings(frames, fwd, bwd, factor, return_stats, return_displacements)


# ---- colour frame interpolation ---------------------------------------------------------------------------------------------------

def interpolate_frames_colour(a: np.ndarray, b: np.ndarray, disp_ab: np.ndarray, disp_ba: np.ndarray, times):
    """ofx_interpolate_frames_3ch on host arrays: interpolate_frames for a pair of interleaved 3-channel images [h, w, 3] ("colour
    frame interpolation" in include/ofx.h): one geometry per pixel, every channel blended with it.  Returns (frames uint8
    [T, h, w, 3], stats int64 [T, 4]), the stats counted once per pixel."""
    import torch

    L = _lib.load()
    h, w, _ = a.shape
    assert a.shape == (h, w, 3) and b.shape == (h, w, 3) and tuple(disp_ab.shape) == (h, w, 2) and tuple(disp_ba.shape) == (h, w, 2)
    t, tp = _times(times)
    ta = torch.from_numpy(np.array(a, dtype=np.uint8, order="C")).cuda()    # (copies: the caller's arrays may be read-only)
    tb = torch.from_numpy(np.array(b, dtype=np.uint8, order="C")).cuda()
    tab = torch.from_numpy(np.array(disp_ab, dtype=np.float32, order="C")).cuda()
    tba = torch.from_numpy(np.array(disp_ba, dtype=np.float32, order="C")).cuda()
    td = torch.zeros((t.size, h, w, 3), dtype=torch.uint8, device="cuda")
    ts = torch.zeros((t.size, 4), dtype=torch.int64, device="cuda")
    check(L.ofx_interpolate_frames_3ch(ta.data_ptr(), 3 * w, tb.data_ptr(), 3 * w, w, h, tab.data_ptr(), tba.data_ptr(), tp, int(t.size),
                                       td.data_ptr(), 3 * w, h * 3 * w, ts.data_ptr(), _stream_ptr()), "ofx_interpolate_frames_3ch")
    torch.cuda.synchronize()
    return td.cpu().numpy(), ts.cpu().numpy()


def _interp_clip_colour(frames, factor):
    """what video_interpolate_colour and video_interpolate_colour_dense require of their clip: (the clip with usable strides, N, H, W)"""
    import torch

    assert frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 4 and int(frames.shape[3]) == 3, \
        "video_interpolate_colour: colour clips only, uint8 CUDA tensor [N, H, W, 3] (a grey clip goes through video_interpolate)"
    N, H, W = _clip_shape(frames)
    assert isinstance(factor, int) and 2 <= factor <= INTERP_MAX_TIMES + 1, f"factor: an integer 2 .. {INTERP_MAX_TIMES + 1}, not {factor!r}"
    assert frames.stride(3) == 1 and frames.stride(2) == 3, "frames: unit channel stride and a pixel stride of 3"
    if frames.stride(1) < 3 * W or frames.stride(0) < 0:
        frames = frames.contiguous()
    return frames, N, H, W


def video_interpolate_colour(frames, levels: int, window: int, mode: str = "lk_float", factor: int = 2, iters: int = 1, min_det: float = 0.0,
                             batch: Optional[int] = None, frontend: str = "grey", bilateral=(9, 2.0, 10.0), fast: bool = False,
                             return_stats: bool = False, return_displacements: bool = False):
    """video_interpolate for a colour clip: the factor - 1 in-between COLOUR frames of every consecutive pair, by "colour frame
    interpolation" of include/ofx.h.  The clip goes through the stream pipeline twice with a level-0 displacement ring -- as it is
    and in reverse frame order -- its colour front end making the grey images the flow is computed on (frontend: "grey", the
    channel average, or "bilateral", the average then the pre-filter with bilateral = (window, sigma_s, sigma_b), fast as in
    video_flow.  "main_cu" is refused: it treats the first frame submitted differently from the others, so the two runs would
    see different images of frames 0 and N-1).  The colour frames are then read in place, at the tensor's own pitch and
    alignment, by ofx_interpolate_frames_3ch_batch, up to 16 pairs per launch: one launch reads a pair's two fields once and
    writes all three channels of all its in-between frames.

    frames: uint8 CUDA tensor [N, H, W, 3], N >= 2, unit channel stride and a pixel stride of 3; factor: 2 .. 9.  Returns uint8
    [N-1, factor-1, H, W, 3]; return_stats and return_displacements as video_interpolate (the stats count pixels, not bytes)."""
    frames, N, H, W = _interp_clip_colour(frames, factor)
    assert frontend in ("grey", "bilateral"), \
        f"frontend: 'grey' or 'bilateral', not {frontend!r} ('main_cu' filters all frames but the first one submitted: the reversed run would see other images)"
    rings = []
    for order in (None, range(N - 1, -1, -1)):
        ring = _ring_for(N, H, W, 0, frames.device, None)
        _run_clip(frames, levels, window, mode, iters, min_det, batch, frontend, bilateral, fast,
                  lambda s, ring=ring: s.stream_displacement(ring, 0), order=order)
        rings.append(ring)
    return _interpolate_rings(frames, rings[0], rings[1], factor, return_stats, return_displacements)


def _grey_clip(frames):
    """the channel average of a colour clip [N, H, W, 3] on the device (ofx_frontend_1ch in OFX_FRONTEND_GREY mode, 16 frames per
    call) as a grey clip [N, H, W] with rows pitch_for(W) apart"""
    import torch

    N, H, W = _clip_shape(frames)
    L, st = _lib.load(), _stream_ptr()
    src = frames
    if not (src.data_ptr() % 4 == 0 and int(src.stride(0)) % 4 == 0 and src.stride(1) >= 3 * W):
        # (every frame's base 4-byte aligned: rows padded to a multiple of four bytes, as _run_clip does)
        padded = torch.empty((N, H, 3 * W + (-3 * W) % 4), dtype=torch.uint8, device=frames.device)
        padded[:, :, :3 * W] = frames.reshape(N, H, 3 * W)
        src = padded[:, :, :3 * W].unflatten(2, (W, 3))
    pitch = pitch_for(W)
    grey = torch.zeros((N, H, pitch), dtype=torch.uint8, device=frames.device)
    for i0 in range(0, N, 16):
        n = min(16, N - i0)
        srcs = (_vp * n)(*[src[i0 + i].data_ptr() for i in range(n)])
        dsts = (_vp * n)(*[grey[i0 + i].data_ptr() for i in range(n)])
        check(L.ofx_frontend_1ch(srcs, None, int(src.stride(1)), dsts, None, pitch, n, W, H, None, 1, 9, 2.0, 10.0, st), "ofx_frontend_1ch")
    torch.cuda.current_stream().synchronize()   # (a padded copy goes with this call)
    return grey[:, :, :W]


def video_interpolate_colour_dense(frames, levels: int, window: int, factor: int = 2, iters: int = 3, min_det: float = 1.0,
                                   max_px: Optional[float] = None, return_stats: bool = False, return_displacements: bool = False,
                                   mode: str = "lk_float", median: int = 0):
    """video_interpolate_colour with the displacements of the coarse-to-fine dense flow: the clip's channel average, made on the
    device, goes through _dense_ring at level 0 forwards and in reverse frame order, and the two rings and the colour frames (read
    in place) then go through ofx_interpolate_frames_3ch_batch.  Arguments and results as video_interpolate_dense."""
    frames, N, H, W = _interp_clip_colour(frames, factor)
    grey = _grey_clip(frames)
    fwd = _dense_ring(grey, list(range(N)), levels, window, iters, min_det, max_px, 0, mode, None, median)
    bwd = _dense_ring(grey, list(range(N - 1, -1, -1)), levels, window, iters, min_det, max_px, 0, mode, None, median)
    return _interpolate_rings(frames, fwd, bwd, factor, return_stats, return_displacements)


# ---- texture strength and feature selection --------------------------------------------------------------------------------------

def _texture_plane(img):
    """(tensor that owns the plane, pointer, pitch, w, h) of an (h, w) uint8 host array or CUDA tensor; a CUDA tensor is read in
    place when its rows are a multiple of 4 bytes apart and 4-byte aligned, otherwise through a padded copy"""
    import torch

    if isinstance(img, torch.Tensor) and img.is_cuda:
        assert img.dtype == torch.uint8 and img.dim() == 2, "img: uint8 [h, w]"
        h, w = (int(v) for v in img.shape)
        if (img.stride(1) == 1 or w == 1) and img.stride(0) % 4 == 0 and img.stride(0) >= w and img.data_ptr() % 4 == 0:
            return img, img.data_ptr(), int(img.stride(0)), w, h
        t = torch.zeros((h, pitch_for(w)), dtype=torch.uint8, device=img.device)
        t[:, :w] = img
        return t, t.data_ptr(), pitch_for(w), w, h
    arr = np.asarray(img)
    assert arr.dtype == np.uint8 and arr.ndim == 2, "img: uint8 [h, w]"
    t, pitch = _u8_plane(arr)
    return t, t.data_ptr(), pitch, arr.shape[1], arr.shape[0]


def texture_strength(img, window: int):
    """The texture strength of a uint8 plane [h, w] (host array or CUDA tensor) for an odd window 3 .. 23 ("texture strength and
    feature selection" in include/ofx.h): the smaller eigenvalue of the window's structure tensor, float32 [h, w], +0 where the
    window is flat or holds a single edge.  A host array comes back as an array, a CUDA tensor as a CUDA tensor."""
    import torch
    from .lib import TextureDesc

    keep, ptr, pitch, w, h = _texture_plane(img)
    out = torch.empty((h, w), dtype=torch.float32, device=keep.device)
    d = TextureDesc(ptr, pitch, w, h, out.data_ptr(), w, None, None, None, 0, 0, 0.0)
    check(_lib.load().ofx_texture_features(C.byref(d), 1, int(window), _stream_ptr()), "ofx_texture_features")
    if isinstance(img, torch.Tensor):
        return out
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _good_features_device(ptr, pitch, w, h, window, cell, border, min_strength, max_points, device):
    """(points float32 [n, 2], strengths float32 [n]) as CUDA tensors, of a plane on the device"""
    import torch
    from .lib import TextureDesc

    L, st = _lib.load(), _stream_ptr()
    border = window // 2 + 1 if border is None else int(border)
    ncx, ncy = -(-w // cell), -(-h // cell)
    cap = ncx * ncy if max_points is None else max(0, min(int(max_points), ncx * ncy))
    strength = torch.empty((h, w), dtype=torch.float32, device=device)
    cells = torch.empty((ncy, ncx, 2), dtype=torch.int32, device=device)
    cs = torch.empty((ncy, ncx), dtype=torch.float32, device=device)
    points = torch.zeros((max(cap, 1), 2), dtype=torch.float32, device=device)
    count = torch.zeros(1, dtype=torch.int32, device=device)
    d = TextureDesc(ptr, pitch, w, h, strength.data_ptr(), w, cells.data_ptr(), cs.data_ptr(), None, int(cell), border, float(min_strength))
    check(L.ofx_texture_features(C.byref(d), 1, int(window), st), "ofx_texture_features")
    check(L.ofx_compact_features(cells.data_ptr(), ncx * ncy, cap, points.data_ptr(), count.data_ptr(), st), "ofx_compact_features")
    n = int(count.item())
    pts = points[:n]
    # the strengths of the points: the occupied cells' in the same (cell raster) order
    occupied = cs.reshape(-1)[cells.reshape(-1, 2)[:, 0] >= 0]
    return pts, occupied[:n]


def good_features(img, window: int, cell: int = 16, border: Optional[int] = None, min_strength: float = 0.0, max_points: Optional[int] = None):
    """Points worth tracking in a uint8 plane [h, w] (host array or CUDA tensor): per cell of cell x cell pixels the local maximum
    of the texture strength with the largest strength, at least `border` pixels from the image's edge (None: window // 2 + 1, the
    first border at which no candidate's window touches the edge) and stronger than min_strength ("texture strength and feature
    selection" in include/ofx.h; ofx_texture_features, ofx_compact_features).  Returns (points float32 [n, 2] of (x, y) in cell raster
    order, strengths float32 [n]); at most max_points of them (None: all).  A host array gives arrays, a CUDA tensor CUDA tensors."""
    import torch

    keep, ptr, pitch, w, h = _texture_plane(img)
    pts, strengths = _good_features_device(ptr, pitch, w, h, int(window), int(cell), border, min_strength, max_points, keep.device)
    if isinstance(img, torch.Tensor):
        return pts, strengths
    return pts.cpu().numpy(), strengths.cpu().numpy()


def video_tracks_auto(frames, levels: int, window: int, cell: int = 16, level: int = 0, border: Optional[int] = None, min_strength: float = 0.0,
                      max_points: Optional[int] = None, **kw):
    """video_tracks with the points chosen on the device: good_features of frame 0 at `level` -- the level of the pyramid that
    ofx_pyramid_1ch makes of frame 0, which is the plane the session tracks on -- and then video_tracks, unchanged, with these
    points.  frames: a grey clip, uint8 CUDA tensor [N, H, W].  kw: video_tracks' other arguments (mode, iters, min_det, batch).
    Returns (positions float32 [N, n, 2], status int32 [n], strengths float32 [n]); a clip without a single feature is an error."""
    import torch

    N, H, W = _clip_shape(frames)
    assert frames.dim() == 3, "video_tracks_auto: a grey clip [N, H, W] (a colour clip's grey frames live inside the session)"
    assert 0 <= level < levels
    keep, ptr, pitch, w, h = _texture_plane(frames[0])
    if level > 0:
        planes = [None] + [torch.zeros((H >> k, pitch_for(W >> k)), dtype=torch.uint8, device=frames.device) for k in range(1, level + 1)]
        d_levels = (_vp * (level + 1))(None, *[p.data_ptr() for p in planes[1:]])
        pitches = (C.c_int * (level + 1))(0, *[pitch_for(W >> k) for k in range(1, level + 1)])
        check(_lib.load().ofx_pyramid_1ch(ptr, pitch, W, H, d_levels, pitches, level + 1, _stream_ptr()), "ofx_pyramid_1ch")
        keep, ptr, pitch, w, h = planes[level], planes[level].data_ptr(), pitch_for(W >> level), W >> level, H >> level
    pts, strengths = _good_features_device(ptr, pitch, w, h, int(window), int(cell), border, min_strength, max_points, frames.device)
    if pts.shape[0] == 0:
        raise OfxError(f"video_tracks_auto: frame 0 has no feature at level {level} (window {window}, cell {cell}, min_strength {min_strength})")
    positions, status = video_tracks(frames, pts, levels, window, level=level, **kw)
    return positions, status, strengths


# ---- sparse Lucas-Kanade tracking ---------------------------------------------------------------------------------------------------

TRACK_START, TRACK_SINGULAR, TRACK_OUT, TRACK_RESIDUAL, TRACK_FB = 1, 2, 3, 4, 5


class _KltPyramid:
    """The grey pyramid of one frame for ofx_track_points: level 0 the frame itself (read in place when its rows are pitch_for(w)
    apart and 4-byte aligned, otherwise a padded copy), the levels above made by ofx_pyramid_1ch"""

    def __init__(self, img, levels: int):
        import torch

        keep, ptr, pitch, w, h = _texture_plane(img)
        if pitch != pitch_for(w):                       # one pitch per level for every frame of a clip
            t = torch.zeros((h, pitch_for(w)), dtype=torch.uint8, device=keep.device)
            t[:, :w] = keep[:, :w]
            keep, ptr, pitch = t, t.data_ptr(), pitch_for(w)
        self.w, self.h, self.levels = w, h, int(levels)
        assert 1 <= self.levels <= 8 and (w >> (self.levels - 1)) >= 1 and (h >> (self.levels - 1)) >= 1, "levels: 1 .. 8, the coarsest level not empty"
        self.planes = [keep] + [torch.zeros((h >> k, pitch_for(w >> k)), dtype=torch.uint8, device=keep.device) for k in range(1, self.levels)]
        self.ptrs = [ptr] + [p.data_ptr() for p in self.planes[1:]]
        self.pitches = [pitch] + [pitch_for(w >> k) for k in range(1, self.levels)]
        if self.levels > 1:
            d_levels = (_vp * self.levels)(None, *self.ptrs[1:])
            pitches = (C.c_int * self.levels)(*self.pitches)
            check(_lib.load().ofx_pyramid_1ch(ptr, pitch, w, h, d_levels, pitches, self.levels, _stream_ptr()), "ofx_pyramid_1ch")

    def host(self):
        """the levels as arrays [h >> k, w >> k] (tests: what the referee is fed)"""
        return [p[:, :self.w >> k].cpu().numpy() for k, p in enumerate(self.planes)]


def klt_pyramid(img, levels: int) -> _KltPyramid:
    """The pyramid engine.track_points and engine.video_klt track on, of a uint8 plane [h, w] (host array or CUDA tensor)"""
    return _KltPyramid(img, levels)


def _track_params(window, max_iters, eps, min_lambda, max_sad):
    import math
    from .lib import TrackParams

    return TrackParams(int(window), int(max_iters), int(math.floor(float(eps) * 32.0)), int(max_sad), float(min_lambda))


def _track_launch(pyramids, prm, pair0, points, status, history=None, sad=None, stats=None):
    """ofx_track_points on the pyramids of consecutive frames; points [n, 2] float32 and status [n] int32 are CUDA tensors updated in
    place, history [pairs, n, 2] float32, sad [pairs, n] int32 and stats [pairs, 7] int64 contiguous CUDA tensors or None"""
    from .lib import TrackClip

    p0 = pyramids[0]
    assert all(p.w == p0.w and p.h == p0.h and p.levels == p0.levels and p.pitches == p0.pitches for p in pyramids)
    n_frames, levels = len(pyramids), p0.levels
    table = (_vp * (n_frames * levels))(*[p.ptrs[k] for p in pyramids for k in range(levels)])
    pitches = (C.c_int * levels)(*p0.pitches)
    clip = TrackClip(p0.w, p0.h, levels, n_frames, table, pitches)
    assert points.is_contiguous() and status.is_contiguous() and all(t is None or t.is_contiguous() for t in (history, sad, stats))
    ptr = lambda t: None if t is None else t.data_ptr()
    check(_lib.load().ofx_track_points(C.byref(clip), C.byref(prm), int(pair0), points.data_ptr(), status.data_ptr(), int(points.shape[0]),
                                       ptr(history), ptr(sad), ptr(stats), _stream_ptr()), "ofx_track_points")


def track_points(prev, next, points, levels: int, window: int, max_iters: int = 10, eps: float = 1 / 32, min_lambda: float = 0.0, max_sad: int = 0,
                 fb_max: Optional[float] = None):
    """Track points from `prev` to `next` in pixels ("sparse Lucas-Kanade tracking" in include/ofx.h; ofx_track_points): per point
    an iterative, coarse-to-fine Lucas-Kanade on a lattice of 1/32 px over `levels` levels of the pyramids ofx_pyramid_1ch makes of
    the two frames.  prev, next: uint8 [h, w], host arrays or CUDA tensors; points: float32 [n, 2] of (x, y), n >= 1.  eps: an
    iteration whose step is at most this many pixels in both coordinates is the last (in 1/32 px, rounded down); min_lambda: the
    smaller eigenvalue of the window's gradient matrix a level needs; max_sad: the largest residual a tracked point may have (0:
    any).  Returns (positions float32 [n, 2], status int32 [n], sad int32 [n]): status 0 = tracked, otherwise (1 << 8) | reason
    with reason 1 START, 2 SINGULAR, 3 OUT, 4 RESIDUAL, and the point keeps its position; sad is -1 for a lost point.  With fb_max
    the tracked points are tracked back next -> prev as well, and one that gets lost on the way or misses its start (on the
    lattice) by more than fb_max pixels in either coordinate is lost with reason 5 (FB).  Host frames give arrays, CUDA tensors
    CUDA tensors."""
    import math
    import torch

    pa, pb = _KltPyramid(prev, levels), _KltPyramid(next, levels)
    dev = pa.planes[0].device
    start = torch.as_tensor(np.asarray(points, np.float32) if not isinstance(points, torch.Tensor) else points, dtype=torch.float32, device=dev).reshape(-1, 2).contiguous()
    n = int(start.shape[0])
    pos, status = start.clone(), torch.zeros(n, dtype=torch.int32, device=dev)
    sad = torch.empty((1, n), dtype=torch.int32, device=dev)
    prm = _track_params(window, max_iters, eps, min_lambda, max_sad)
    _track_launch([pa, pb], prm, 1, pos, status, None, sad)
    sad = sad[0]
    if fb_max is not None:
        back, bstat = pos.clone(), status.clone()
        _track_launch([pb, pa], prm, 1, back, bstat)
        lim = int(math.floor(32.0 * float(fb_max)))
        q0, q1 = torch.round(start * 32.0).to(torch.int64), torch.round(back * 32.0).to(torch.int64)   # (exact: the lattice)
        miss = (status == 0) & ((bstat != 0) | ((q1 - q0).abs() > lim).any(dim=1))
        pos[miss] = start[miss]
        status[miss] = (1 << 8) | TRACK_FB
        sad[miss] = -1
    if isinstance(prev, torch.Tensor):
        return pos, status, sad
    torch.cuda.synchronize()
    return pos.cpu().numpy(), status.cpu().numpy(), sad.cpu().numpy()


def video_klt(frames, points=None, levels: int = 3, window: int = 9, cell: int = 16, batch: int = 16, max_iters: int = 10, eps: float = 1 / 32,
              min_lambda: float = 0.0, max_sad: int = 0, return_stats: bool = False):
    """Track points through a grey clip in pixels: ofx_track_points over chains of up to `batch` pairs per launch (1 .. 16; the
    result does not depend on it).  frames: uint8 CUDA tensor [N, H, W]; the pyramids are built frame by frame and only those of
    the chain in flight are kept.  points: float32 [n, 2], or None for good_features(frames[0], window, cell).  Pair p (1 .. N - 1)
    goes from frame p - 1 to frame p.  Returns (positions float32 [N, n, 2] -- [0] the seeds, [p] after pair p, a lost point
    staying where it was --, status int32 [n] -- 0 or (pair << 8) | reason --, sad int32 [N - 1, n], -1 where a point was not
    tracked in that pair) and, with return_stats, the int64 [N - 1, 7] counts of include/ofx.h."""
    import torch

    N, H, W = _clip_shape(frames)
    assert frames.dim() == 3, "video_klt: a grey clip [N, H, W]"
    assert 1 <= batch <= 16, "batch: 1 .. 16"
    dev = frames.device
    last = _KltPyramid(frames[0], levels)
    if points is None:
        points, _ = _good_features_device(last.ptrs[0], last.pitches[0], W, H, int(window), int(cell), None, 0.0, None, dev)
        if points.shape[0] == 0:
            raise OfxError(f"video_klt: frame 0 has no feature (window {window}, cell {cell})")
    pts = torch.as_tensor(np.asarray(points, np.float32) if not isinstance(points, torch.Tensor) else points, dtype=torch.float32, device=dev).reshape(-1, 2)
    n = int(pts.shape[0])
    positions = torch.empty((N, n, 2), dtype=torch.float32, device=dev)
    positions[0] = pts
    cur, status = pts.clone().contiguous(), torch.zeros(n, dtype=torch.int32, device=dev)
    sad = torch.empty((N - 1, n), dtype=torch.int32, device=dev)
    stats = torch.empty((N - 1, 7), dtype=torch.int64, device=dev) if return_stats else None
    prm = _track_params(window, max_iters, eps, min_lambda, max_sad)
    for f0 in range(0, N - 1, batch):
        f1 = min(f0 + batch, N - 1)                       # the pairs f0 + 1 .. f1
        chain = [last] + [_KltPyramid(frames[f], levels) for f in range(f0 + 1, f1 + 1)]
        _track_launch(chain, prm, f0 + 1, cur, status, positions[f0 + 1:f1 + 1], sad[f0:f1], None if stats is None else stats[f0:f1])
        last = chain[-1]
    return (positions, status, sad, stats) if return_stats else (positions, status, sad)


# ---- camera motion from point matches -----------------------------------------------------------------------------------------------

MOTION_MODELS = {"translation": 0, "similarity": 1, "affine": 2}      # OFX_MOTION_*
FIT_OK, FIT_FEW, FIT_DEGENERATE = 0, 1, 2


def _fit_params(model, hypotheses, thr, refits, seed):
    import math
    from .lib import FitParams

    assert model in MOTION_MODELS, f"model: one of {sorted(MOTION_MODELS)}"
    return FitParams(MOTION_MODELS[model], int(hypotheses), int(math.floor(float(thr) * 32.0)), int(refits), int(seed) & 0xFFFFFFFF)


def _fit_launch(items, prm, models, info, work, inliers=None, call="ofx_fit_motion"):
    """ofx_fit_motion on items (p, q, status or None, n, pair, w, h) of contiguous CUDA tensors; item i writes models[i] (float64
    [6]), info[i] (int32 [8]) and inliers[i] (uint8 [n], or None) and works in work[i]"""
    from .lib import FitDesc

    ptr = lambda t: None if t is None else t.data_ptr()
    descs = (FitDesc * len(items))()
    for i, (p, q, status, n, pair, w, h) in enumerate(items):
        assert p.is_contiguous() and q.is_contiguous() and (status is None or status.is_contiguous())
        descs[i] = FitDesc(p.data_ptr(), q.data_ptr(), ptr(status), int(n), int(pair), int(w), int(h), models[i].data_ptr(), info[i].data_ptr(),
                           None if inliers is None else ptr(inliers[i]), work[i].data_ptr())
    check(getattr(_lib.load(), call)(descs, len(items), C.byref(prm), _stream_ptr()), call)


def _fit_work(prm, n_items, device, call="ofx_fit_motion_work_bytes"):
    import torch

    nbytes = int(getattr(_lib.load(), call)(C.byref(prm)))
    if nbytes == 0:
        check(1, call)
    return torch.empty((n_items, nbytes // 8), dtype=torch.float64, device=device)


def _fit_pair(p, q, size, status, pair, prm, n_model, launch, work, return_inliers):
    """fit_motion and fit_homography behind their parameters: one item, host or device"""
    import torch

    on_device = isinstance(p, torch.Tensor) and p.is_cuda
    dev = p.device if on_device else torch.device("cuda")
    as_dev = lambda t, dt: torch.as_tensor(np.ascontiguousarray(t) if not isinstance(t, torch.Tensor) else t, device=dev).to(dt).contiguous()
    tp, tq = as_dev(p, torch.float32).reshape(-1, 2), as_dev(q, torch.float32).reshape(-1, 2)
    n = int(tp.shape[0])
    assert tq.shape[0] == n, "p and q: the same number of matches"
    ts = None if status is None else as_dev(status, torch.int32).reshape(-1)
    assert ts is None or ts.shape[0] == n, "status: one per match"
    models = torch.empty((1, n_model), dtype=torch.float64, device=dev)
    info = torch.empty((1, 8), dtype=torch.int32, device=dev)
    mask = torch.empty((1, max(n, 1)), dtype=torch.uint8, device=dev) if return_inliers else None
    launch([(tp, tq, ts, n, pair, size[0], size[1])], prm, models, info, work(prm, 1, dev), mask)
    out = (models[0], info[0]) + ((mask[0, :n],) if return_inliers else ())
    if on_device:
        return out
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def fit_motion(p, q, size, status=None, pair: int = 0, model: str = "similarity", hypotheses: int = 256, thr: float = 1.0, refits: int = 2,
               seed: int = 0, return_inliers: bool = False):
    """The camera motion between two frames from point matches ("camera motion from point matches" in include/ofx.h;
    ofx_fit_motion): a robust "translation", "similarity" or "affine" model by RANSAC over `hypotheses` samples and `refits`
    least-squares refits on the inliers.  p, q: float32 [n, 2] of (x, y) in the first and in the second frame, host arrays or CUDA
    tensors; size: (w, h) of the frames; status: int32 [n] in ofx_track_points' encoding, with which a match counts when it is
    alive through pair number `pair`; thr: the inlier radius in pixels (in 1/32 px, rounded down).  Returns (model float64 [6] =
    (a, b, tx, c, d, ty) with q ~ (a x + b y + tx, c x + d y + ty), info int32 [8]) and, with return_inliers, the uint8 [n] mask.
    Host inputs give arrays, a CUDA tensor p gives CUDA tensors."""
    return _fit_pair(p, q, size, status, pair, _fit_params(model, hypotheses, thr, refits, seed), 6, _fit_launch, _fit_work, return_inliers)


def motion_compose(m2, m1) -> np.ndarray:
    """m2 after m1 on float64 [6] models (ofx_motion_compose)"""
    a, b = np.ascontiguousarray(m2, np.float64).reshape(6), np.ascontiguousarray(m1, np.float64).reshape(6)
    out = np.empty(6, np.float64)
    check(_lib.load().ofx_motion_compose(a.ctypes.data, b.ctypes.data, out.ctypes.data), "ofx_motion_compose")
    return out


def motion_invert(m) -> np.ndarray:
    """the inverse of a float64 [6] model (ofx_motion_invert); a singular or non-finite one is an error"""
    a = np.ascontiguousarray(m, np.float64).reshape(6)
    out = np.empty(6, np.float64)
    check(_lib.load().ofx_motion_invert(a.ctypes.data, out.ctypes.data), "ofx_motion_invert")
    return out


# ---- planar homography from point matches --------------------------------------------------------------------------------------------

MOTION_HOMOGRAPHY = 3                                  # OFX_MOTION_HOMOGRAPHY
CLIP_MOTION_MODELS = dict(MOTION_MODELS, homography=MOTION_HOMOGRAPHY)      # what video_camera_motion and video_stabilize accept
IDENTITY9 = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


def _homography_params(hypotheses, thr, refits, seed):
    import math
    from .lib import FitParams

    return FitParams(MOTION_HOMOGRAPHY, int(hypotheses), int(math.floor(float(thr) * 32.0)), int(refits), int(seed) & 0xFFFFFFFF)


def _homography_launch(items, prm, models, info, work, inliers=None):
    """ofx_fit_homography on _fit_launch's items; item i writes models[i] (float64 [9])"""
    _fit_launch(items, prm, models, info, work, inliers, call="ofx_fit_homography")


def _homography_work(prm, n_items, device):
    return _fit_work(prm, n_items, device, call="ofx_fit_homography_work_bytes")


def fit_homography(p, q, size, status=None, pair: int = 0, hypotheses: int = 256, thr: float = 1.0, refits: int = 2, seed: int = 0,
                   return_inliers: bool = False):
    """The planar homography between two frames from point matches ("planar homography from point matches" in include/ofx.h;
    ofx_fit_homography): RANSAC over `hypotheses` four-point samples and `refits` least-squares refits on the inliers.  The
    arguments are fit_motion's.  Returns (model float64 [9], row-major 3 x 3 with entry 8 = 1 and q ~ ((m0 x + m1 y + m2) / W,
    (m3 x + m4 y + m5) / W), W = m6 x + m7 y + 1, info int32 [8]) and, with return_inliers, the uint8 [n] mask.  Host inputs give
    arrays, a CUDA tensor p gives CUDA tensors."""
    return _fit_pair(p, q, size, status, pair, _homography_params(hypotheses, thr, refits, seed), 9, _homography_launch, _homography_work, return_inliers)


def _homography_call(name, *models):
    ins = [np.ascontiguousarray(m, np.float64).reshape(-1) for m in models]
    out = np.empty(9, np.float64)
    check(getattr(_lib.load(), name)(*[a.ctypes.data for a in ins], out.ctypes.data), name)
    return out


def homography_compose(m2, m1) -> np.ndarray:
    """m2 after m1 on float64 [9] models, the 3 x 3 product, not renormalised (ofx_homography_compose)"""
    return _homography_call("ofx_homography_compose", np.asarray(m2, np.float64).reshape(9), np.asarray(m1, np.float64).reshape(9))


def homography_invert(m) -> np.ndarray:
    """the inverse of a float64 [9] model (ofx_homography_invert); a singular or non-finite one is an error"""
    return _homography_call("ofx_homography_invert", np.asarray(m, np.float64).reshape(9))


def homography_normalize(m) -> np.ndarray:
    """a float64 [9] model divided by its entry 8 (ofx_homography_normalize); an entry 8 that is 0 or not finite is an error"""
    return _homography_call("ofx_homography_normalize", np.asarray(m, np.float64).reshape(9))


def homography_from_affine(m6) -> np.ndarray:
    """(a, b, tx, c, d, ty) as the float64 [9] model (a, b, tx, c, d, ty, 0, 0, 1) (ofx_homography_from_affine)"""
    return _homography_call("ofx_homography_from_affine", np.asarray(m6, np.float64).reshape(6))


def smooth_homography_path(models, radius: int) -> np.ndarray:
    """The moving average of a homography path: models float64 [N, 9]; every row is normalised (homography_normalize), and row f of
    the result is the mean of the normalised rows max(f - radius, 0) .. min(f + radius, N - 1), entry by entry, summed in index
    order and divided once"""
    m = np.ascontiguousarray(models, np.float64).reshape(-1, 9)
    m = np.stack([homography_normalize(r) for r in m]) if m.shape[0] else m
    N, radius = m.shape[0], int(radius)
    assert radius >= 0
    out = np.empty_like(m)
    for f in range(N):
        g0, g1 = max(f - radius, 0), min(f + radius, N - 1)
        for e in range(9):
            s = np.float64(0.0)
            for g in range(g0, g1 + 1):
                s = s + m[g, e]
            out[f, e] = s / np.float64(g1 - g0 + 1)
    return out


def smooth_path(models, radius: int) -> np.ndarray:
    """The moving average of a camera path: models float64 [N, 6]; row f of the result is the mean of rows max(f - radius, 0) ..
    min(f + radius, N - 1), entry by entry, summed in index order and divided once"""
    m = np.ascontiguousarray(models, np.float64).reshape(-1, 6)
    N, radius = m.shape[0], int(radius)
    assert radius >= 0
    out = np.empty_like(m)
    for f in range(N):
        g0, g1 = max(f - radius, 0), min(f + radius, N - 1)
        for e in range(6):
            s = np.float64(0.0)
            for g in range(g0, g1 + 1):
                s = s + m[g, e]
            out[f, e] = s / np.float64(g1 - g0 + 1)
    return out


def video_camera_motion(frames, model: str = "similarity", levels: int = 3, window: int = 9, cell: int = 16, reseed: int = 16, hypotheses: int = 256,
                        thr: float = 1.0, refits: int = 2, seed: int = 0, max_iters: int = 10, eps: float = 1 / 32, min_lambda: float = 0.0,
                        max_sad: int = 0):
    """The camera motion of every pair of a grey clip, on the device: frames uint8 CUDA tensor [N, H, W]; pair p (1 .. N - 1) goes
    from frame p - 1 to frame p.  Per chain of `reseed` pairs (1 .. 16): good_features(window, cell) of the chain's first frame, ONE
    ofx_track_points launch that keeps every pair's positions, then ONE ofx_fit_motion launch whose items read those rows and the
    chain's status array in place; nothing returns to the host between the launches beyond what good_features does.  Returns
    (models float64 [N - 1, 6], info int32 [N - 1, 8]) as CUDA tensors, row p - 1 for pair p; a pair of a chain without a feature
    gets the identity and status FIT_FEW.  model "homography": the fit is ofx_fit_homography and the models are float64 [N - 1, 9]."""
    import torch

    N, H, W = _clip_shape(frames)
    assert frames.dim() == 3, "video_camera_motion: a grey clip [N, H, W]"
    assert 1 <= reseed <= 16, "reseed: 1 .. 16"
    dev = frames.device
    assert model in CLIP_MOTION_MODELS, f"model: one of {sorted(CLIP_MOTION_MODELS)}"
    homography = model == "homography"
    tprm = _track_params(window, max_iters, eps, min_lambda, max_sad)
    prm = _homography_params(hypotheses, thr, refits, seed) if homography else _fit_params(model, hypotheses, thr, refits, seed)
    ident = IDENTITY9 if homography else (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
    launch = _homography_launch if homography else _fit_launch
    models = torch.empty((max(N - 1, 0), len(ident)), dtype=torch.float64, device=dev)
    info = torch.empty((max(N - 1, 0), 8), dtype=torch.int32, device=dev)
    work = (_homography_work if homography else _fit_work)(prm, reseed, dev)
    last = _KltPyramid(frames[0], levels)
    for f0 in range(0, N - 1, reseed):
        f1 = min(f0 + reseed, N - 1)                      # the pairs f0 + 1 .. f1
        pairs = f1 - f0
        chain = [last] + [_KltPyramid(frames[f], levels) for f in range(f0 + 1, f1 + 1)]
        last = chain[-1]
        seeds, _ = _good_features_device(chain[0].ptrs[0], chain[0].pitches[0], W, H, int(window), int(cell), None, 0.0, None, dev)
        n = int(seeds.shape[0])
        if n == 0:
            models[f0:f1] = torch.tensor(ident, dtype=torch.float64, device=dev)
            info[f0:f1] = torch.tensor([FIT_FEW, 0, 0, -1, 0, 0, 0, 0], dtype=torch.int32, device=dev)
            continue
        pos = torch.empty((pairs + 1, n, 2), dtype=torch.float32, device=dev)
        pos[0] = seeds
        cur, status = pos[0].clone(), torch.zeros(n, dtype=torch.int32, device=dev)
        _track_launch(chain, tprm, f0 + 1, cur, status, pos[1:])
        launch([(pos[b], pos[b + 1], status, n, f0 + 1 + b, W, H) for b in range(pairs)], prm, models[f0:f1], info[f0:f1], work)
    return models, info


# ---- affine frame warp and the clip stabiliser --------------------------------------------------------------------------------------

BORDERS = {"constant": 0, "replicate": 1}      # OFX_BORDER_*


def _warp_launch(items, perspective=False):
    """ofx_warp_affine (or, perspective, ofx_warp_perspective) on items (src, dst, model, border, fill, outside): src and dst uint8
    CUDA tensors [h, w] or [h, w, 3] whose pixels are contiguous (rows any distance apart), model six (nine) floats, outside a
    one-element int64 CUDA tensor or None"""
    from .lib import WarpAffineDesc, WarpPerspDesc

    Desc, n_model, name = (WarpPerspDesc, 9, "ofx_warp_perspective") if perspective else (WarpAffineDesc, 6, "ofx_warp_affine")
    descs = (Desc * len(items))()
    for i, (src, dst, model, border, fill, outside) in enumerate(items):
        ch = 3 if src.dim() == 3 else 1
        assert dst.dim() == src.dim() and (ch == 1 or (src.shape[2] == 3 and dst.shape[2] == 3 and src.stride(2) == 1 and dst.stride(2) == 1))
        assert (src.stride(1) == ch or src.shape[1] == 1) and (dst.stride(1) == ch or dst.shape[1] == 1), "pixels must be contiguous"
        descs[i] = Desc(src.data_ptr(), int(src.stride(0)), int(src.shape[1]), int(src.shape[0]), dst.data_ptr(), int(dst.stride(0)),
                        int(dst.shape[1]), int(dst.shape[0]), ch, int(border), int(fill), (C.c_double * n_model)(*[float(v) for v in model]),
                        None if outside is None else outside.data_ptr())
    check(getattr(_lib.load(), name)(descs, len(items), _stream_ptr()), name)


def _warp_affine_launch(items):
    _warp_launch(items)


def _warp_frame(img, model, n_model, out_size, border, fill, return_outside):
    import torch

    assert border in BORDERS, f"border: one of {sorted(BORDERS)}"
    on_device = isinstance(img, torch.Tensor) and img.is_cuda
    src = (img if on_device else torch.from_numpy(np.ascontiguousarray(img)).cuda()).contiguous()
    assert src.dtype == torch.uint8 and (src.dim() == 2 or (src.dim() == 3 and src.shape[2] == 3)), "img: uint8 [H, W] or [H, W, 3]"
    w, h = (int(src.shape[1]), int(src.shape[0])) if out_size is None else (int(out_size[0]), int(out_size[1]))
    dst = torch.empty((h, w) + tuple(src.shape[2:]), dtype=torch.uint8, device=src.device)
    outside = torch.empty(1, dtype=torch.int64, device=src.device) if return_outside else None
    _warp_launch([(src, dst, np.asarray(model, np.float64).reshape(n_model), BORDERS[border], fill, outside)], perspective=n_model == 9)
    if not on_device:
        torch.cuda.synchronize()
        dst = dst.cpu().numpy()
    return (dst, int(outside.item())) if return_outside else dst


def warp_affine(img, model, out_size=None, border: str = "replicate", fill: int = 0, return_outside: bool = False):
    """A frame seen through a parametric motion ("affine frame warp" in include/ofx.h; ofx_warp_affine).  img: uint8 [H, W] or
    [H, W, 3], host array or CUDA tensor; model: float64 [6] = (a, b, tx, c, d, ty), the INVERSE map -- output pixel (x, y) shows the
    source at (a x + b y + tx, c x + d y + ty); out_size: (w, h) of the result (None: the source's); border: "replicate", or
    "constant" with `fill` in every channel of a pixel whose source position is out of range.  Positions are on the 1/32 px lattice
    and the result is the same bits everywhere.  Returns the warped frame and, with return_outside, the number of output pixels out
    of range.  A host array gives an array, a CUDA tensor a CUDA tensor."""
    return _warp_frame(img, model, 6, out_size, border, fill, return_outside)


def warp_perspective(img, model9, out_size=None, border: str = "replicate", fill: int = 0, return_outside: bool = False):
    """A frame seen through a planar homography ("perspective frame warp" in include/ofx.h; ofx_warp_perspective).  The arguments
    and the result are warp_affine's, with model9 float64 [9], row-major 3 x 3, the INVERSE map -- output pixel (x, y) shows the
    source at ((m0 x + m1 y + m2) / W, (m3 x + m4 y + m5) / W), W = m6 x + m7 y + m8.  A pixel with W <= 0 or a position beyond
    2^35 px gets `fill` under either border mode and counts as outside."""
    return _warp_frame(img, model9, 9, out_size, border, fill, return_outside)


def stabilising_maps(models, info, smooth) -> np.ndarray:
    """The inverse maps W_f, float64 [N, 6], that video_stabilize warps frame f with, from the N - 1 pair models and their info rows
    (host arrays):  C_0 = I, C_f = M_f after C_{f-1} with M_f the identity where the pair's status is not FIT_OK;  S_f = the mean of
    C_g over g in [f - smooth, f + smooth] clipped to the clip (smooth_path), or I for smooth None;  W_f = C_f after the inverse of
    S_f."""
    models, info = np.asarray(models, np.float64), np.asarray(info).reshape(-1, 8)
    if models.ndim == 2 and models.shape[1] == 9:
        return _stabilising_homographies(models, info, smooth)
    models = models.reshape(-1, 6)
    ident = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0])
    path = [ident]
    for f in range(models.shape[0]):
        path.append(motion_compose(models[f] if info[f, 0] == FIT_OK else ident, path[-1]))
    path = np.stack(path)
    if smooth is None:
        return path
    smoothed = smooth_path(path, smooth)
    return np.stack([motion_compose(path[f], motion_invert(smoothed[f])) for f in range(path.shape[0])])


def _stabilising_homographies(models, info, smooth) -> np.ndarray:
    """stabilising_maps for float64 [N - 1, 9] pair models, float64 [N, 9]:  C_0 = I, C_f = normalize(M_f after C_{f-1});  S_f from
    smooth_homography_path;  W_f = normalize(C_f after the inverse of S_f)"""
    ident = np.array(IDENTITY9)
    path = [ident]
    for f in range(models.shape[0]):
        path.append(homography_normalize(homography_compose(models[f] if info[f, 0] == FIT_OK else ident, path[-1])))
    path = np.stack(path)
    if smooth is None:
        return path
    smoothed = smooth_homography_path(path, smooth)
    return np.stack([homography_normalize(homography_compose(path[f], homography_invert(smoothed[f]))) for f in range(path.shape[0])])


def video_stabilize(frames, model: str = "similarity", smooth: Optional[int] = 15, border: str = "replicate", fill: int = 0, **motion):
    """A clip with the camera's shake taken out: video_camera_motion (its other arguments in `motion`) on the clip -- for a colour
    clip [N, H, W, 3] on the integer channel average of its frames --, the camera path C_f composed from the pair models, its moving
    average S_f over `smooth` frames on either side, and every frame f warped with the inverse map C_f after the inverse of S_f
    (ofx_warp_affine, up to 16 frames per launch).  smooth None locks the clip to frame 0; smooth 0 returns the clip unchanged.
    model "homography": the pair models are float64 [9], the path is composed, normalised and smoothed entry by entry
    (smooth_homography_path) and the frames go through ofx_warp_perspective.
    frames: uint8 CUDA tensor [N, H, W] or [N, H, W, 3].  Returns (the stabilised clip, models float64 [N - 1, 6] (or [N - 1, 9]), info
    int32 [N - 1, 8], outside int64 [N]: the pixels of each frame whose source position was out of range) as CUDA tensors."""
    import torch

    N, H, W = _clip_shape(frames)
    assert border in BORDERS, f"border: one of {sorted(BORDERS)}"
    assert smooth is None or smooth >= 0
    grey = frames if frames.dim() == 3 else _grey_clip(frames)
    models, info = video_camera_motion(grey, model=model, **motion)
    outside = torch.zeros(N, dtype=torch.int64, device=frames.device)
    if smooth == 0:
        return frames.clone(), models, info, outside
    maps = stabilising_maps(models.cpu().numpy(), info.cpu().numpy(), smooth)
    src = frames.contiguous()
    out = torch.empty_like(src)
    for f0 in range(0, N, 16):
        _warp_launch([(src[f], out[f], maps[f], BORDERS[border], fill, outside[f:f + 1]) for f in range(f0, min(f0 + 16, N))],
                     perspective=maps.shape[1] == 9)
    return out, models, info, outside


# ---- frame mosaic and the filled stabiliser ------------------------------------------------------------------------------------------

MOSAIC_MAX_SOURCES = 9                                 # OFX_MOSAIC_MAX_SOURCES


def _mosaic_launch(items):
    """ofx_warp_mosaic on items (srcs, models, dst, border, fill, which, counts): srcs 1 .. 9 uint8 CUDA tensors [h, w] or [h, w, 3]
    whose pixels are contiguous (rows any distance apart), models nine floats each, dst like a source, which a uint8 CUDA tensor
    [h, w] or None, counts an int64 CUDA tensor of ten entries or None"""
    from .lib import MosaicDesc

    descs = (MosaicDesc * len(items))()
    for i, (srcs, models, dst, border, fill, which, counts) in enumerate(items):
        d = descs[i]
        ch = 3 if dst.dim() == 3 else 1
        assert 1 <= len(srcs) <= MOSAIC_MAX_SOURCES and len(models) == len(srcs), "1 .. 9 sources, a model each"
        for k, (src, model) in enumerate(zip(srcs, models)):
            assert src.dim() == dst.dim() and (ch == 1 or (src.shape[2] == 3 and src.stride(2) == 1)), "sources and destination: the same channels"
            assert src.stride(1) == ch or src.shape[1] == 1, "pixels must be contiguous"
            s = d.source[k]
            s.d_src, s.src_pitch, s.sw, s.sh = src.data_ptr(), int(src.stride(0)), int(src.shape[1]), int(src.shape[0])
            s.model = (C.c_double * 9)(*[float(v) for v in model])
        assert (dst.stride(1) == ch or dst.shape[1] == 1) and (ch == 1 or (dst.shape[2] == 3 and dst.stride(2) == 1)), "pixels must be contiguous"
        d.n_sources, d.d_dst, d.dst_pitch, d.w, d.h = len(srcs), dst.data_ptr(), int(dst.stride(0)), int(dst.shape[1]), int(dst.shape[0])
        d.channels, d.border, d.fill = ch, int(border), int(fill)
        if which is not None:
            assert which.stride(1) == 1 or which.shape[1] == 1
            d.d_which, d.which_pitch = which.data_ptr(), int(which.stride(0))
        if counts is not None:
            assert counts.numel() == MOSAIC_MAX_SOURCES + 1 and counts.is_contiguous()
            d.d_counts = counts.data_ptr()
    check(_lib.load().ofx_warp_mosaic(descs, len(items), _stream_ptr()), "ofx_warp_mosaic")


def warp_mosaic(srcs, models, out_size=None, border: str = "replicate", fill: int = 0, return_which: bool = False, return_counts: bool = False):
    """Several frames seen through a planar homography each, the first that holds a pixel shown there ("frame mosaic" in
    include/ofx.h; ofx_warp_mosaic, one launch).  srcs: a list of 1 .. 9 uint8 images, each [H, W] or [H, W, 3], all host arrays or
    all CUDA tensors, of any sizes, in priority order; models: float64 [S, 9], the INVERSE map of each source as in warp_perspective;
    out_size: (w, h) of the result (None: source 0's); border: "constant" gives `fill` where no source covers a pixel, "replicate"
    what warp_perspective gives for source 0 there.  Returns the frame and, with return_which, the uint8 [h, w] index of the source
    shown at each pixel (255: none) and, with return_counts, int64 [10]: the pixels per source, entry 9 those that no source covers.
    Arrays in give arrays out, CUDA tensors give CUDA tensors.  A seam between two sources is not blended."""
    import torch

    assert border in BORDERS, f"border: one of {sorted(BORDERS)}"
    srcs = list(srcs)
    assert 1 <= len(srcs) <= MOSAIC_MAX_SOURCES, "srcs: 1 .. 9 images"
    on_device = all(isinstance(s, torch.Tensor) and s.is_cuda for s in srcs)
    assert on_device or not any(isinstance(s, torch.Tensor) for s in srcs), "srcs: all host arrays or all CUDA tensors"
    planes = [(s if on_device else torch.from_numpy(np.ascontiguousarray(s)).cuda()).contiguous() for s in srcs]
    for p in planes:
        assert p.dtype == torch.uint8 and p.dim() == planes[0].dim() and (p.dim() == 2 or (p.dim() == 3 and p.shape[2] == 3)), \
            "srcs: uint8 [H, W] or [H, W, 3], all alike"
    models = np.ascontiguousarray(models, np.float64).reshape(len(planes), 9)
    w, h = (int(planes[0].shape[1]), int(planes[0].shape[0])) if out_size is None else (int(out_size[0]), int(out_size[1]))
    dev = planes[0].device
    dst = torch.empty((h, w) + tuple(planes[0].shape[2:]), dtype=torch.uint8, device=dev)
    which = torch.empty((h, w), dtype=torch.uint8, device=dev) if return_which else None
    counts = torch.empty(MOSAIC_MAX_SOURCES + 1, dtype=torch.int64, device=dev) if return_counts else None
    _mosaic_launch([(planes, models, dst, BORDERS[border], fill, which, counts)])
    res = [dst] + ([which] if return_which else []) + ([counts] if return_counts else [])
    if not on_device:
        torch.cuda.synchronize()
        res = [t.cpu().numpy() for t in res]
    return res[0] if len(res) == 1 else tuple(res)


def stabilising_source_maps(models, info, smooth, reach: int):
    """The sources of the filled stabiliser, from the N - 1 pair models and their info rows (host arrays), with C_f and S_f of
    stabilising_maps: (maps float64 [N, 1 + 2 reach, 9], frames int32 [N, 1 + 2 reach]).  Row f lists the source frames in the order
    f, f - 1, f + 1, f - 2, f + 2, .. up to `reach` (0 .. 4) frames away; frames outside the clip are left out, the rest packed to
    the front, and the tail holds -1 and zeros.  The map of source g in output f is normalize(C_g after the inverse of S_f) for
    float64 [9] models (C_g for smooth None) and homography_from_affine(C_g after the inverse of S_f) for float64 [6] models
    (homography_from_affine(C_g) for smooth None); the entry for g = f is stabilising_maps' row f."""
    reach = int(reach)
    assert 0 <= reach <= 4, "reach: 0 .. 4"
    assert smooth is None or smooth >= 0
    models, info = np.asarray(models, np.float64), np.asarray(info).reshape(-1, 8)
    nine = models.ndim == 2 and models.shape[1] == 9
    models = models.reshape(-1, 9 if nine else 6)
    ident = np.array(IDENTITY9 if nine else (1.0, 0.0, 0.0, 0.0, 1.0, 0.0))
    path = [ident]
    for f in range(models.shape[0]):
        m = models[f] if info[f, 0] == FIT_OK else ident
        path.append(homography_normalize(homography_compose(m, path[-1])) if nine else motion_compose(m, path[-1]))
    path = np.stack(path)
    N = path.shape[0]
    back = None
    if smooth is not None:
        smoothed = smooth_homography_path(path, smooth) if nine else smooth_path(path, smooth)
        back = [homography_invert(s) if nine else motion_invert(s) for s in smoothed]
    maps = np.zeros((N, 1 + 2 * reach, 9), np.float64)
    frames = np.full((N, 1 + 2 * reach), -1, np.int32)
    for f in range(N):
        order = [f] + [g for r in range(1, reach + 1) for g in (f - r, f + r)]
        for k, g in enumerate([g for g in order if 0 <= g < N]):
            if nine:
                m = path[g] if back is None else homography_normalize(homography_compose(path[g], back[f]))
            else:
                m = homography_from_affine(path[g] if back is None else motion_compose(path[g], back[f]))
            maps[f, k], frames[f, k] = m, g
    return maps, frames


def video_stabilize_filled(frames, model: str = "similarity", smooth: Optional[int] = 15, reach: int = 2, border: str = "replicate", fill: int = 0,
                           **motion):
    """video_stabilize with the border of every frame filled from its neighbours: frame f is ONE mosaic item (ofx_warp_mosaic, 16
    frames per launch) whose sources are the frames f, f - 1, f + 1, .. up to `reach` (0 .. 4) away, read in place out of the clip,
    each through its map of stabilising_source_maps; a pixel shows the first of them that holds it, and `border` / `fill` act only
    where none does.  The other arguments are video_stabilize's; smooth 0 returns the clip unchanged.
    frames: uint8 CUDA tensor [N, H, W] or [N, H, W, 3].  Returns (the stabilised clip, models, info, outside int64 [N]: the pixels of
    each frame that no source covers, borrowed int64 [N]: the pixels taken from a neighbour) as CUDA tensors.
    For the float64 [6] models the frame's own pixels go through the perspective warp's position rule (float64, rounded to the 1/32 px
    lattice), not ofx_warp_affine's quantised model: they can differ from video_stabilize's by one lattice step, except where nothing
    rounds (whole-pixel motion).  A seam between two sources is not blended."""
    import torch

    N, H, W = _clip_shape(frames)
    assert border in BORDERS, f"border: one of {sorted(BORDERS)}"
    assert smooth is None or smooth >= 0
    assert 0 <= int(reach) <= 4, "reach: 0 .. 4"
    grey = frames if frames.dim() == 3 else _grey_clip(frames)
    models, info = video_camera_motion(grey, model=model, **motion)
    outside = torch.zeros(N, dtype=torch.int64, device=frames.device)
    borrowed = torch.zeros(N, dtype=torch.int64, device=frames.device)
    if smooth == 0:
        return frames.clone(), models, info, outside, borrowed
    maps, index = stabilising_source_maps(models.cpu().numpy(), info.cpu().numpy(), smooth, reach)
    src = frames.contiguous()
    out = torch.empty_like(src)
    counts = torch.empty((N, MOSAIC_MAX_SOURCES + 1), dtype=torch.int64, device=frames.device)
    for f0 in range(0, N, 16):
        items = []
        for f in range(f0, min(f0 + 16, N)):
            S = int((index[f] >= 0).sum())
            items.append(([src[int(g)] for g in index[f, :S]], maps[f, :S], out[f], BORDERS[border], fill, None, counts[f]))
        _mosaic_launch(items)
    if N:
        outside, borrowed = counts[:, MOSAIC_MAX_SOURCES].clone(), counts[:, 1:MOSAIC_MAX_SOURCES].sum(dim=1)
    return out, models, info, outside, borrowed


# ---- temporal noise filter --------------------------------------------------------------------------------------------------------

TEMPORAL_MAX_NEIGHBOURS = 4                            # OFX_TEMPORAL_MAX_NEIGHBOURS


def temporal_weights(sigma: float) -> np.ndarray:
    """The weight table of the temporal noise filter for a noise of standard deviation sigma (grey levels), uint16 [256]:
    w[i] = rint(256 exp(-t^2 / (2 (0.75 sigma)^2))) with t = max(0, i - 1.5 sigma), in float64.  i is the rounded mean absolute
    difference of two 3 x 3 patches: two patches of one scene point differ by about 1.13 sigma on average, so a difference up to
    1.5 sigma counts fully, and the weight is gone about 2 sigma above that."""
    sigma = float(sigma)
    assert np.isfinite(sigma) and sigma > 0.0, "sigma: a positive number"
    t = np.maximum(0.0, np.arange(256, dtype=np.float64) - 1.5 * sigma)
    return np.rint(256.0 * np.exp(-(t * t) / (2.0 * (0.75 * sigma) ** 2))).astype(np.uint16)


def _temporal_params(weights, centre_weight):
    from .lib import TemporalParams

    table = temporal_weights(weights) if np.isscalar(weights) else np.asarray(weights)
    assert table.shape == (256,) and np.all(table >= 0) and np.all(table <= 256), "weights: a sigma, or 256 integers in 0 .. 256"
    prm = TemporalParams()
    prm.weights = (C.c_uint16 * 256)(*[int(v) for v in table])
    prm.centre_weight, prm.reserved = int(centre_weight), 0
    return prm


def _temporal_descs(items):
    """the ofx_temporal_desc array of items (centre, planes, fields, dst, stats): centre, dst and the 1 .. 4 planes uint8 CUDA tensors
    [h, w] or [h, w, 3] whose pixels are contiguous (rows any distance apart), fields float32 CUDA tensors [h, w, 2], tightly packed,
    stats an int64 CUDA tensor of eight entries or None.  It holds addresses only: the tensors must outlive its use."""
    from .lib import TemporalDesc

    descs = (TemporalDesc * len(items))()
    for i, (centre, planes, fields, dst, stats) in enumerate(items):
        d = descs[i]
        ch = 3 if centre.dim() == 3 else 1
        h, w = int(centre.shape[0]), int(centre.shape[1])
        assert 1 <= len(planes) <= TEMPORAL_MAX_NEIGHBOURS and len(fields) == len(planes), "1 .. 4 neighbours, a field each"
        for t in [centre, dst] + list(planes):
            assert t.dim() == centre.dim() and tuple(t.shape) == tuple(centre.shape), "centre, neighbours and destination: one shape"
            assert (t.stride(1) == ch or w == 1) and (ch == 1 or (t.shape[2] == 3 and t.stride(2) == 1)), "pixels must be contiguous"
        for k, (plane, field) in enumerate(zip(planes, fields)):
            assert tuple(field.shape) == (h, w, 2) and field.stride(2) == 1 and (field.stride(1) == 2 or w == 1) and (field.stride(0) == 2 * w or h == 1), \
                "fields: float32 [h, w, 2], tightly packed"
            s = d.neighbour[k]
            s.d_plane, s.pitch, s.pad, s.d_field = plane.data_ptr(), int(plane.stride(0)), 0, field.data_ptr()
        d.n_neighbours, d.w, d.h, d.channels = len(planes), w, h, ch
        d.d_centre, d.centre_pitch, d.d_dst, d.dst_pitch = centre.data_ptr(), int(centre.stride(0)), dst.data_ptr(), int(dst.stride(0))
        if stats is not None:
            assert stats.numel() == 8 and stats.is_contiguous()
            d.d_stats = stats.data_ptr()
    return descs


def _temporal_launch(items, prm):
    """ofx_temporal_filter on the items of _temporal_descs, one launch"""
    check(_lib.load().ofx_temporal_filter(_temporal_descs(items), len(items), C.byref(prm), _stream_ptr()), "ofx_temporal_filter")


def temporal_filter(centre, neighbours, fields, weights, centre_weight: int = 256, return_stats: bool = False):
    """A frame averaged with its motion-compensated neighbours, each weighted per pixel by the patch test ("temporal noise filter"
    in include/ofx.h; ofx_temporal_filter, one launch).  centre: uint8 [H, W] or [H, W, 3]; neighbours: 1 .. 4 images like it;
    fields: float32 [H, W, 2] each, the displacement in pixels centre -> neighbour on the centre's grid; all host arrays or all
    CUDA tensors.  weights: uint16 [256] with entries <= 256, indexed by the rounded mean absolute difference of the 3 x 3 patches,
    or a float sigma for temporal_weights(sigma); centre_weight: 1 .. 256.  Returns the filtered frame and, with return_stats,
    int64 [8]: (pixels, pixels where neighbour 0 / 1 / 2 / 3 is not usable, pixels left as they were for want of any weight, sum of
    |out - centre|, sum of the weights given).  Arrays in give arrays out, CUDA tensors give CUDA tensors.
    A field per neighbour: a neighbour two frames away takes a chained field (displacement_chain, chain_ring; denoise_rings(reach=2)
    does so for a clip).  No recursive filter, no planar colour."""
    import torch

    neighbours, fields = list(neighbours), list(fields)
    assert 1 <= len(neighbours) <= TEMPORAL_MAX_NEIGHBOURS and len(fields) == len(neighbours), "1 .. 4 neighbours, a field each"
    every = [centre] + neighbours + fields
    on_device = all(isinstance(s, torch.Tensor) and s.is_cuda for s in every)
    assert on_device or not any(isinstance(s, torch.Tensor) for s in every), "all host arrays or all CUDA tensors"
    up = lambda s, dt: (s if on_device else torch.from_numpy(np.ascontiguousarray(s, dt)).cuda()).contiguous()
    c = up(centre, np.uint8)
    planes = [up(s, np.uint8) for s in neighbours]
    flds = [up(s, np.float32) for s in fields]
    assert c.dtype == torch.uint8 and (c.dim() == 2 or (c.dim() == 3 and c.shape[2] == 3)), "centre: uint8 [H, W] or [H, W, 3]"
    assert all(p.dtype == torch.uint8 for p in planes) and all(f.dtype == torch.float32 for f in flds)
    dst = torch.empty_like(c)
    stats = torch.empty(8, dtype=torch.int64, device=c.device) if return_stats else None
    _temporal_launch([(c, planes, flds, dst, stats)], _temporal_params(weights, centre_weight))
    res = [dst] + ([stats] if return_stats else [])
    if not on_device:
        torch.cuda.synchronize()
        res = [t.cpu().numpy() for t in res]
    return res[0] if len(res) == 1 else tuple(res)


def _denoise_rings(frames, fwd, bwd, weights, centre_weight, return_stats):
    """Every frame of a clip filtered with its two neighbours from the clip's two level-0 displacement rings in the convention of
    _interpolate_rings: fwd[p] is the displacement frame p -> p+1, and bwd, in the REVERSED run's order, holds frame p+1 -> p in
    bwd[N-2-p].  Frame f takes frame f-1 with bwd[N-1-f] and then frame f+1 with fwd[f]; the first and the last frame have one
    neighbour.  Up to 16 frames per ofx_temporal_filter launch, frames read in place, fields straight out of the rings."""
    import torch

    N, H, W = _clip_shape(frames)
    prm = _temporal_params(weights, centre_weight)
    out = torch.empty(tuple(frames.shape), dtype=torch.uint8, device=frames.device)
    stats = torch.empty((N, 8), dtype=torch.int64, device=frames.device) if return_stats else None
    for f0 in range(0, N, 16):
        items = []
        for f in range(f0, min(f0 + 16, N)):
            near = ([(frames[f - 1], bwd[N - 1 - f])] if f >= 1 else []) + ([(frames[f + 1], fwd[f])] if f + 1 < N else [])
            items.append((frames[f], [p for p, _ in near], [d for _, d in near], out[f], stats[f] if return_stats else None))
        _temporal_launch(items, prm)
    return (out, stats) if return_stats else out


# ---- displacement chain ----------------------------------------------------------------------------------------------------------

CHAIN_MAX_LINKS = 4                                    # OFX_CHAIN_MAX_LINKS


def _chain_launch(items):
    """ofx_displacement_chain on items (link addresses, w, h, dst, mask or None, stats or None), one launch: dst a float32 CUDA
    tensor [h, w, 2], mask uint8 [h, w] with contiguous pixels, stats int64 [4].  It passes addresses: the tensors must outlive it."""
    from .lib import ChainDesc

    descs = (ChainDesc * len(items))()
    for d, (links, w, h, dst, mask, stats) in zip(descs, items):
        assert 2 <= len(links) <= CHAIN_MAX_LINKS, "2 .. 4 links"
        for k, ptr in enumerate(links):
            d.d_link[k] = ptr
        d.n_links, d.w, d.h, d.d_dst = len(links), w, h, dst.data_ptr()
        if mask is not None:
            d.d_mask, d.mask_pitch = mask.data_ptr(), max(int(mask.stride(0)), w)
        if stats is not None:
            d.d_stats = stats.data_ptr()
    check(_lib.load().ofx_displacement_chain(descs, len(items), _stream_ptr()), "ofx_displacement_chain")


def displacement_chain(links, return_mask: bool = False, return_stats: bool = False):
    """The displacement of a frame towards the frame len(links) frames on, from the displacements of the consecutive pairs between
    them ("displacement chain" in include/ofx.h; ofx_displacement_chain, one launch): D_ac(x) = D_ab(x) + D_bc(x + D_ab(x)), folded
    over 2 .. 4 links.  links: float32 [H, W, 2] each, in pixels, link j the displacement of frame j -> frame j + 1 on frame j's
    grid; all host arrays or all CUDA tensors.  Returns the chained field, float32 [H, W, 2] -- where the path leaves the frame or
    is not defined, both components are the NaN 0x7fc00000, which the temporal filter and the frame interpolation treat as not
    defined -- and, with return_mask, uint8 [H, W] (0 ok, 2 leaves the frame, 3 undefined), with return_stats, int64 [4]: (pixels,
    pixels of class 2, of class 3, of class 0).  Arrays in give arrays out, CUDA tensors give CUDA tensors."""
    import torch

    links = list(links)
    assert 2 <= len(links) <= CHAIN_MAX_LINKS, "2 .. 4 links"
    on_device = all(isinstance(s, torch.Tensor) and s.is_cuda for s in links)
    assert on_device or not any(isinstance(s, torch.Tensor) for s in links), "all host arrays or all CUDA tensors"
    # (a copy of a host array: the caller's may be read-only)
    flds = [(s if on_device else torch.from_numpy(np.array(s, dtype=np.float32, order="C")).cuda()).contiguous() for s in links]
    h, w = int(flds[0].shape[0]), int(flds[0].shape[1])
    assert all(f.dtype == torch.float32 and tuple(f.shape) == (h, w, 2) for f in flds), "links: float32 [H, W, 2], one size"
    dst = torch.empty_like(flds[0])
    mask = torch.empty((h, w), dtype=torch.uint8, device=dst.device) if return_mask else None
    stats = torch.empty(4, dtype=torch.int64, device=dst.device) if return_stats else None
    _chain_launch([([f.data_ptr() for f in flds], w, h, dst, mask, stats)])
    res = [dst] + ([mask] if return_mask else []) + ([stats] if return_stats else [])
    if not on_device:
        torch.cuda.synchronize()
        res = [t.cpu().numpy() for t in res]
    return res[0] if len(res) == 1 else tuple(res)


def chain_ring(ring, span: int):
    """The displacements over `span` frames of a ring of consecutive pairs: ring a float32 CUDA tensor [P, H, W, 2], tightly packed,
    ring[p] the displacement of frame p -> p + 1 (a ring of a REVERSED run chains the same way: it is a run of consecutive pairs
    too); span in 2 .. 4 <= P.  Returns [P - span + 1, H, W, 2]: entry p is the chain of ring[p .. p + span - 1], the displacement
    of frame p -> p + span.  Up to 16 entries per ofx_displacement_chain launch, the links read in place out of the ring."""
    import torch

    assert isinstance(ring, torch.Tensor) and ring.is_cuda and ring.dtype == torch.float32 and ring.dim() == 4 and ring.shape[3] == 2 and ring.is_contiguous(), \
        "ring: a float32 CUDA tensor [P, H, W, 2], tightly packed"
    span = int(span)
    P, H, W = int(ring.shape[0]), int(ring.shape[1]), int(ring.shape[2])
    assert 2 <= span <= CHAIN_MAX_LINKS and span <= P, "span: 2 .. 4 and at most the ring's pairs"
    out = torch.empty((P - span + 1, H, W, 2), dtype=torch.float32, device=ring.device)
    slot = _slot_ptrs(ring)
    for p0 in range(0, P - span + 1, 16):
        _chain_launch([(slot[p:p + span], W, H, out[p], None, None) for p in range(p0, min(p0 + 16, P - span + 1))])
    return out


def denoise_rings(frames, fwd, bwd, sigma, reach: int = 1, centre_weight: int = 256, return_stats: bool = False):
    """Every frame of a clip filtered with its neighbours up to `reach` frames away, from the clip's two level-0 displacement rings
    in the convention of _denoise_rings (fwd[p]: frame p -> p+1; bwd[N-2-p]: frame p+1 -> p) -- what
    video_denoise(..., return_displacements=True) returns.  frames: uint8 CUDA tensor [N, H, W] or [N, H, W, 3]; sigma: the noise's
    standard deviation in grey levels, or a table uint16 [256].  reach=1 is _denoise_rings.  reach=2 (N >= 3) chains the rings first
    (fwd2 = chain_ring(fwd, 2): frame p -> p+2; bwd2 = chain_ring(bwd, 2): bwd2[N-3-p] is frame p+2 -> p), and frame f takes, in
    this order and skipping what lies outside the clip, frame f-1 with bwd[N-1-f], f+1 with fwd[f], f-2 with bwd2[N-1-f] and f+2
    with fwd2[f]: the stats slots 1 and 2 keep their meaning for interior frames, and where a chained vector is not defined the
    neighbour is not usable.  Returns the filtered clip and, with return_stats, int64 [N, 8] (temporal_filter's, per frame)."""
    assert reach in (1, 2), "reach: 1 or 2 frames on either side"
    if reach == 1:
        return _denoise_rings(frames, fwd, bwd, sigma, centre_weight, return_stats)
    return _denoise_reach2(frames, fwd, bwd, chain_ring(fwd, 2), chain_ring(bwd, 2), sigma, centre_weight, return_stats)


def _denoise_reach2(frames, fwd, bwd, fwd2, bwd2, weights, centre_weight, return_stats):
    """denoise_rings(reach=2) on the rings and their two-link chains"""
    import torch

    N, H, W = _clip_shape(frames)
    assert N >= 3 and int(fwd2.shape[0]) == N - 2 == int(bwd2.shape[0]), "reach 2: three frames or more"
    prm = _temporal_params(weights, centre_weight)
    out = torch.empty(tuple(frames.shape), dtype=torch.uint8, device=frames.device)
    stats = torch.empty((N, 8), dtype=torch.int64, device=frames.device) if return_stats else None
    for f0 in range(0, N, 16):
        items = []
        for f in range(f0, min(f0 + 16, N)):
            near = ([(frames[f - 1], bwd[N - 1 - f])] if f >= 1 else []) + ([(frames[f + 1], fwd[f])] if f + 1 < N else []) + \
                   ([(frames[f - 2], bwd2[N - 1 - f])] if f >= 2 else []) + ([(frames[f + 2], fwd2[f])] if f + 2 < N else [])
            items.append((frames[f], [p for p, _ in near], [d for _, d in near], out[f], stats[f] if return_stats else None))
        _temporal_launch(items, prm)
    return (out, stats) if return_stats else out


def _denoise_result(out, fwd, bwd, return_stats, return_displacements, chained=()):
    res = (out if isinstance(out, tuple) else (out,)) + ((fwd, bwd) + tuple(chained) if return_displacements else ())
    return res[0] if len(res) == 1 else res


def video_denoise(frames, levels: int, window: int, sigma, mode: str = "lk_float", iters: int = 1, min_det: float = 0.0,
                  batch: Optional[int] = None, centre_weight: int = 256, return_stats: bool = False, return_displacements: bool = False):
    """Temporal noise reduction of a grey clip: every frame averaged with the previous and the next one along the motion, by
    "temporal noise filter" of include/ofx.h.  The clip goes through the stream pipeline twice with a level-0 displacement ring, as
    it is and in reverse frame order, exactly as in video_interpolate; the frames then go through ofx_temporal_filter, up to 16 per
    launch, read in place, with the fields straight out of the two rings.

    frames: uint8 CUDA tensor [N, H, W], N >= 2, unit column stride.  sigma: the noise's standard deviation in grey levels
    (temporal_weights(sigma) is the table), or a table uint16 [256].  Returns the filtered clip, uint8 [N, H, W]; return_stats
    appends int64 [N, 8] (temporal_filter's, per frame; the end frames have one neighbour), return_displacements the two rings as
    video_interpolate does.  One frame on either side here; two with engine.denoise_rings(frames, fwd, bwd, sigma, reach=2) on the
    returned rings, which chains them (engine.chain_ring).  No recursive filter; not a stage of the stream pipeline itself."""
    assert frames.dim() == 3, "video_denoise: grey clips only, uint8 [N, H, W] (a colour clip [N, H, W, 3] goes through video_denoise_dense)"
    frames, N, H, W = _interp_clip(frames, 2)
    rings = []
    for order in (None, range(N - 1, -1, -1)):
        ring = _ring_for(N, H, W, 0, frames.device, None)
        _run_clip(frames, levels, window, mode, iters, min_det, batch, None, None, False,
                  lambda s, ring=ring: s.stream_displacement(ring, 0), order=order)
        rings.append(ring)
    out = _denoise_rings(frames, rings[0], rings[1], sigma, centre_weight, return_stats)
    return _denoise_result(out, rings[0], rings[1], return_stats, return_displacements)


def video_denoise_dense(frames, levels: int, window: int, sigma, iters: int = 3, min_det: float = 1.0, max_px: Optional[float] = None,
                        median: int = 0, mode: str = "lk_float", centre_weight: int = 256, return_stats: bool = False,
                        return_displacements: bool = False, reach: int = 1):
    """video_denoise with the displacements of the coarse-to-fine dense flow (_dense_ring at level 0, forwards and in reverse frame
    order, as video_interpolate_dense), for a grey clip [N, H, W] or an interleaved colour clip [N, H, W, 3]; a colour clip gets
    its flow from the channel average, made on the device, and all three channels of a pixel share one geometry and one set of
    weights.  median as video_displacement_dense's; the other arguments and the results as video_denoise's.  reach=2 (N >= 3)
    filters every frame with up to two frames on either side, as denoise_rings(reach=2) does, through the rings chained over two
    frames ("displacement chain" in include/ofx.h); return_displacements then appends fwd2 and bwd2 after fwd and bwd."""
    assert reach in (1, 2), "reach: 1 or 2 frames on either side"
    if frames.dim() == 4:
        frames, N, H, W = _interp_clip_colour(frames, 2)
        grey = _grey_clip(frames)
    else:
        frames, N, H, W = _interp_clip(frames, 2)
        grey = frames
    fwd = _dense_ring(grey, list(range(N)), levels, window, iters, min_det, max_px, 0, mode, None, median)
    bwd = _dense_ring(grey, list(range(N - 1, -1, -1)), levels, window, iters, min_det, max_px, 0, mode, None, median)
    if reach == 2:
        fwd2, bwd2 = chain_ring(fwd, 2), chain_ring(bwd, 2)
        out = _denoise_reach2(frames, fwd, bwd, fwd2, bwd2, sigma, centre_weight, return_stats)
        return _denoise_result(out, fwd, bwd, return_stats, return_displacements, (fwd2, bwd2))
    out = _denoise_rings(frames, fwd, bwd, sigma, centre_weight, return_stats)
    return _denoise_result(out, fwd, bwd, return_stats, return_displacements)
