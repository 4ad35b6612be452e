"""ctypes binding of libofx_hip.so (the C ABI declared in include/ofx.h).

There is no CPU fallback: if the library is missing or fails to load, importing the engine raises.
"""
from __future__ import annotations

import ctypes as C
import os

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG, os.environ.get("OFX_LIB", "libofx_hip.so"))  # OFX_LIB: A/B an alternative build

OFX_MAX_LEVELS = 12
MODE_COMPAT_CPU = 0
MODE_LK_FLOAT = 1
MODE_LK_FLOAT_FAST = 2   # lk_float with the <= 1 ulp solve (include/ofx.h)
MODES = {"compat_cpu": MODE_COMPAT_CPU, "lk_float": MODE_LK_FLOAT, "lk_float_fast": MODE_LK_FLOAT_FAST}
SOLVE_F64, SOLVE_INLINE_CPU, SOLVE_F32 = 0, 1, 2


class OfxError(RuntimeError):
    pass


class Geom(C.Structure):
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("pitch", C.c_int), ("row0", C.c_int), ("rows", C.c_int),
                ("out_y0", C.c_int), ("out_y1", C.c_int)]

    @classmethod
    def full(cls, w, h, pitch):
        return cls(w, h, pitch, 0, h, 0, h)


class Params(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("levels", C.c_int), ("window", C.c_int), ("mode", C.c_int),
                ("device", C.c_int), ("sharded", C.c_int),
                ("own_y0", C.c_int * OFX_MAX_LEVELS), ("own_y1", C.c_int * OFX_MAX_LEVELS),
                ("buf_y0", C.c_int * OFX_MAX_LEVELS), ("buf_y1", C.c_int * OFX_MAX_LEVELS),
                ("comp_y0", C.c_int * OFX_MAX_LEVELS), ("comp_y1", C.c_int * OFX_MAX_LEVELS),
                ("iters", C.c_int), ("local_corner", C.c_int), ("patch_size", C.c_int), ("stream_batch", C.c_int), ("borrow_frames", C.c_int), ("min_det", C.c_float),
                ("stream_two_stage", C.c_int), ("frames_partial", C.c_int), ("deep_fetch", C.c_int)]


class ProlongDesc(C.Structure):
    """ofx_prolong_desc (include/ofx.h, "coarse-to-fine propagation")"""
    _fields_ = [("d_coarse", C.c_void_p), ("wc", C.c_int), ("hc", C.c_int), ("d_fine", C.c_void_p), ("w", C.c_int), ("h", C.c_int),
                ("scale", C.c_float), ("max_px", C.c_float), ("d_src", C.c_void_p), ("src_pitch", C.c_int), ("d_dst", C.c_void_p),
                ("dst_pitch", C.c_int)]


class MedianDesc(C.Structure):
    """ofx_median_desc (include/ofx.h, "flow median")"""
    _fields_ = [("d_src_flow", C.c_void_p), ("d_dst_flow", C.c_void_p), ("w", C.c_int), ("h", C.c_int), ("radius", C.c_int),
                ("scale", C.c_float), ("d_src", C.c_void_p), ("src_pitch", C.c_int), ("d_dst", C.c_void_p), ("dst_pitch", C.c_int)]


class TextureDesc(C.Structure):
    """ofx_texture_desc (include/ofx.h, "texture strength and feature selection")"""
    _fields_ = [("d_plane", C.c_void_p), ("pitch", C.c_int), ("w", C.c_int), ("h", C.c_int), ("d_strength", C.c_void_p),
                ("strength_pitch", C.c_int), ("d_cells", C.c_void_p), ("d_cell_strength", C.c_void_p), ("d_stats", C.c_void_p),
                ("cell", C.c_int), ("border", C.c_int), ("min_strength", C.c_float)]


class TrackClip(C.Structure):
    """ofx_track_clip (include/ofx.h, "sparse Lucas-Kanade tracking"): planes and pitches are host tables"""
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("levels", C.c_int), ("n_frames", C.c_int), ("planes", C.POINTER(C.c_void_p)),
                ("pitches", C.POINTER(C.c_int))]


class TrackParams(C.Structure):
    """ofx_track_params (include/ofx.h, "sparse Lucas-Kanade tracking")"""
    _fields_ = [("window", C.c_int), ("max_iters", C.c_int), ("eps_q", C.c_int), ("max_sad", C.c_int), ("min_lambda", C.c_float)]


class FitDesc(C.Structure):
    """ofx_fit_desc (include/ofx.h, "camera motion from point matches"; d_model is float64 [9] for ofx_fit_homography)"""
    _fields_ = [("d_p", C.c_void_p), ("d_q", C.c_void_p), ("d_status", C.c_void_p), ("n", C.c_int), ("pair", C.c_int), ("w", C.c_int),
                ("h", C.c_int), ("d_model", C.c_void_p), ("d_info", C.c_void_p), ("d_inlier", C.c_void_p), ("d_work", C.c_void_p)]


class FitParams(C.Structure):
    """ofx_fit_params (include/ofx.h, "camera motion from point matches")"""
    _fields_ = [("model", C.c_int), ("hypotheses", C.c_int), ("thr_q", C.c_int), ("refits", C.c_int), ("seed", C.c_uint32)]


class WarpAffineDesc(C.Structure):
    """ofx_warp_affine_desc (include/ofx.h, "affine frame warp")"""
    _fields_ = [("d_src", C.c_void_p), ("src_pitch", C.c_int), ("sw", C.c_int), ("sh", C.c_int), ("d_dst", C.c_void_p), ("dst_pitch", C.c_int),
                ("w", C.c_int), ("h", C.c_int), ("channels", C.c_int), ("border", C.c_int), ("fill", C.c_int), ("model", C.c_double * 6),
                ("d_outside", C.c_void_p)]


class WarpPerspDesc(C.Structure):
    """ofx_warp_persp_desc (include/ofx.h, "perspective frame warp")"""
    _fields_ = [("d_src", C.c_void_p), ("src_pitch", C.c_int), ("sw", C.c_int), ("sh", C.c_int), ("d_dst", C.c_void_p), ("dst_pitch", C.c_int),
                ("w", C.c_int), ("h", C.c_int), ("channels", C.c_int), ("border", C.c_int), ("fill", C.c_int), ("model", C.c_double * 9),
                ("d_outside", C.c_void_p)]


OFX_MOSAIC_MAX_SOURCES = 9


class MosaicSource(C.Structure):
    """ofx_mosaic_source (include/ofx.h, "frame mosaic")"""
    _fields_ = [("d_src", C.c_void_p), ("src_pitch", C.c_int), ("sw", C.c_int), ("sh", C.c_int), ("model", C.c_double * 9)]


class MosaicDesc(C.Structure):
    """ofx_mosaic_desc (include/ofx.h, "frame mosaic")"""
    _fields_ = [("source", MosaicSource * OFX_MOSAIC_MAX_SOURCES), ("n_sources", C.c_int), ("d_dst", C.c_void_p), ("dst_pitch", C.c_int),
                ("w", C.c_int), ("h", C.c_int), ("channels", C.c_int), ("border", C.c_int), ("fill", C.c_int), ("d_which", C.c_void_p),
                ("which_pitch", C.c_int), ("d_counts", C.c_void_p)]


OFX_TEMPORAL_MAX_NEIGHBOURS = 4


class TemporalNeighbour(C.Structure):
    """ofx_temporal_neighbour (include/ofx.h, "temporal noise filter")"""
    _fields_ = [("d_plane", C.c_void_p), ("pitch", C.c_int), ("pad", C.c_int), ("d_field", C.c_void_p)]


class TemporalDesc(C.Structure):
    """ofx_temporal_desc (include/ofx.h, "temporal noise filter")"""
    _fields_ = [("neighbour", TemporalNeighbour * OFX_TEMPORAL_MAX_NEIGHBOURS), ("n_neighbours", C.c_int), ("w", C.c_int), ("h", C.c_int),
                ("channels", C.c_int), ("d_centre", C.c_void_p), ("centre_pitch", C.c_int), ("dst_pitch", C.c_int), ("d_dst", C.c_void_p),
                ("d_stats", C.c_void_p)]


class TemporalParams(C.Structure):
    """ofx_temporal_params (include/ofx.h, "temporal noise filter")"""
    _fields_ = [("weights", C.c_uint16 * 256), ("centre_weight", C.c_int), ("reserved", C.c_int)]


OFX_CHAIN_MAX_LINKS = 4


class ChainDesc(C.Structure):
    """ofx_chain_desc (include/ofx.h, "displacement chain")"""
    _fields_ = [("d_link", C.c_void_p * OFX_CHAIN_MAX_LINKS), ("n_links", C.c_int), ("w", C.c_int), ("h", C.c_int), ("mask_pitch", C.c_int),
                ("d_dst", C.c_void_p), ("d_mask", C.c_void_p), ("d_stats", C.c_void_p)]


class LkDesc(C.Structure):
    """ofx_lk_desc (include/ofx.h): one level of an ofx_lk_levels / ofx_corner_flows launch"""
    _fields_ = [("d_prev", C.c_void_p), ("d_next", C.c_void_p), ("geom", Geom), ("d_flow", C.c_void_p), ("flow_row0", C.c_int),
                ("d_uv", C.c_void_p), ("accumulate", C.c_int), ("min_det", C.c_float), ("d_warp_src", C.c_void_p),
                ("d_warp_out", C.c_void_p), ("warp_scale", C.c_float), ("d_warp_status", C.c_void_p), ("warp_status_bit", C.c_int)]


class ShiftDesc(C.Structure):
    """ofx_shift_desc (include/ofx.h): one level of an ofx_shift_levels launch"""
    _fields_ = [("d_src", C.c_void_p), ("d_dst", C.c_void_p), ("geom", Geom), ("d_uv", C.c_void_p)]


class WarpDesc(C.Structure):
    """ofx_warp_desc (include/ofx.h): one level of an ofx_warp_levels launch"""
    _fields_ = [("d_src", C.c_void_p), ("d_dst", C.c_void_p), ("geom", Geom), ("d_flow", C.c_void_p), ("flow_row0", C.c_int),
                ("scale", C.c_float), ("d_status", C.c_void_p), ("status_bit", C.c_int)]


_vp = C.c_void_p
_i = C.c_int
_d = C.c_double
_gp = C.POINTER(Geom)

# name -> argtypes; every function returns int unless listed in _RESTYPE
_SIGS = {
    "ofx_abi_version": [],
    "ofx_device_count": [],
    "ofx_lk_level": [_vp, _vp, _gp, _i, _i, _vp, _i, _vp],
    "ofx_lk_levels": [_vp, _i, _i, _i, _vp],
    "ofx_corner_flows": [_vp, _i, _i, _i, _vp, _vp],
    "ofx_shift_levels": [_vp, _i, _vp],
    "ofx_lk_level_sums": [_vp, _vp, _gp, _i, _i, _vp, _i, _vp],
    "ofx_downsample_1ch": [_vp, _i, _i, _i, _vp, _gp, _vp],
    "ofx_pyramid_1ch": [_vp, _i, _i, _i, C.POINTER(_vp), C.POINTER(_i), _i, _vp],
    "ofx_shift_vector": [C.POINTER(_vp), _i, _i, _vp, _vp],
    "ofx_shift_1ch": [_vp, _vp, _gp, _vp, _vp],
    "ofx_warp_levels": [_vp, _i, _vp],
    "ofx_compose_flow": [C.POINTER(_vp), _i, _i, _i, _i, _vp, _vp],
    "ofx_extract_ch0": [_vp, _vp, _i, _i, _i, _vp],
    "ofx_replicate_3ch": [_vp, _i, _vp, _i, _i, _vp],
    "ofx_grayscale_avg_3ch": [_vp, _vp, _i, _i, _vp],
    "ofx_conv_3ch": [_vp, _vp, _i, _i, _vp, _i, _i, _i, _vp],
    "ofx_conv_3ch_1ch_u8": [_vp, _i, _i, _vp, _vp, _i, _i, _vp],
    "ofx_conv_3ch_1ch_f32": [_vp, _i, _i, _vp, _vp, _i, _i, _vp],
    "ofx_downsample_3ch": [_vp, _vp, _i, _i, _vp],
    "ofx_srm_u8": [_vp, _vp, _i, _i, _i, _i, _vp, _vp],
    "ofx_srm_f32": [_vp, _vp, _i, _i, _i, _i, _vp, _vp],
    "ofx_solve_i32": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp],
    "ofx_solve_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp],
    "ofx_generate_gaussian_kernel": [_d, _i, _vp],
    "ofx_bilateral_3ch": [_vp, _vp, _vp, _i, _i, _i, _i, _d, _d, _vp],
    "ofx_bilateral_3ch_fast": [_vp, _vp, _vp, _i, _i, _i, _i, _d, _d, _vp],
    "ofx_bilateral_wrappers_fast": [_i],
    "ofx_frontend_1ch": [C.POINTER(_vp), C.POINTER(_i), _i, C.POINTER(_vp), C.POINTER(_i), _i, _i, _i, _i, C.POINTER(_i), _i, _i, _d, _d, _vp],
    "ofx_sub_u8": [_vp, _vp, C.c_size_t, _vp, _vp],
    "ofx_srm_3ch_u8": [_vp, _vp, _i, _i, _i, _i, _vp, _vp],
    "ofx_downscale_mask_3ch": [_vp, _vp, _i, _i, _vp, _i, _i, _vp],
    "ofx_shift_3ch": [_vp, _vp, _i, _i, _vp, _vp],
    "ofx_session_create": [C.POINTER(Params), C.POINTER(_vp)],
    "ofx_session_destroy": [_vp],
    "ofx_session_set_frame_host": [_vp, _vp, _vp],
    "ofx_session_set_frame_host_3ch": [_vp, _vp, _vp],
    "ofx_session_set_frame_device": [_vp, _vp, _i, _vp],
    "ofx_session_build_pyramid": [_vp, _vp],
    "ofx_session_downsample_level": [_vp, _i, _vp],
    "ofx_session_run_flow": [_vp, _vp],
    "ofx_session_corner_flows": [_vp, _vp],
    "ofx_session_run_levels": [_vp, _vp],
    "ofx_session_run_flow_sequential": [_vp, _vp],
    "ofx_session_compute_uv": [_vp, _i, _vp],
    "ofx_session_run_level": [_vp, _i, _vp],
    "ofx_session_swap": [_vp],
    "ofx_session_stream_begin": [_vp],
    "ofx_session_corner_status": [_vp, C.POINTER(_i), _vp],
    "ofx_session_pair_status": [_vp, _i, C.POINTER(_i), _vp],
    "ofx_stage_threads": [],
    "ofx_debug_stream_trace": [_vp, _i, C.POINTER(_i)],
    "ofx_session_flow_of": [_vp, _i, _i, C.POINTER(_vp), C.POINTER(_i), C.POINTER(_i)],
    "ofx_session_stream_compose": [_vp, _i, _vp, C.c_size_t, _i],
    "ofx_session_composed_of": [_vp, _i, C.POINTER(_vp), C.POINTER(_i), C.POINTER(_i)],
    "ofx_sample_arrows": [C.POINTER(_vp), _i, _i, _i, _i, _i, _vp, _vp],
    "ofx_advect_points": [C.POINTER(_vp), _i, _i, _i, _i, _i, _vp, _vp, _i, _vp],
    "ofx_session_stream_arrows": [_vp, _i, _i, _vp, C.c_size_t, _i],
    "ofx_session_arrows_of": [_vp, _i, C.POINTER(_vp), C.POINTER(_i), C.POINTER(_i)],
    "ofx_session_stream_tracks": [_vp, _i, _vp, _vp, _i, _vp, C.c_size_t, _i],
    "ofx_motion_compensate": [_vp, _i, _vp, _i, _i, _i, _vp, _vp, C.c_float, _vp, _i, _vp, _vp],
    "ofx_session_stream_motion": [_vp, _i, C.c_float, _vp, _i, C.c_size_t, _i, _vp],
    "ofx_session_motion_of": [_vp, _i, C.POINTER(_vp), C.POINTER(_i), C.POINTER(_vp)],
    "ofx_flow_consistency": [_vp, _vp, _i, _i, C.c_float, C.c_float, C.c_float, _vp, _i, _vp, _vp, _vp],
    "ofx_flow_consistency_batch": [C.POINTER(_vp), C.POINTER(_vp), _i, _i, _i, C.c_float, C.c_float, C.c_float, C.POINTER(_vp), _i,
                                   C.POINTER(_vp), C.POINTER(_vp), _vp],
    "ofx_flow_displacement": [_vp, _i, _i, _vp, C.c_float, _vp, _vp],
    "ofx_session_stream_displacement": [_vp, _i, C.c_float, _vp, C.c_size_t, _i],
    "ofx_session_displacement_of": [_vp, _i, C.POINTER(_vp)],
    "ofx_flow_prolong": [C.POINTER(ProlongDesc), _i, _vp],
    "ofx_session_run_flow_dense": [_vp, C.c_float, _vp],
    "ofx_flow_median": [C.POINTER(MedianDesc), _i, _vp],
    "ofx_session_run_flow_dense_median": [_vp, C.c_float, _i, _vp, C.c_size_t, _vp],
    "ofx_session_dense_median_scratch_bytes": [_vp, C.POINTER(C.c_size_t)],
    "ofx_texture_features": [C.POINTER(TextureDesc), _i, _i, _vp],
    "ofx_compact_features": [_vp, _i, _i, _vp, _vp, _vp],
    "ofx_track_points": [C.POINTER(TrackClip), C.POINTER(TrackParams), _i, _vp, _vp, _i, _vp, _vp, _vp, _vp],
    "ofx_fit_motion_work_bytes": [C.POINTER(FitParams)],
    "ofx_fit_motion": [C.POINTER(FitDesc), _i, C.POINTER(FitParams), _vp],
    "ofx_fit_homography_work_bytes": [C.POINTER(FitParams)],
    "ofx_fit_homography": [C.POINTER(FitDesc), _i, C.POINTER(FitParams), _vp],
    "ofx_motion_compose": [_vp, _vp, _vp],
    "ofx_motion_invert": [_vp, _vp],
    "ofx_warp_affine": [C.POINTER(WarpAffineDesc), _i, _vp],
    "ofx_warp_perspective": [C.POINTER(WarpPerspDesc), _i, _vp],
    "ofx_warp_mosaic": [C.POINTER(MosaicDesc), _i, _vp],
    "ofx_temporal_filter": [C.POINTER(TemporalDesc), _i, C.POINTER(TemporalParams), _vp],
    "ofx_displacement_chain": [C.POINTER(ChainDesc), _i, _vp],
    "ofx_homography_compose": [_vp, _vp, _vp],
    "ofx_homography_invert": [_vp, _vp],
    "ofx_homography_normalize": [_vp, _vp],
    "ofx_homography_from_affine": [_vp, _vp],
    "ofx_interpolate_frames": [_vp, _i, _vp, _i, _i, _i, _vp, _vp, C.POINTER(C.c_float), _i, _vp, _i, C.c_size_t, _vp, _vp],
    "ofx_interpolate_frames_batch": [C.POINTER(_vp), C.POINTER(_i), C.POINTER(_vp), C.POINTER(_i), _i, _i, _i, C.POINTER(_vp), C.POINTER(_vp),
                                     C.POINTER(C.c_float), _i, C.POINTER(_vp), _i, C.c_size_t, C.POINTER(_vp), _vp],
    "ofx_interpolate_frames_3ch": [_vp, _i, _vp, _i, _i, _i, _vp, _vp, C.POINTER(C.c_float), _i, _vp, _i, C.c_size_t, _vp, _vp],
    "ofx_interpolate_frames_3ch_batch": [C.POINTER(_vp), C.POINTER(_i), C.POINTER(_vp), C.POINTER(_i), _i, _i, _i, C.POINTER(_vp), C.POINTER(_vp),
                                         C.POINTER(C.c_float), _i, C.POINTER(_vp), _i, C.c_size_t, C.POINTER(_vp), _vp],
    "ofx_session_stream_frontend": [_vp, _i, _i, _d, _d, _i],
    "ofx_session_stream_submit_3ch": [_vp, _vp, _i, _vp, C.POINTER(_i)],
    "ofx_session_stream_submit_frames_3ch": [_vp, C.POINTER(_vp), C.POINTER(_i), _i, _i, _vp, C.POINTER(_i)],
    "ofx_session_stream_submit": [_vp, _vp, _i, _vp, C.POINTER(_i)],
    "ofx_session_stream_drain": [_vp, _vp, C.POINTER(_i)],
    "ofx_session_stream_submit_frames": [_vp, C.POINTER(_vp), C.POINTER(_i), _i, _i, _vp, C.POINTER(_i)],
    "ofx_stream_launch": [_vp, _i, _i, _vp],
    "ofx_session_submit_device": [_vp, _vp, _i, _vp],
    "ofx_session_stage_frame": [_vp, _vp, _i, _vp],
    "ofx_session_stage_shift": [_vp, _vp],
    "ofx_session_solve_staged": [_vp, _vp],
    "ofx_session_aux_stream": [_vp, C.POINTER(_vp)],
    "ofx_session_plane": [_vp, _i, _i, C.POINTER(_vp), _gp],
    "ofx_session_flow": [_vp, _i, C.POINTER(_vp), C.POINTER(_i), C.POINTER(_i)],
    "ofx_session_shift_uv": [_vp, _i, C.POINTER(_vp)],
    "ofx_session_get_flow_host": [_vp, _i, _vp, _vp],
    "ofx_session_timing": [_vp, _i],
    "ofx_session_timing_read": [_vp, C.POINTER(_d), C.POINTER(_d), C.POINTER(_i)],
    "ofx_session_timing_read_kind": [_vp, _i, C.POINTER(_d), C.POINTER(_d), C.POINTER(_i)],
    "ofx_compose_flow_host": [C.POINTER(_vp), _i, _i, _i, _i, _vp],
    "ofx_calc_opt_flow_host": [_vp, _vp, _i, _i, C.POINTER(_vp), _i, _i, _i, _i],
}
_RESTYPE = {"ofx_generate_gaussian_kernel": None, "ofx_fit_motion_work_bytes": C.c_size_t, "ofx_fit_homography_work_bytes": C.c_size_t}

EXPORTS = sorted(list(_SIGS) + ["ofx_last_error"])

_lib = None


def load() -> C.CDLL:
    """Load libofx_hip.so once.  Raises if it has not been built (python -m cuda_optical_flow_2_amd.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OfxError(f"{LIB_PATH} is missing: build it with `python -m cuda_optical_flow_2_amd.build` "
                       "(hipcc, gfx950). This engine has no CPU fallback.")
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7 (same SONAME as /opt/rocm's).  Import
    # torch first so that our library binds to the runtime torch's tensors and streams live in; loading ours first
    # would bring in a second, different runtime (on the GPU boxes of this pool that one does not even see the device).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, args in _SIGS.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = _RESTYPE.get(name, C.c_int)
    lib.ofx_last_error.restype = C.c_char_p
    lib.ofx_last_error.argtypes = []
    _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().ofx_last_error()
        raise OfxError(f"{what or 'ofx call'} failed (code {rc}): {msg.decode() if msg else ''}")
