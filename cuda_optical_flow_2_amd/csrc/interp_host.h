// The host side of frame interpolation, grey (interp.hip) and colour (interp3.hip): one batch builder for the two exported batch
// calls and one launch function body for ofx_interp_batch_launch and ofx_interp3_batch_launch.  The two differ in the kernel, in
// the planes' bytes per pixel and in the argument names their messages use; ofx_interp3_batch is ofx_interp_batch.
#pragma once
#include <string.h>

#include "quad_stage.h"

namespace quad {

// the names of the plane and frame arguments in the entry points' messages: d_a, d_b, d_dst or d_a3, d_b3, d_dst3
struct InterpNames {
    const char *a, *b, *dst;
};

// fill *ib from the arguments of ofx_interpolate_frames_batch / ofx_interpolate_frames_3ch_batch (`who`), including the
// definition's host step for the times; what it does not look at, the launch function checks
inline int interp_fill_batch(const char *who, const InterpNames &nm, ofx_interp_batch *ib, const uint8_t *const *d_a, const int *a_pitches,
                             const uint8_t *const *d_b, const int *b_pitches, int n, int w, int h, const float *const *d_disp_ab,
                             const float *const *d_disp_ba, const float *h_times, int n_times, uint8_t *const *d_dst, int dst_pitch,
                             size_t time_stride_bytes, int64_t *const *d_stats)
{
    OFX_REQUIRE(d_a && d_b && a_pitches && b_pitches, "%s: null plane or pitch array (%s, %s, a_pitches, b_pitches)", who, nm.a, nm.b);
    OFX_REQUIRE(d_disp_ab && d_disp_ba, "%s: null field array (d_disp_ab, d_disp_ba)", who);
    OFX_REQUIRE(d_dst, "%s: %s is null", who, nm.dst);
    OFX_REQUIRE(h_times, "%s: h_times is null", who);
    OFX_REQUIRE(n >= 1 && n <= OFX_STREAM_MAX_BATCH, "%s: n = %d is not in 1 .. %d", who, n, OFX_STREAM_MAX_BATCH);
    OFX_REQUIRE(n_times >= 1 && n_times <= OFX_INTERP_MAX_TIMES, "%s: n_times = %d is not in 1 .. %d", who, n_times, OFX_INTERP_MAX_TIMES);
    memset(ib, 0, sizeof *ib);
    ib->n = n, ib->w = w, ib->h = h, ib->n_times = n_times, ib->dst_pitch = dst_pitch, ib->time_stride = time_stride_bytes;
    for (int k = 0; k < n_times; ++k) { // the definition's host step, in float32
        const float t = h_times[k], omt = 1.0f - t;
        ib->t[k] = t, ib->c00[k] = -(omt * t), ib->c01[k] = t * t, ib->c10[k] = omt * omt;
    }
    for (int i = 0; i < n; ++i) {
        OFX_REQUIRE(d_a[i] && d_b[i] && d_disp_ab[i] && d_disp_ba[i] && d_dst[i] && (!d_stats || d_stats[i]), "%s: pair %d: a null entry in an array", who, i);
        ib->a[i] = d_a[i], ib->a_pitch[i] = a_pitches[i], ib->b[i] = d_b[i], ib->b_pitch[i] = b_pitches[i];
        ib->dab[i] = d_disp_ab[i], ib->dba[i] = d_disp_ba[i], ib->dst[i] = d_dst[i];
        ib->stats[i] = d_stats ? reinterpret_cast<unsigned long long *>(d_stats[i]) : nullptr;
    }
    return OFX_OK;
}

// check every argument, zero the stats slots on the stream, launch `kernel` over planes of bpp bytes per pixel.  The kernel gets
// `dwords`: whole quads of a frame may leave as dwords (every destination, dst_pitch and the time stride 4-byte aligned).
template <typename Batch>
inline int interp_launch(const char *who, void (*kernel)(const Batch, const int), int bpp, const InterpNames &nm, const Batch *a, void *stream)
{
    OFX_REQUIRE(a, "%s: bad arguments", who);
    OFX_TRY(check_batch(who, a->n, a->w, a->h, bpp, {a->a_pitch, a->b_pitch}, {a->dab, a->dba}, a->stats));
    OFX_REQUIRE(a->n_times >= 1 && a->n_times <= OFX_INTERP_MAX_TIMES, "%s: n_times = %d is not in 1 .. %d", who, a->n_times, OFX_INTERP_MAX_TIMES);
    for (int k = 0; k < a->n_times; ++k)
        OFX_REQUIRE(__builtin_isfinite(a->t[k]) && a->t[k] > 0.0f && a->t[k] < 1.0f, "%s: h_times[%d] = %g is not in (0, 1)", who, k, (double)a->t[k]);
    OFX_REQUIRE(a->dst_pitch >= bpp * a->w, "%s: dst_pitch %d is below the %d bytes of a row of width %d", who, a->dst_pitch, bpp * a->w, a->w);
    OFX_REQUIRE(a->n_times == 1 || a->time_stride >= (size_t)a->h * (size_t)a->dst_pitch,
                "%s: time_stride_bytes %zu is below a frame's h * dst_pitch = %zu bytes", who, a->time_stride, (size_t)a->h * (size_t)a->dst_pitch);
    bool dwords = (a->dst_pitch & 3) == 0 && (a->n_times == 1 || (a->time_stride & 3) == 0);
    for (int i = 0; i < a->n; ++i) {
        OFX_REQUIRE(a->a[i] && a->b[i], "%s: pair %d: a null plane (%s, %s)", who, i, nm.a, nm.b);
        OFX_REQUIRE(a->dst[i], "%s: pair %d: %s is null", who, i, nm.dst);
        dwords = dwords && ((uintptr_t)a->dst[i] & 3) == 0;
    }
    OFX_TRY(zero_stats(a->stats, a->n, 4 * (size_t)a->n_times, stream)); // (everything is checked; a slot: four words per time)
    hipLaunchKernelGGL(kernel, grid(a->w, a->h, a->n), dim3(kThreads), 0, ofx_stream(stream), *a, (int)dwords);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}

} // namespace quad
