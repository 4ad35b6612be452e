// The stream pipeline's sampled output stage (ofx_session_stream_arrows / _stream_tracks): for every pair one call of the pipeline
// completes, the arrow field of main.cu:123-169 and a set of points advected through the pairs -- the composed field of
// main.cu:138-147 (compose_px.h, the bits of ofx_compose_flow) read at a few positions instead of composed everywhere -- in ONE
// launch.  Also behind the stateless ofx_sample_arrows / ofx_advect_points.
//
// Shape: one grid, blockIdx.x < arrow_blocks are the arrow blocks, the rest the track blocks.
//   arrows: blockIdx.y is the pair, a thread is an arrow: its level loads, the ordered accumulation, clamp, one float add and
//     truncation per coordinate, ONE dwordx4 store of (x0, y0, x1, y1).
//   tracks: the track blocks of all gridDim.y rows form one linear range that strides over the points; a thread is a point.  It
//     loads position and status once, walks the call's pairs serially with the state in registers (the pair index is
//     wave-uniform: pointer selection stays in scalar loads), per pair issues all level loads, accumulates, adds and -- with a
//     history ring -- stores the position as one dwordx2; state and status are written once at the end.  The result therefore
//     does not depend on how many pairs a launch carries.
// Every store is plain C++.
#include <string.h>

#include "compose_px.h"

namespace {

constexpr int kThreads = 256;
constexpr unsigned kMaxTrackBlocks = 1u << 16; // (beyond this the point loop strides)

__device__ __forceinline__ void arrow(const ofx_sample_batch &A, int b, unsigned a)
{
    const int gi = (int)(a / (unsigned)A.a_nx), gj = (int)(a - (unsigned)gi * (unsigned)A.a_nx);
    const int i = gi * A.a_offset, j = gj * A.a_offset;
    float2 c = ofx_compose_px(ofx_px_pyramid_of(A.lv[b], A.own0, A.levels, A.a_level), A.a_w, i, j);
    // main.cu:150-157: a NaN fails every comparison and stays
    const float lim = (float)A.a_offset;
    if (c.x > lim)
        c.x = lim;
    else if (c.x < -lim)
        c.x = -lim;
    if (c.y > lim)
        c.y = lim;
    else if (c.y < -lim)
        c.y = -lim;
    const float fx = c.x + (float)j, fy = c.y + (float)i; // (finite or NaN: the clamp took the infinities)
    int x1 = -1, y1 = -1;
    if (fx == fx && fy == fy) {
        x1 = (int)fx, y1 = (int)fy;
        if (x1 < 0 || y1 < 0) x1 = y1 = -1;
    }
    reinterpret_cast<int4 *>(A.arrows[b])[a] = make_int4(j, i, x1, y1);
}

__device__ __forceinline__ bool is_finite(float v) { return fabsf(v) <= 3.402823466e+38f; } // (false for NaN)

__global__ __launch_bounds__(kThreads) void sample_ring_kernel(const ofx_sample_batch A, unsigned arrow_blocks)
{
    if (blockIdx.x < arrow_blocks) {
        const unsigned a = blockIdx.x * kThreads + threadIdx.x;
        if (a < (unsigned)(A.a_ny * A.a_nx)) arrow(A, (int)blockIdx.y, a);
        return;
    }
    const unsigned block = (blockIdx.x - arrow_blocks) * gridDim.y + blockIdx.y, blocks = (gridDim.x - arrow_blocks) * gridDim.y;
    const float fw = (float)A.t_w, fh = (float)A.t_h;
    for (size_t i = (size_t)block * kThreads + threadIdx.x; i < (size_t)A.n_points; i += (size_t)blocks * kThreads) {
        float2 p = reinterpret_cast<const float2 *>(A.points)[i];
        const int st0 = A.status[i];
        int st = st0;
        for (int b = 0; b < A.n; ++b) {
            const ofx_px_pyramid P = ofx_px_pyramid_of(A.lv[b], A.own0, A.levels, A.t_level);
            if (st == 0) {
                if (!(p.x >= 0.0f && p.x < fw && p.y >= 0.0f && p.y < fh)) {
                    st = A.pair0 + b;
                } else {
                    const float2 c = ofx_compose_px(P, A.t_w, (int)p.y, (int)p.x);
                    const float nx = p.x + c.x, ny = p.y + c.y;
                    if (is_finite(nx) && is_finite(ny))
                        p = make_float2(nx, ny);
                    else
                        st = A.pair0 + b;
                }
            }
            if (A.hist[b]) reinterpret_cast<float2 *>(A.hist[b])[i] = p;
        }
        if (st0 == 0) {
            reinterpret_cast<float2 *>(A.points)[i] = p;
            if (st != 0) A.status[i] = st;
        }
    }
}

} // namespace

int ofx_arrow_grid(int w, int h, int arrow_res, int *offset, int *ny, int *nx, const char *who)
{
    OFX_REQUIRE(w > 0 && h > 0 && arrow_res >= 1, "%s: bad arrow grid (%dx%d, arrow_res %d)", who, w, h, arrow_res);
    const int off = w / arrow_res;
    OFX_REQUIRE(off >= 1, "%s: arrow_res %d is more than the level's width %d (the grid step w / arrow_res would be 0)", who, arrow_res, w);
    *offset = off;
    *ny = (h + off - 1) / off;
    *nx = (w + off - 1) / off;
    return OFX_OK;
}

int ofx_check_sample_pyramid(int w, int h, int levels, int level, const char *who)
{
    OFX_REQUIRE(w > 0 && h > 0 && levels >= 1 && levels <= OFX_MAX_LEVELS && level >= 0 && level < levels, "%s: bad size or level", who);
    const int m = 1 << (levels - 1 - level);
    OFX_REQUIRE(w % m == 0 && h % m == 0, "%s: %dx%d is not a multiple of %d (the coarsest level's scale)", who, w, h, m);
    return OFX_OK;
}

int ofx_sample_batch_launch(const ofx_sample_batch *a, void *stream)
{
    OFX_REQUIRE(a && a->n >= 1 && a->n <= OFX_STREAM_MAX_BATCH && a->levels >= 1 && a->levels <= OFX_MAX_LEVELS,
                "ofx_sample_batch_launch: bad arguments");
    const bool arrows = a->arrows[0] != nullptr, tracks = a->points != nullptr;
    int lo = a->levels;
    unsigned arrow_blocks = 0, track_blocks = 0;
    if (arrows) {
        OFX_TRY(ofx_check_sample_pyramid(a->a_w, a->a_h, a->levels, a->a_level, "ofx_sample_batch_launch (arrows)"));
        OFX_REQUIRE(a->a_offset >= 1 && a->a_ny == (a->a_h + a->a_offset - 1) / a->a_offset && a->a_nx == (a->a_w + a->a_offset - 1) / a->a_offset,
                    "ofx_sample_batch_launch: arrow grid %d x %d does not belong to step %d on %dx%d", a->a_ny, a->a_nx, a->a_offset, a->a_w, a->a_h);
        OFX_REQUIRE((size_t)a->a_ny * (size_t)a->a_nx < ((size_t)1 << 31), "ofx_sample_batch_launch: too many arrows");
        for (int i = 0; i < a->n; ++i)
            OFX_REQUIRE(a->arrows[i] && ((uintptr_t)a->arrows[i] & 15) == 0, "ofx_sample_batch_launch: arrow slot %d must be 16-byte aligned", i);
        arrow_blocks = (unsigned)(((size_t)a->a_ny * (size_t)a->a_nx + kThreads - 1) / kThreads);
        lo = a->a_level;
    }
    if (tracks) {
        OFX_TRY(ofx_check_sample_pyramid(a->t_w, a->t_h, a->levels, a->t_level, "ofx_sample_batch_launch (tracks)"));
        OFX_REQUIRE(a->status && a->n_points >= 1 && a->pair0 >= 1, "ofx_sample_batch_launch: bad points, status or first pair");
        OFX_REQUIRE(((uintptr_t)a->points & 7) == 0 && ((uintptr_t)a->status & 3) == 0, "ofx_sample_batch_launch: points must be 8-byte, status 4-byte aligned");
        for (int i = 0; i < a->n; ++i)
            OFX_REQUIRE(((uintptr_t)a->hist[i] & 7) == 0, "ofx_sample_batch_launch: history slot %d must be 8-byte aligned", i);
        const unsigned need = (unsigned)(((size_t)a->n_points + kThreads - 1) / kThreads);
        const unsigned per_row = (need + (unsigned)a->n - 1) / (unsigned)a->n, cap = kMaxTrackBlocks / (unsigned)a->n;
        track_blocks = per_row < cap ? per_row : cap;
        lo = a->t_level < lo ? a->t_level : lo;
    }
    if (!arrows && !tracks) return OFX_OK;
    for (int i = 0; i < a->n; ++i)
        for (int k = lo; k < a->levels; ++k) OFX_REQUIRE(a->lv[i][k], "ofx_sample_batch_launch: pair %d level %d is null", i, k);
    dim3 grid(arrow_blocks + track_blocks, a->n);
    hipLaunchKernelGGL(sample_ring_kernel, grid, dim3(kThreads), 0, ofx_stream(stream), *a, arrow_blocks);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}

extern "C" int ofx_sample_arrows(const float *const *d_flow_levels, int w, int h, int levels, int level, int arrow_res, int32_t *d_dst, void *stream)
{
    OFX_REQUIRE(d_flow_levels && d_dst, "ofx_sample_arrows: null argument");
    OFX_TRY(ofx_check_sample_pyramid(w, h, levels, level, "ofx_sample_arrows"));
    static thread_local ofx_sample_batch sb;
    memset(&sb, 0, sizeof sb);
    OFX_TRY(ofx_arrow_grid(w, h, arrow_res, &sb.a_offset, &sb.a_ny, &sb.a_nx, "ofx_sample_arrows"));
    for (int k = level; k < levels; ++k) sb.lv[0][k] = d_flow_levels[k];
    sb.arrows[0] = d_dst;
    sb.n = 1, sb.levels = levels;
    sb.a_level = level, sb.a_w = w, sb.a_h = h;
    return ofx_sample_batch_launch(&sb, stream);
}

extern "C" int ofx_advect_points(const float *const *d_flow_levels, int w, int h, int levels, int level, int pair, float *d_points,
                                 int32_t *d_status, int n_points, void *stream)
{
    OFX_REQUIRE(d_flow_levels && d_points && d_status, "ofx_advect_points: null argument");
    OFX_REQUIRE(pair >= 1 && n_points >= 1, "ofx_advect_points: pair %d (the status a lost point gets) and n_points %d must be >= 1", pair, n_points);
    OFX_TRY(ofx_check_sample_pyramid(w, h, levels, level, "ofx_advect_points"));
    static thread_local ofx_sample_batch sb;
    memset(&sb, 0, sizeof sb);
    for (int k = level; k < levels; ++k) sb.lv[0][k] = d_flow_levels[k];
    sb.points = d_points, sb.status = d_status;
    sb.n = 1, sb.levels = levels;
    sb.t_level = level, sb.t_w = w, sb.t_h = h, sb.n_points = n_points, sb.pair0 = pair;
    return ofx_sample_batch_launch(&sb, stream);
}
