// The flow median (ofx_flow_median): a 3x3 or 5x5 median of a flow field, per component, and, fused, the next image warped by the
// filtered field.  The definition is the comment block "flow median" in include/ofx.h.  A median is a selection: nothing below
// rounds, except the one add that turns a selected -0 into +0.
//
// One launch, blockIdx.y = the descriptor; the quad, its loads and its stores are quad_stage.h's: a thread owns four adjacent
// pixels of one row and takes kQuads quads, one after the other.  The PLACES are not the row-major ones of quad_stage.h: a block
// covers a tile of 256 columns x 16 rows, a wave one row of it per step (wave i the rows i, 4 + i, 8 + i, 12 + i), because the
// window's rows are then the block's own: in row-major order the 2r + 1 rows a quad reads belong to 2r + 1 other blocks, which the
// dispatcher deals to other XCDs, and every row crossed the fabric 2r + 1 times (DESIGN.md section 4.15 has both timings).  The
// windows cover the columns x0 - r .. x0 + 3 + r on the rows y - r .. y + r, clamped to the field: per row the quad's own four
// vectors by two 16-byte loads (load_field's: a row's ragged end reads on into the next row, or 0 past the field, and the lane
// then copies its last own column over what it got), and the r columns either side by one 8-byte load each at a clamped position.
// Every load goes through a buffer resource of exactly the field's w * h * 8 bytes and every vector is sanitised as it arrives,
// so no NaN reaches v_min_f32 / v_max_f32 / v_med3_f32.  A column of the window is ordered once for all outputs that contain it;
// the networks and the reason they select the median are in median_net.h.
//
// The filtered quad stays in registers: it leaves by quad_part_flow_store.h and feeds the fused warp, quad_part_warp.h, the two
// parts this kernel shares with prolong_kernel (the rules of both are stated there).
//
// Traffic: 8 B read and 8 B written per pixel, and with the warp 1 B of taps and 1 B written; the (2r + 1) rows x (4 + 2r) columns
// a thread loads are its neighbours' too and come from the vector cache.
#include <string.h>

#include "quad_stage.h"

namespace {

using namespace quad;

// (the sanitised operands are never NaN, so these are plain selections: v_min_f32, v_max_f32, v_med3_f32)
__device__ __forceinline__ float lo(float a, float b) { return __builtin_fminf(a, b); }
__device__ __forceinline__ float hi(float a, float b) { return __builtin_fmaxf(a, b); }
__device__ __forceinline__ float mid3(float a, float b, float c) { return __builtin_amdgcn_fmed3f(a, b, c); }

} // namespace

#include "median_net.h"

namespace {

struct MedianItem {
    const float *src_flow;
    float *dst_flow;
    const uint8_t *src;
    uint8_t *dst;
    int w, h, radius, src_pitch, dst_pitch, dwords;
    float scale;
};
struct MedianArgs {
    MedianItem it[OFX_STREAM_MAX_BATCH];
};

constexpr int kTileQuads = 64;                          // a tile's width in quads: one per lane of a wave
constexpr int kTileRows = kQuads * (kThreads / 64);     // and its height: a row per wave and step

// the tiles of a w x h field: (across, down)
__host__ __device__ inline uint32_t tiles_across(int w) { return ((uint32_t)(w + 3) / 4 + kTileQuads - 1) / kTileQuads; }
__host__ __device__ inline uint32_t tiles_down(int h) { return ((uint32_t)h + kTileRows - 1) / kTileRows; }

// the place (y, x0) of this thread's g-th quad in the block's tile; false: outside the field -- and then so are the later ones
__device__ __forceinline__ bool place_tile(int w, int h, int g, int &y, int &x0)
{
    const uint32_t across = tiles_across(w), ty = blockIdx.x / across, tx = blockIdx.x - ty * across;
    x0 = 4 * (int)(tx * kTileQuads + (threadIdx.x & 63));
    y = (int)(ty * kTileRows) + (kThreads / 64) * g + (int)(threadIdx.x >> 6);
    return x0 < w && y < h;
}

// step 1 of the definition: a vector with a component that is not finite reads as (+0, +0)
__device__ __forceinline__ void sanitise(float &u, float &v)
{
    const bool bad = !(__builtin_fabsf(u) < __builtin_inff() && __builtin_fabsf(v) < __builtin_inff()); // (a NaN fails)
    u = bad ? 0.0f : u, v = bad ? 0.0f : v;
}

// the filtered vectors of the quad at (y, x0): fu / fv[k] = the median of the window around pixel x0 + k (steps 1 to 3)
template <int R> __device__ __forceinline__ void median_quad(const __amdgpu_buffer_rsrc_t &rs, int w, int h, int y, int x0, int npx, float *fu, float *fv)
{
    constexpr int NR = 2 * R + 1, NC = 4 + 2 * R;
    float U[NC][NR], V[NC][NR];
    uint32_t side[2 * R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
        side[i] = (uint32_t)max(x0 - R + i, 0);         // columns x0 - R .. x0 - 1
        side[R + i] = (uint32_t)min(x0 + 4 + i, w - 1); // columns x0 + 4 .. x0 + 3 + R
    }
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        const int yy = min(max(y + j - R, 0), h - 1);
        const uint32_t row = (uint32_t)yy * (uint32_t)w;
        float f[8];
        load_field(rs, w, true, yy, x0, f);
#pragma unroll
        for (int i = 0; i < 2 * R; ++i) {
            const f32x2 t = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rs, 8u * (row + side[i]), 0, 0));
            const int c = i < R ? i : 4 + i;
            U[c][j] = t[0], V[c][j] = t[1];
        }
        // past the row's end the window reads column w - 1 = the quad's last own column
#pragma unroll
        for (int k = 1; k < 4; ++k)
            if (k >= npx) f[2 * k] = f[2 * k - 2], f[2 * k + 1] = f[2 * k - 1];
#pragma unroll
        for (int k = 0; k < 4; ++k) U[R + k][j] = f[2 * k], V[R + k][j] = f[2 * k + 1];
    }
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int j = 0; j < NR; ++j) sanitise(U[c][j], V[c][j]);
    if constexpr (R == 1) {
        mednet::median9_quad(U, fu);
        mednet::median9_quad(V, fv);
    } else {
        mednet::median25_quad(U, fu);
        mednet::median25_quad(V, fv);
    }
    // step 3: a selected -0 leaves as +0; every other value keeps its bits (denormals are kept)
#pragma unroll
    for (int k = 0; k < 4; ++k) fu[k] = fu[k] + 0.0f, fv[k] = fv[k] + 0.0f;
}

// the march over one item, for one radius (the kernel below picks it: an item's radius is block-uniform)
template <int R> __device__ __forceinline__ void median_march(const MedianItem &P)
{
    const int w = P.w, h = P.h, wmax = w - 1, hmax = h - 1;
    const float scale = P.scale;
    const int sp = P.src_pitch;
    const bool warp = P.src != nullptr;
    const __amdgpu_buffer_rsrc_t rs_i = rsrc(P.src_flow, w * h * 8), rs_f = rsrc(P.dst_flow, w * h * 8);
    const __amdgpu_buffer_rsrc_t rs_s = rsrc(P.src, warp ? hmax * sp + w : 0);
    const float wmaxf = (float)wmax, hmaxf = (float)hmax;

#pragma nounroll
    for (int g = 0; g < kQuads; ++g) {
        int y, x0;
        if (!place_tile(w, h, g, y, x0)) break;
        const int npx = w - x0 < 4 ? w - x0 : 4;
        float fu[4], fv[4];
        median_quad<R>(rs_i, w, h, y, x0, npx, fu, fv);
        // the filtered quad leaves from registers
#include "quad_part_flow_store.h"
        if (warp) { // (block-uniform)
            // step 4: the warp of the quad by the vectors it holds
#include "quad_part_warp.h"
            store_quad_u8(P.dst + (size_t)y * (size_t)P.dst_pitch + (size_t)x0, out, npx, P.dwords);
        }
    }
}

// (One kernel for both radii has the 5x5 march's registers, 114 against the 3x3 march's 56.  A kernel per radius was measured: the
// 3x3 launch took the same time at 8 waves per SIMD as at 4)
__global__ __launch_bounds__(kThreads) void median_kernel(const MedianArgs A)
{
    const MedianItem &P = A.it[blockIdx.y];
    if (blockIdx.x >= tiles_across(P.w) * tiles_down(P.h)) return; // (the grid is the largest item's)
    if (P.radius == 2) median_march<2>(P);
    else median_march<1>(P);
}

} // namespace

extern "C" int ofx_flow_median(const ofx_median_desc *items, int n, void *stream)
{
    const char *who = "ofx_flow_median";
    OFX_REQUIRE(items != nullptr, "%s: items is null", who);
    OFX_REQUIRE(n >= 1 && n <= OFX_STREAM_MAX_BATCH, "%s: n = %d is not in 1 .. %d", who, n, OFX_STREAM_MAX_BATCH);
    static thread_local MedianArgs A;
    memset(&A, 0, sizeof A);
    unsigned blocks = 1;
    for (int i = 0; i < n; ++i) {
        const ofx_median_desc &d = items[i];
        OFX_REQUIRE(d.d_src_flow && d.d_dst_flow, "%s: item %d: d_src_flow or d_dst_flow is null", who, i);
        OFX_REQUIRE(d.w > 0 && d.h > 0, "%s: item %d: the size %d x %d must be positive", who, i, d.w, d.h);
        OFX_REQUIRE((size_t)d.w * (size_t)d.h < ((size_t)1 << 28), "%s: item %d: w * h = %d x %d is more than this build takes (2^28 pixels)", who, i, d.w, d.h);
        OFX_REQUIRE(d.radius == 1 || d.radius == 2, "%s: item %d: the radius %d is not 1 (3x3) or 2 (5x5)", who, i, d.radius);
        OFX_REQUIRE(__builtin_isfinite(d.scale), "%s: item %d: the scale must be finite", who, i);
        OFX_REQUIRE((((uintptr_t)d.d_src_flow | (uintptr_t)d.d_dst_flow) & 7) == 0, "%s: item %d: d_src_flow and d_dst_flow must be 8-byte aligned", who, i);
        const size_t fb = (size_t)d.w * (size_t)d.h * 8;
        const uintptr_t c0 = (uintptr_t)d.d_src_flow, c1 = c0 + fb, f0 = (uintptr_t)d.d_dst_flow, f1 = f0 + fb;
        OFX_REQUIRE(f1 <= c0 || c1 <= f0, "%s: item %d: d_dst_flow overlaps d_src_flow (a median is out of place)", who, i);
        OFX_REQUIRE((d.d_src != nullptr) == (d.d_dst != nullptr), "%s: item %d: d_src and d_dst go together (both, or neither for the flow alone)", who, i);
        MedianItem &P = A.it[i];
        P = MedianItem{d.d_src_flow, d.d_dst_flow, d.d_src, d.d_dst, d.w, d.h, d.radius, 0, 0, 0, d.scale};
        if (d.d_src) {
            OFX_TRY(check_warp_planes(who, "item", i, d.w, d.h, d.d_src, d.src_pitch, d.d_dst, d.dst_pitch, &P.dwords));
            P.src_pitch = d.src_pitch, P.dst_pitch = d.dst_pitch;
        }
        const unsigned b = tiles_across(d.w) * tiles_down(d.h);
        blocks = b > blocks ? b : blocks;
    }
    hipLaunchKernelGGL(median_kernel, dim3(blocks, n), dim3(kThreads), 0, ofx_stream(stream), A);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}
