// The stream pipeline's colour front end (main.cu:222-240): grayscale_avg of a colour frame, then the bilateral pre-filter with
// the grey image as its own source, in ONE launch over up to OFX_STREAM_MAX_BATCH frames (frame = blockIdx.z), writing the
// one-channel plane the pyramid stage reads.  The three-launch chain it replaces (ofx_grayscale_avg_3ch -> ofx_bilateral_3ch ->
// ofx_extract_ch0) moves 3 + 3 + 3 + 3 + 3 + 1 bytes per pixel; this reads the colour frame once and writes one byte per pixel.
//
// The two bilateral forms are bilateral_exact_own_kernel (bit-exact) and bilateral_lut_kernel (+-1 LSB) of primitives.hip with
// two changes each: the tile loader forms the channel average of the three dwords (four pixels) it reads instead of checking that
// the channels are equal -- so every tile is a grey tile and the colour path is gone -- and the store writes one byte per pixel
// (a lane's two pixels of a row as one 16-bit store).  Tap loop, tables, tap order and arithmetic are theirs (bilateral_common.h).
// A frame in grey mode is averaged only (main.cu:198-209: the first frame of the reference's loop is not filtered).
//
// The colour frame is read through a buffer resource of exactly (h - 1) * pitch + 3 * w bytes: a group of four pixels whose
// three dwords would reach past it is read byte by byte, in-frame bytes only.
#include <memory>

#include "bilateral_common.h"

namespace {

constexpr int kFrontMax = OFX_STREAM_MAX_BATCH;
enum : uint8_t { kSkip = 0, kGrey = 1, kFilter = 2 }; // what a launch does with a frame
struct FrontFrames {
    const uint8_t *src[kFrontMax]; // interleaved 3-channel u8, 4-byte aligned
    uint8_t *dst[kFrontMax];       // one-channel u8
    int spitch[kFrontMax], dpitch[kFrontMax];
    uint8_t mode[kFrontMax];
};

// OptFlowGpu.cu:47-60 (gray_kernel): (c0 + c1 + c2) / 3 in integers
__device__ __forceinline__ int avg3(uint32_t a, uint32_t b, uint32_t c) { return (int)(a + b + c) / 3; }

// the averages of pixels tx .. tx + 3 of row ty (the row is in the frame, tx + 3 >= 0 and tx < w); those outside [0, w) are left alone
__device__ __forceinline__ void load_grey4(const __amdgpu_buffer_rsrc_t rs, const uint8_t *img3, int sp, int bytes, int w, int tx, int ty,
                                           int (&g)[4])
{
    const int off = ty * sp + 3 * tx;
    if (off >= 0 && off + 12 <= bytes) { // twelve bytes = four pixels in three dwords (a pixel left of column 0 is the end of the row above)
        const uint32_t a = __builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0), b = __builtin_amdgcn_raw_buffer_load_b32(rs, off + 4, 0, 0),
                       c = __builtin_amdgcn_raw_buffer_load_b32(rs, off + 8, 0, 0);
        const int v[4] = {avg3(a & 0xffu, (a >> 8) & 0xffu, (a >> 16) & 0xffu), avg3(a >> 24, b & 0xffu, (b >> 8) & 0xffu),
                          avg3((b >> 16) & 0xffu, b >> 24, c & 0xffu), avg3((c >> 8) & 0xffu, (c >> 16) & 0xffu, c >> 24)};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (tx + k >= 0 && tx + k < w) g[k] = v[k];
    } else { // the frame's first and last bytes
        for (int k = 0; k < 4; ++k)
            if (tx + k >= 0 && tx + k < w) {
                const uint8_t *q = img3 + (size_t)ty * sp + 3 * (tx + k);
                g[k] = avg3(q[0], q[1], q[2]);
            }
    }
}

// grey mode: the averages of one tile, a pixel per thread
template <int TW, int TH, int NT>
__device__ void grey_tile(const uint8_t *img3, int sp, uint8_t *dst, int dp, int w, int h, int x0, int y0)
{
    for (int i = (int)threadIdx.x; i < TW * TH; i += NT) {
        const int x = x0 + i % TW, y = y0 + i / TW;
        if (x < w && y < h) {
            const uint8_t *q = img3 + (size_t)y * sp + 3 * x;
            dst[(size_t)y * dp + x] = (uint8_t)avg3(q[0], q[1], q[2]);
        }
    }
}

// bilateral_exact_own_kernel on the averages of a colour frame
template <int WW>
__global__ __launch_bounds__(kExThreads) void frontend_exact_kernel(const FrontFrames F, int w, int h, const BilateralArg B)
{
    const int f = (int)blockIdx.z, mode = F.mode[f];
    if (mode == kSkip) return;
    const uint8_t *img3 = F.src[f];
    uint8_t *dst = F.dst[f];
    const int sp = F.spitch[f], dp = F.dpitch[f];
    const int tid = (int)threadIdx.x, x0 = (int)blockIdx.x * kExTileW, y0 = (int)blockIdx.y * kExTileH;
    if (mode == kGrey) {
        grey_tile<kExTileW, kExTileH, kExThreads>(img3, sp, dst, dp, w, h, x0, y0);
        return;
    }
    constexpr int R = WW >> 1, TW = kExTileW + 2 * R, NG = (TW + 3) / 4, TWP = NG * 4, ROWS = kExTileH + 2 * R;
    __shared__ __attribute__((aligned(16))) double lut[kBilLut];
    __shared__ __attribute__((aligned(16))) int gt[ROWS * TWP]; // grey value, or kBilSentinel
    const int bytes = (h - 1) * sp + 3 * w; // (below 2 GB: ofx_frontend_run)
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(img3), 0, bytes, 0x00027000);
    for (int i = tid; i < kBilLut; i += kExThreads) {
        const int d = i - 255; // signed grey difference
        lut[i] = (d >= -255 && d <= 255) ? B.range[d < 0 ? -d : d] : 0.0;
    }
    for (int i = tid; i < ROWS * NG; i += kExThreads) {
        const int gr = i / NG, gc = i - gr * NG, ty = y0 - R + gr, tx = x0 - R + 4 * gc;
        int g[4] = {kBilSentinel, kBilSentinel, kBilSentinel, kBilSentinel};
        if (ty >= 0 && ty < h && tx + 3 >= 0 && tx < w) load_grey4(rs, img3, sp, bytes, w, tx, ty, g);
        *reinterpret_cast<int4 *>(gt + gr * TWP + 4 * gc) = int4{g[0], g[1], g[2], g[3]};
    }
    __syncthreads();
    const int lane = tid & 63, wv = tid >> 6;
    const uint8_t *lut_b = reinterpret_cast<const uint8_t *>(lut);
#pragma unroll 1
    for (int pr = 0; pr < 2; ++pr) {
        const int ly = 4 * wv + 2 * pr; // output rows ly, ly + 1 of the tile
        const int g00 = gt[(ly + R) * TWP + 2 * lane + R], g01 = gt[(ly + R) * TWP + 2 * lane + 1 + R], g10 = gt[(ly + 1 + R) * TWP + 2 * lane + R],
                  g11 = gt[(ly + 1 + R) * TWP + 2 * lane + 1 + R];
        // byte offset of table entry (g - g_0 + 255) = 8 g + base
        const int b00 = 8 * (255 - g00), b01 = 8 * (255 - g01), b10 = 8 * (255 - g10), b11 = 8 * (255 - g11);
        double acc0[4] = {0.0, 0.0, 0.0, 0.0}, acc1[4] = {0.0, 0.0, 0.0, 0.0}; // per output row: wsum A, a A, wsum B, a B
#pragma unroll 1
        for (int t = 0; t <= WW; ++t) { // tile row ly + t: tap row t of output row ly, tap row t - 1 of output row ly + 1
            const int2 *grow = reinterpret_cast<const int2 *>(gt + (ly + t) * TWP + 2 * lane);
            int v[WW + 1];
#pragma unroll
            for (int k = 0; k < (WW + 1) / 2; ++k) {
                const int2 q = grow[k];
                v[2 * k] = q.x;
                v[2 * k + 1] = q.y;
            }
            if (t < WW) exact_row_taps<WW>(v, b00, b01, lut_b, B.spatial + (t < WW ? t : 0) * WW, acc0);
            if (t > 0) exact_row_taps<WW>(v, b10, b11, lut_b, B.spatial + (t > 0 ? t - 1 : 0) * WW, acc1);
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int y = y0 + ly + r, xA = x0 + 2 * lane;
            if (y >= h || xA >= w) continue;
            const double(&acc)[4] = r ? acc1 : acc0;
            const uint32_t bA = (uint32_t)(uint8_t)(int)(acc[1] / acc[0]), bB = (uint32_t)(uint8_t)(int)(acc[3] / acc[2]);
            uint8_t *d = dst + (size_t)y * dp + xA;
            if (xA + 1 < w)
                *reinterpret_cast<uint16_t *>(d) = (uint16_t)(bA | (bB << 8)); // (unaligned two-byte stores are fine in global memory)
            else
                *d = (uint8_t)bA;
        }
    }
}

// bilateral_lut_kernel on the averages of a colour frame
template <int WW, int EVERY>
__global__ __launch_bounds__(kLutThreads) void frontend_lut_kernel(const FrontFrames F, int w, int h, const BilateralLutArg B)
{
    const int f = (int)blockIdx.z, mode = F.mode[f];
    if (mode == kSkip) return;
    const uint8_t *img3 = F.src[f];
    uint8_t *dst = F.dst[f];
    const int sp = F.spitch[f], dp = F.dpitch[f];
    const int tid = (int)threadIdx.x, x0 = (int)blockIdx.x * kLutTileW, y0 = (int)blockIdx.y * kLutTileH;
    if (mode == kGrey) {
        grey_tile<kLutTileW, kLutTileH, kLutThreads>(img3, sp, dst, dp, w, h, x0, y0);
        return;
    }
    constexpr int R = WW >> 1, TW = kLutTileW + 2 * R, NG = (TW + 3) / 4, TWP = NG * 4, ROWS = kLutTileH + 2 * R;
    __shared__ __attribute__((aligned(16))) float g4[ROWS * TWP]; // 4 * grey value, or kLutOutside
    __shared__ __attribute__((aligned(16))) float tab[WW * kLutEntries];
    const int bytes = (h - 1) * sp + 3 * w; // (below 2 GB: ofx_frontend_run)
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(img3), 0, bytes, 0x00027000);
    for (int i = tid; i < ROWS * NG; i += kLutThreads) {
        const int gr = i / NG, gc = i - gr * NG, ty = y0 - R + gr, tx = x0 - R + 4 * gc;
        int g[4] = {-256, -256, -256, -256}; // (4 * -256 = kLutOutside)
        if (ty >= 0 && ty < h && tx + 3 >= 0 && tx < w) load_grey4(rs, img3, sp, bytes, w, tx, ty, g);
        *reinterpret_cast<float4 *>(g4 + gr * TWP + 4 * gc) = float4{4.0f * (float)g[0], 4.0f * (float)g[1], 4.0f * (float)g[2], 4.0f * (float)g[3]};
    }
    {
        const float rg = tid < 256 ? B.range[tid] : 0.0f; // 512 threads: one entry each, times every column's a_n
#pragma unroll
        for (int n = 0; n < WW; ++n) tab[n * kLutEntries + tid] = B.row[n] * rg;
    }
    __syncthreads();
    const int lane = tid & 63, wv = tid >> 6;
    const char *tabb = reinterpret_cast<const char *>(tab);
#pragma unroll 1
    for (int pr = 0; pr < 2; ++pr) {
        const int ly = 4 * wv + 2 * pr; // output rows ly, ly + 1 of the tile
        const float2 c0 = *reinterpret_cast<const float2 *>(g4 + (ly + R) * TWP + 2 * lane + R - (R & 1)),
                     c0b = *reinterpret_cast<const float2 *>(g4 + (ly + R) * TWP + 2 * lane + R + (R & 1)),
                     c1 = *reinterpret_cast<const float2 *>(g4 + (ly + 1 + R) * TWP + 2 * lane + R - (R & 1)),
                     c1b = *reinterpret_cast<const float2 *>(g4 + (ly + 1 + R) * TWP + 2 * lane + R + (R & 1));
        const float g00 = (R & 1) ? c0.y : c0.x, g01 = (R & 1) ? c0b.x : c0.y, g10 = (R & 1) ? c1.y : c1.x, g11 = (R & 1) ? c1b.x : c1.y;
        float acc0[4] = {0.0f, 0.0f, 0.0f, 0.0f}, acc1[4] = {0.0f, 0.0f, 0.0f, 0.0f}; // per output row: wsum A, a A, wsum B, a B
#pragma unroll 1
        for (int t = 0; t <= WW; ++t) { // tile row ly + t: tap row t of output row ly, tap row t - 1 of output row ly + 1
            const float2 *grow = reinterpret_cast<const float2 *>(g4 + (ly + t) * TWP + 2 * lane); // (TWP and 2 * lane are even: 8-byte aligned)
            float v[WW + 1];
#pragma unroll
            for (int k = 0; k < (WW + 1) / 2; ++k) {
                const float2 q = grow[k];
                v[2 * k] = q.x;
                v[2 * k + 1] = q.y;
            }
            if (t < WW) lut_row_taps<WW, EVERY>(v, g00, g01, tabb, B.row[t < WW ? t : 0], acc0, B);
            if (t > 0) lut_row_taps<WW, EVERY>(v, g10, g11, tabb, B.row[t > 0 ? t - 1 : 0], acc1, B);
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int y = y0 + ly + r, xA = x0 + 2 * lane;
            if (y >= h || xA >= w) continue;
            const float(&acc)[4] = r ? acc1 : acc0;
            const float gA = r ? g10 : g00, gB = r ? g11 : g01;
            const uint32_t bA = (uint32_t)(int)(0.25f * (gA + acc[1] / acc[0])), bB = (uint32_t)(int)(0.25f * (gB + acc[3] / acc[2])); // g_0 + sum d w / sum w
            uint8_t *d = dst + (size_t)y * dp + xA;
            if (xA + 1 < w)
                *reinterpret_cast<uint16_t *>(d) = (uint16_t)(bA | (bB << 8));
            else
                *d = (uint8_t)bA;
        }
    }
}

template <int WW>
void launch_front_exact(const FrontFrames &F, int n, int w, int h, const BilateralArg &B, hipStream_t st)
{
    hipLaunchKernelGGL(frontend_exact_kernel<WW>, dim3(ofx_div_up(w, kExTileW), ofx_div_up(h, kExTileH), n), dim3(kExThreads), 0, st, F, w, h, B);
}

template <int WW>
void launch_front_lut(const FrontFrames &F, int n, int w, int h, const BilateralLutArg &B, bool computed_columns, hipStream_t st)
{
    // (launch_bilateral_lut's default split; a computed column needs the out-of-image taps' weight to underflow: sigma_b <= ~17)
    const dim3 grid(ofx_div_up(w, kLutTileW), ofx_div_up(h, kLutTileH), n);
    constexpr int split = OFX_LUT_SPLIT_DEFAULT;
    if (computed_columns)
        hipLaunchKernelGGL((frontend_lut_kernel<WW, split>), grid, dim3(kLutThreads), 0, st, F, w, h, B);
    else
        hipLaunchKernelGGL((frontend_lut_kernel<WW, split / 10 * 10>), grid, dim3(kLutThreads), 0, st, F, w, h, B);
}

} // namespace

struct ofx_frontend_tables {
    int window = 0; // 0: grey only
    double sigma_s = 0.0, sigma_b = 0.0;
    BilateralArg exact{};
    BilateralLutArg lut{};
    bool lut_ok = false; // the +-1 LSB kernel applies (separable mask, sigma_b <= 2e4 as ofx_bilateral_3ch_fast); else it runs exact
};

int ofx_frontend_tables_make(int window, double sigma_s, double sigma_b, ofx_frontend_tables **out)
{
    OFX_REQUIRE(out, "ofx_frontend_tables_make: null argument");
    if (window != 0 && (window < 3 || window > kMaxBilateral || !(window & 1))) {
        ofx_set_error("front end: window %d unsupported (square odd windows 3 .. %d)", window, kMaxBilateral);
        return OFX_E_UNSUPPORTED;
    }
    OFX_REQUIRE(window == 0 || (sigma_s > 0.0 && sigma_b > 0.0), "front end: sigma_s %g and sigma_b %g must be > 0", sigma_s, sigma_b);
    ofx_frontend_tables *t = new (std::nothrow) ofx_frontend_tables();
    OFX_REQUIRE(t, "ofx_frontend_tables_make: out of host memory");
    t->window = window;
    t->sigma_s = sigma_s;
    t->sigma_b = sigma_b;
    if (window) {
        bilateral_exact_tables(sigma_s, sigma_b, window, &t->exact);
        // the float tables as ofx_bilateral_3ch_fast builds them
        double sp[kMaxBilateral * kMaxBilateral];
        ofx_generate_gaussian_kernel(sigma_s, window, sp);
        t->lut_ok = sigma_b <= 2.0e4 && bilateral_sep_rows(sp, window, t->lut.row, t->lut.log2_col);
        bilateral_lut_range((float)(-M_LOG2E / (2.0 * sigma_b * sigma_b)), &t->lut);
    }
    *out = t;
    return OFX_OK;
}

void ofx_frontend_tables_free(ofx_frontend_tables *t) { delete t; }

int ofx_frontend_run(const ofx_frontend_tables *t, const uint8_t *const *src3, const int *src_pitch, uint8_t *const *dst, const int *dst_pitch,
                     const int *modes, int n, int w, int h, hipStream_t st)
{
    OFX_REQUIRE(t && src3 && src_pitch && dst && dst_pitch && modes, "front end: null argument");
    OFX_REQUIRE(n >= 1 && n <= kFrontMax && w > 0 && h > 0, "front end: %d frames of %dx%d (1 .. %d frames)", n, w, h, kFrontMax);
    bool any_exact = false, any_fast = false, any_grey = false;
    for (int i = 0; i < n; ++i) {
        OFX_REQUIRE(src3[i] && dst[i], "front end: frame %d: null pointer", i);
        OFX_REQUIRE(((uintptr_t)src3[i] & 3) == 0, "front end: frame %d: the colour frame must be 4-byte aligned", i);
        OFX_REQUIRE(src_pitch[i] >= 3 * w && dst_pitch[i] >= w, "front end: frame %d: pitches %d / %d below 3 * %d / %d bytes", i, src_pitch[i],
                    dst_pitch[i], w, w);
        if ((long long)(h - 1) * src_pitch[i] + 3ll * w >= (1ll << 31) || (long long)h * dst_pitch[i] >= (1ll << 31)) {
            ofx_set_error("front end: frame %d: 2 GB or more per frame", i);
            return OFX_E_UNSUPPORTED;
        }
        OFX_REQUIRE(modes[i] == OFX_FRONTEND_GREY || modes[i] == OFX_FRONTEND_BILATERAL || modes[i] == OFX_FRONTEND_BILATERAL_FAST,
                    "front end: frame %d: mode %d (OFX_FRONTEND_GREY / _BILATERAL / _BILATERAL_FAST)", i, modes[i]);
        const bool fast = modes[i] == OFX_FRONTEND_BILATERAL_FAST && t->lut_ok;
        any_grey |= modes[i] == OFX_FRONTEND_GREY;
        any_fast |= fast;
        any_exact |= modes[i] != OFX_FRONTEND_GREY && !fast;
    }
    if ((any_exact || any_fast) && t->window == 0) {
        ofx_set_error("front end: a bilateral frame needs a window (3 .. %d)", kMaxBilateral);
        return OFX_E_UNSUPPORTED;
    }
    FrontFrames F{};
    for (int i = 0; i < n; ++i) {
        F.src[i] = src3[i];
        F.dst[i] = dst[i];
        F.spitch[i] = src_pitch[i];
        F.dpitch[i] = dst_pitch[i];
    }
    // one launch per arithmetic in the call (one in the stream pipeline: a session uses one), grey frames with the first
    if (any_fast) {
        for (int i = 0; i < n; ++i) F.mode[i] = modes[i] == OFX_FRONTEND_GREY ? kGrey : (modes[i] == OFX_FRONTEND_BILATERAL_FAST && t->lut_ok) ? kFilter : kSkip;
        const bool computed = (double)t->lut.c * 65536.0 <= -150.0;
        switch (t->window) {
        case 3: launch_front_lut<3>(F, n, w, h, t->lut, computed, st); break;
        case 5: launch_front_lut<5>(F, n, w, h, t->lut, computed, st); break;
        case 7: launch_front_lut<7>(F, n, w, h, t->lut, computed, st); break;
        case 9: launch_front_lut<9>(F, n, w, h, t->lut, computed, st); break;
        case 11: launch_front_lut<11>(F, n, w, h, t->lut, computed, st); break;
        default: launch_front_lut<13>(F, n, w, h, t->lut, computed, st); break;
        }
        OFX_HIP(hipGetLastError());
    }
    if (any_exact || (any_grey && !any_fast)) {
        for (int i = 0; i < n; ++i) {
            const bool fast = modes[i] == OFX_FRONTEND_BILATERAL_FAST && t->lut_ok;
            F.mode[i] = modes[i] == OFX_FRONTEND_GREY ? (any_fast ? kSkip : kGrey) : fast ? kSkip : kFilter;
        }
        switch (t->window) {
        case 0: // (grey frames only: no bilateral tile is ever run)
        case 3: launch_front_exact<3>(F, n, w, h, t->exact, st); break;
        case 5: launch_front_exact<5>(F, n, w, h, t->exact, st); break;
        case 7: launch_front_exact<7>(F, n, w, h, t->exact, st); break;
        case 9: launch_front_exact<9>(F, n, w, h, t->exact, st); break;
        case 11: launch_front_exact<11>(F, n, w, h, t->exact, st); break;
        default: launch_front_exact<13>(F, n, w, h, t->exact, st); break;
        }
        OFX_HIP(hipGetLastError());
    }
    return OFX_OK;
}

extern "C" int ofx_frontend_1ch(const uint8_t *const *d_src3, const int *src_pitches, int src_pitch0, uint8_t *const *d_dst, const int *dst_pitches,
                                int dst_pitch0, int n, int w, int h, const int *modes, int mode0, int window, double sigma_s, double sigma_b,
                                void *stream)
{
    OFX_REQUIRE(d_src3 && d_dst, "ofx_frontend_1ch: null argument");
    OFX_REQUIRE(n >= 1 && n <= kFrontMax, "ofx_frontend_1ch: %d frames (1 .. %d)", n, kFrontMax);
    int sp[kFrontMax], dp[kFrontMax], md[kFrontMax];
    bool filter = false;
    for (int i = 0; i < n; ++i) {
        sp[i] = src_pitches ? src_pitches[i] : src_pitch0;
        dp[i] = dst_pitches ? dst_pitches[i] : dst_pitch0;
        md[i] = modes ? modes[i] : mode0;
        filter |= md[i] != OFX_FRONTEND_GREY;
    }
    // the tables of the last (window, sigma_s, sigma_b) a thread asked for are kept
    static thread_local std::unique_ptr<ofx_frontend_tables> cache;
    const int win = filter ? window : 0;
    if (!cache || cache->window != win || (win && (cache->sigma_s != sigma_s || cache->sigma_b != sigma_b))) {
        ofx_frontend_tables *t = nullptr;
        OFX_TRY(ofx_frontend_tables_make(win, sigma_s, sigma_b, &t));
        cache.reset(t);
    }
    return ofx_frontend_run(cache.get(), d_src3, sp, d_dst, dp, md, n, w, h, ofx_stream(stream));
}
