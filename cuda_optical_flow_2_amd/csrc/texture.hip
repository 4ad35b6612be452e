// Texture strength and feature selection (ofx_texture_features, ofx_compact_features).  The definition is the comment block
// "texture strength and feature selection" in include/ofx.h; DESIGN.md section 4.16 has the choices and the times.
//
// STRENGTH, one launch, blockIdx.y = the item.  A block of 256 threads owns a tile of kTile derivative columns and marches down a
// strip of kStrip output rows; thread t owns derivative column x0 - R + t, and the columns R .. kTile - 1 - R of the tile are
// output columns.  Per step one derivative row: the thread loads the three pixels of the next image row around its column (taps
// outside the image read as 0, which is what "skipped" means for a sum), forms Ix and Iy of its column from the 3 x 3 pixels it
// holds, and adds the three products to its column's vertical running sums; the row that leaves the window is subtracted again,
// its (Ix, Iy) come back as one packed dword from a ring in LDS that only the owning thread ever touches.  A derivative position
// outside the image contributes 0: that is the window clipped at the image.  Once the window is full the column sums go to LDS
// (two buffers, one barrier per row), every output thread adds the 2R + 1 columns around its own, all of them the block's, and
// step 2 of the definition runs in fp64.  Everything before that is exact integer arithmetic below 2^31.
//
// Traffic: the three byte loads of a step are the neighbours' too and come from the vector cache; a plane is read from memory
// once plus (2R + 2) / kStrip of its rows and 2R + 2 of every kTile columns.  Every tap goes through a buffer resource of exactly
// (h - 1) * pitch + w bytes, and a tap outside the image gets the offset kNowhere beyond it: nothing is read outside the plane.
//
// SELECTION, one launch, blockIdx.y = the item.  A block owns a group of whole cells (kGroup pixels across and down, at least
// one cell), tests every pixel of them (border, threshold, the 8-neighbour rule) and sends each candidate's key -- the strength's
// bits above the inverted pixel index -- to a 64-bit maximum in LDS, one word per cell: the largest strength wins, among equal
// ones the smallest index, in whatever order the candidates arrive.  A block takes its groups in turn (at most kSelectBlocks blocks
// per item) and sends its counts -- integer sums -- by three 64-bit atomic adds when it is done.  The neighbours are read at clamped
// positions, four rows of a wave in flight together: the launch is bound by latency.
//
// COMPACTION, one block: a ballot scan over the cells in raster order.
#include <string.h>

#include "quad_stage.h" // (for the buffer resource only: nothing here marches in quads)

namespace {

constexpr int kThreads = 256;
constexpr int kTile = kThreads;             // derivative columns of a block; kTile - 2R of them are output columns
constexpr int kStrip = 64;                  // output rows of a block
constexpr int kMaxR = 11;
constexpr uint32_t kNowhere = 0x80000000u;  // a buffer offset beyond every plane (a plane is below 2^31 bytes): loads 0
constexpr int kGroup = 64;                  // selection: a block's cells span about this many pixels each way
constexpr int kMaxGroupCells = (kGroup / 4) * (kGroup / 4);
constexpr unsigned kSelectBlocks = 256;     // selection: at most this many blocks per item; a block takes its groups in turn

struct TexItem {
    const uint8_t *plane;
    float *strength;
    int32_t *cells;
    float *cell_strength;
    unsigned long long *stats;
    int pitch, w, h, spitch, cell, border;
    float min_strength;
};
struct TexArgs {
    TexItem it[OFX_STREAM_MAX_BATCH];
};

__host__ __device__ inline int tile_out(int r) { return kTile - 2 * r; }
__host__ __device__ inline unsigned strength_blocks(int w, int h, int r)
{
    return (unsigned)((w + tile_out(r) - 1) / tile_out(r)) * (unsigned)((h + kStrip - 1) / kStrip);
}
// selection: cells per group side, groups across / down
__host__ __device__ inline int group_cells(int c) { return c >= kGroup ? 1 : kGroup / c; }
__host__ __device__ inline int cells_across(int n, int c) { return (n + c - 1) / c; }
__host__ __device__ inline unsigned select_groups(int w, int h, int c)
{
    const int g = group_cells(c);
    return (unsigned)((cells_across(w, c) + g - 1) / g) * (unsigned)((cells_across(h, c) + g - 1) / g);
}

using quad::rsrc;

// step 2 and 3 of the definition (the build has -ffp-contract=off: nothing below fuses)
__device__ __forceinline__ float strength_of(int sxx, int syy, int sxy)
{
    const double tr = (double)(sxx + syy), d = (double)(sxx - syy), b = (double)sxy;
    const double q = d * d;
    const double p2 = b * b;
    const double p4 = 4.0 * p2;
    const double r = q + p4;
    const double s = __dsqrt_rn(r);
    const double m = tr - s;
    const double lam = 0.5 * m;
    return lam > 0.0 ? (float)lam : 0.0f;
}

template <int R> __global__ __launch_bounds__(kThreads) void strength_kernel(const TexArgs A)
{
    constexpr int W = 2 * R + 1, OUT_W = kTile - 2 * R;
    __shared__ uint32_t ring[W][kThreads];        // (Ix, Iy) of the window's rows, packed; column t is thread t's alone
    __shared__ int colsum[2][3][kThreads];        // the column sums of a row, two buffers

    const TexItem &P = A.it[blockIdx.y];
    const int w = P.w, h = P.h, pitch = P.pitch;
    const unsigned across = (unsigned)((w + OUT_W - 1) / OUT_W);
    if (blockIdx.x >= across * (unsigned)((h + kStrip - 1) / kStrip)) return; // (the grid is the largest item's; block-uniform)
    const int ty = (int)(blockIdx.x / across), tx = (int)(blockIdx.x - (unsigned)ty * across);
    const int t = (int)threadIdx.x;
    const int cx = tx * OUT_W - R + t; // this thread's derivative column; its output column when R <= t < kTile - R
    const int ys = ty * kStrip, ye = min(ys + kStrip, h);
    const __amdgpu_buffer_rsrc_t rs = rsrc(P.plane, (h - 1) * pitch + w);

    const bool in_x = cx >= 0 && cx < w;
    const bool ok_l = cx - 1 >= 0 && cx - 1 < w, ok_r = cx + 1 >= 0 && cx + 1 < w;
    // the three pixels of image row y around column cx; 0 outside the image.  Offsets by arithmetic alone -- a column or a row
    // outside the image sets the offset's top bit, which puts it beyond the resource -- so that no load sits behind a branch
    const uint32_t col_l = ok_l ? (uint32_t)(cx - 1) : kNowhere, col_m = in_x ? (uint32_t)cx : kNowhere, col_r = ok_r ? (uint32_t)(cx + 1) : kNowhere;
    auto load_row = [&](int y, int &a, int &b, int &c) {
        const uint32_t o = (uint32_t)min(max(y, 0), h - 1) * (uint32_t)pitch, out = y >= 0 && y < h ? 0u : kNowhere;
        a = (int)__builtin_amdgcn_raw_buffer_load_b8(rs, (o + col_l) | out, 0, 0);
        b = (int)__builtin_amdgcn_raw_buffer_load_b8(rs, (o + col_m) | out, 0, 0);
        c = (int)__builtin_amdgcn_raw_buffer_load_b8(rs, (o + col_r) | out, 0, 0);
    };

    int a0, a1, a2, b0, b1, b2, c0, c1, c2; // pixel rows yd - 1 (a), yd (b), yd + 1 (c) at columns cx - 1, cx, cx + 1
    const int yd0 = ys - R;                 // the first derivative row of the strip's first window
    load_row(yd0 - 1, a0, a1, a2);
    load_row(yd0, b0, b1, b2);
    int n0, n1, n2;                         // the row after: its loads stay in flight across a step
    load_row(yd0 + 1, n0, n1, n2);
    int vxx = 0, vyy = 0, vxy = 0;
    int slot = 0;
    const int steps = (ye - ys) + 2 * R;
#pragma nounroll
    for (int i = 0; i < steps; ++i) {
        const int yd = yd0 + i;
        c0 = n0, c1 = n1, c2 = n2;
        load_row(yd + 2, n0, n1, n2);
        int ix = (a2 + 2 * b2 + c2) - (a0 + 2 * b0 + c0);
        int iy = (c0 + 2 * c1 + c2) - (a0 + 2 * a1 + a2);
        const bool inside = in_x && yd >= 0 && yd < h; // the window is clipped at the image
        ix = inside ? ix : 0, iy = inside ? iy : 0;
        if (i >= W) {                                  // (uniform) the row that leaves the window
            const uint32_t old = ring[slot][t];
            const int ox = (int)(int16_t)(old & 0xffffu), oy = (int)(int16_t)(old >> 16);
            vxx -= __mul24(ox, ox), vyy -= __mul24(oy, oy), vxy -= __mul24(ox, oy);
        }
        ring[slot][t] = ((uint32_t)ix & 0xffffu) | ((uint32_t)iy << 16);
        slot = slot + 1 == W ? 0 : slot + 1;
        vxx += __mul24(ix, ix), vyy += __mul24(iy, iy), vxy += __mul24(ix, iy);
        a0 = b0, a1 = b1, a2 = b2, b0 = c0, b1 = c1, b2 = c2;
        if (i >= 2 * R) {                              // (uniform) the window of output row y = yd - R is full
            const int y = yd - R, buf = i & 1;
            colsum[buf][0][t] = vxx, colsum[buf][1][t] = vyy, colsum[buf][2][t] = vxy;
            __syncthreads(); // (the other buffer was read before the previous barrier: one barrier per row is enough)
            if (t >= R && t < kTile - R && cx < w) {
                int sxx = 0, syy = 0, sxy = 0;
#pragma unroll
                for (int k = -R; k <= R; ++k) sxx += colsum[buf][0][t + k], syy += colsum[buf][1][t + k], sxy += colsum[buf][2][t + k];
                P.strength[(size_t)y * (size_t)P.spitch + (size_t)cx] = strength_of(sxx, syy, sxy);
            }
        }
    }
}

// ---- selection ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void select_kernel(const TexArgs A)
{
    __shared__ unsigned long long best[kMaxGroupCells];
    __shared__ unsigned int count[3];

    const TexItem &P = A.it[blockIdx.y];
    if (P.cells == nullptr) return; // a strength-only item
    const int w = P.w, h = P.h, c = P.cell, b = P.border, sp = P.spitch;
    const int g = group_cells(c), ncx = cells_across(w, c), ncy = cells_across(h, c);
    const int gacross = (ncx + g - 1) / g;
    const unsigned groups = select_groups(w, h, c);
    const int t = (int)threadIdx.x;
    const float thr = P.min_strength;
    const float *R = P.strength;
    // a wave takes rows of the group, its lanes a row's pixels: no division per pixel (lx / c = lx * inv >> 16 is exact
    // for lx < 256 and 4 <= c <= 256, and a group is at most 256 pixels wide and high)
    const int lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const uint32_t inv = (65536u + (uint32_t)c - 1u) / (uint32_t)c;
    unsigned n_cand = 0, n_weak = 0, n_occ = 0; // this thread's counts over all the block's groups
    if (t < 3) count[t] = 0u;

    // the block's groups, one after the other (block-uniform bounds): its counts leave in three atomic adds per block, not per group
    for (unsigned grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const int gy = (int)grp / gacross, gx = (int)grp - gy * gacross;
        const int cx0 = gx * g, cy0 = gy * g;                             // the group's first cell
        const int gcx = min(g, ncx - cx0), gcy = min(g, ncy - cy0);       // its cells across and down
        const int px0 = cx0 * c, py0 = cy0 * c;
        const int pw = min(gcx * c, w - px0), ph = min(gcy * c, h - py0); // its pixels
        for (int i = t; i < gcx * gcy; i += kThreads) best[i] = 0ull;
        __syncthreads();
        // four rows of the wave (kThreads / 64 apart) are in flight together: their 36 loads, at clamped positions, are all issued
        // before the first is looked at (one row at a time the launch waited for memory: DESIGN.md section 4.16)
        constexpr int kRows = 4, kStep = kThreads / 64;
        for (int ly0 = wave; ly0 < ph; ly0 += kRows * kStep) {
            for (int lx = lane; lx < pw; lx += 64) {
                const int x = px0 + lx;
                const bool in_x = x >= b && x < w - b;
                float v[kRows], nb[kRows][8];
#pragma unroll
                for (int j = 0; j < kRows; ++j) {
                    const int y = min(py0 + ly0 + j * kStep, h - 1);
                    v[j] = R[(size_t)y * (size_t)sp + (size_t)x];
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const int dy = (k < 3) ? -1 : (k < 5 ? 0 : 1), dx = k < 3 ? k - 1 : (k == 3 ? -1 : (k == 4 ? 1 : k - 6));
                        nb[j][k] = R[(size_t)min(max(y + dy, 0), h - 1) * (size_t)sp + (size_t)min(max(x + dx, 0), w - 1)];
                    }
                }
#pragma unroll
                for (int j = 0; j < kRows; ++j) {
                    const int ly = ly0 + j * kStep, y = py0 + ly;
                    if (!(ly < ph && in_x && y >= b && y < h - b)) continue;
                    if (!(v[j] > thr)) {
                        ++n_weak;
                        continue;
                    }
                    bool top = true;
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const int dy = (k < 3) ? -1 : (k < 5 ? 0 : 1), dx = k < 3 ? k - 1 : (k == 3 ? -1 : (k == 4 ? 1 : k - 6));
                        const int xx = x + dx, yy = y + dy;
                        const bool out = xx < 0 || xx >= w || yy < 0 || yy >= h; // a neighbour outside the image is none
                        top = top && (out || (k < 4 ? v[j] > nb[j][k] : v[j] >= nb[j][k])); // k < 4: before it in raster order
                    }
                    if (!top) continue;
                    ++n_cand;
                    const unsigned long long key = ((unsigned long long)__float_as_uint(v[j]) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)(y * w + x));
                    atomicMax(&best[(int)(((uint32_t)ly * inv) >> 16) * gcx + (int)(((uint32_t)lx * inv) >> 16)], key);
                }
            }
        }
        __syncthreads();
        for (int i = t; i < gcx * gcy; i += kThreads) {
            const int cy = cy0 + i / gcx, cxx = cx0 + i % gcx;
            const unsigned long long key = best[i];
            const size_t ci = (size_t)cy * (size_t)ncx + (size_t)cxx;
            int fx = -1, fy = -1;
            float fs = 0.0f;
            if (key) {
                const uint32_t idx = 0xffffffffu - (uint32_t)key;
                fy = (int)(idx / (uint32_t)w), fx = (int)(idx - (uint32_t)fy * (uint32_t)w);
                fs = __uint_as_float((uint32_t)(key >> 32));
                ++n_occ;
            }
            P.cells[2 * ci] = fx, P.cells[2 * ci + 1] = fy;
            P.cell_strength[ci] = fs;
        }
        __syncthreads(); // (best is cleared again for the next group)
    }
    if (P.stats == nullptr) return;
    __syncthreads();     // (count is zero)
    if (n_occ) atomicAdd(&count[0], n_occ);
    if (n_cand) atomicAdd(&count[1], n_cand);
    if (n_weak) atomicAdd(&count[2], n_weak);
    __syncthreads();
    if (t < 3 && count[t]) atomicAdd(&P.stats[1 + t], (unsigned long long)count[t]); // (zeroed on the stream before the launch)
    if (t == 3 && blockIdx.x == 0) atomicAdd(&P.stats[0], (unsigned long long)ncx * (unsigned long long)ncy);
}

// ---- compaction ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void compact_kernel(const int32_t *cells, int n_cells, int max_points, float *points, int32_t *count)
{
    __shared__ int wave_n[kThreads / 64];
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    int base = 0; // occupied cells before this chunk (the same in every thread)
    for (int c0 = 0; c0 < n_cells; c0 += kThreads) {
        const int i = c0 + t;
        int x = -1, y = -1;
        if (i < n_cells) x = cells[2 * i], y = cells[2 * i + 1];
        const bool occ = x >= 0;
        const unsigned long long m = __ballot(occ);
        if (lane == 0) wave_n[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < kThreads / 64; ++k) {
            before += k < wave ? wave_n[k] : 0;
            total += wave_n[k];
        }
        const int pos = base + before + __popcll(m & ((1ull << lane) - 1ull));
        if (occ && pos < max_points) points[2 * pos] = (float)x, points[2 * pos + 1] = (float)y;
        base += total;
        __syncthreads();
    }
    if (t == 0) *count = base < max_points ? base : max_points;
}

template <int R> int launch_strength(const TexArgs &A, unsigned blocks, int n, hipStream_t st)
{
    hipLaunchKernelGGL(strength_kernel<R>, dim3(blocks, n), dim3(kThreads), 0, st, A);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}

} // namespace

extern "C" int ofx_texture_features(const ofx_texture_desc *items, int n, int window, void *stream)
{
    const char *who = "ofx_texture_features";
    OFX_REQUIRE(items != nullptr, "%s: items is null", who);
    OFX_REQUIRE(n >= 1 && n <= OFX_STREAM_MAX_BATCH, "%s: n = %d is not in 1 .. %d", who, n, OFX_STREAM_MAX_BATCH);
    OFX_REQUIRE((window & 1) == 1 && window >= 3 && window <= 2 * kMaxR + 1, "%s: the window %d is not odd and in 3 .. %d", who, window, 2 * kMaxR + 1);
    const int r = window >> 1;
    static thread_local TexArgs A;
    memset(&A, 0, sizeof A);
    unsigned blocks = 1, sel_blocks = 0;
    for (int i = 0; i < n; ++i) {
        const ofx_texture_desc &d = items[i];
        OFX_REQUIRE(d.d_plane && d.d_strength, "%s: item %d: d_plane or d_strength is null", who, i);
        OFX_REQUIRE(d.w > 0 && d.h > 0, "%s: item %d: the size %d x %d must be positive", who, i, d.w, d.h);
        OFX_REQUIRE((size_t)d.w * (size_t)d.h < ((size_t)1 << 28), "%s: item %d: w * h = %d x %d is more than this build takes (2^28 pixels)", who, i, d.w, d.h);
        OFX_REQUIRE(d.pitch >= d.w && (d.pitch & 3) == 0, "%s: item %d: the pitch %d is below the width %d or no multiple of 4", who, i, d.pitch, d.w);
        OFX_REQUIRE((size_t)d.h * (size_t)d.pitch < ((size_t)1 << 31), "%s: item %d: the pitch %d makes a plane of 2^31 bytes or more", who, i, d.pitch);
        OFX_REQUIRE(d.strength_pitch >= d.w, "%s: item %d: strength_pitch %d is below the width %d", who, i, d.strength_pitch, d.w);
        OFX_REQUIRE(((uintptr_t)d.d_plane & 3) == 0 && ((uintptr_t)d.d_strength & 3) == 0, "%s: item %d: d_plane and d_strength must be 4-byte aligned", who, i);
        OFX_REQUIRE((d.d_cells != nullptr) == (d.d_cell_strength != nullptr), "%s: item %d: d_cells and d_cell_strength go together (both, or neither for the strength alone)", who, i);
        OFX_REQUIRE(d.d_stats == nullptr || d.d_cells != nullptr, "%s: item %d: d_stats without d_cells", who, i);
        if (d.d_cells) {
            OFX_REQUIRE(((uintptr_t)d.d_cells & 3) == 0 && ((uintptr_t)d.d_cell_strength & 3) == 0 && ((uintptr_t)d.d_stats & 7) == 0,
                        "%s: item %d: d_cells and d_cell_strength must be 4-byte aligned, d_stats 8-byte aligned", who, i);
            OFX_REQUIRE(d.cell >= 4 && d.cell <= 256, "%s: item %d: the cell %d is not in 4 .. 256", who, i, d.cell);
            OFX_REQUIRE(d.border >= 0, "%s: item %d: the border %d is negative", who, i, d.border);
            OFX_REQUIRE(__builtin_isfinite(d.min_strength) && d.min_strength >= 0.0f, "%s: item %d: min_strength must be finite and not negative", who, i);
        }
        TexItem &P = A.it[i];
        P = TexItem{d.d_plane, d.d_strength, d.d_cells, d.d_cell_strength, reinterpret_cast<unsigned long long *>(d.d_stats),
                    d.pitch, d.w, d.h, d.strength_pitch, d.cell, d.border, d.min_strength};
        const unsigned bl = strength_blocks(d.w, d.h, r);
        blocks = bl > blocks ? bl : blocks;
        if (d.d_cells) {
            const unsigned sb = select_groups(d.w, d.h, d.cell);
            sel_blocks = sb > sel_blocks ? sb : sel_blocks;
        }
    }
    hipStream_t st = ofx_stream(stream);
    switch (r) {
    case 1: OFX_TRY(launch_strength<1>(A, blocks, n, st)); break;
    case 2: OFX_TRY(launch_strength<2>(A, blocks, n, st)); break;
    case 3: OFX_TRY(launch_strength<3>(A, blocks, n, st)); break;
    case 4: OFX_TRY(launch_strength<4>(A, blocks, n, st)); break;
    case 5: OFX_TRY(launch_strength<5>(A, blocks, n, st)); break;
    case 6: OFX_TRY(launch_strength<6>(A, blocks, n, st)); break;
    case 7: OFX_TRY(launch_strength<7>(A, blocks, n, st)); break;
    case 8: OFX_TRY(launch_strength<8>(A, blocks, n, st)); break;
    case 9: OFX_TRY(launch_strength<9>(A, blocks, n, st)); break;
    case 10: OFX_TRY(launch_strength<10>(A, blocks, n, st)); break;
    default: OFX_TRY(launch_strength<11>(A, blocks, n, st)); break;
    }
    if (sel_blocks) {
        for (int i = 0; i < n;) { // one zeroing launch per run of consecutive stats slots
            int e = i + 1;
            if (items[i].d_stats) {
                while (e < n && items[e].d_stats == items[i].d_stats + 4 * (e - i)) ++e;
                OFX_TRY(ofx_zero_words(items[i].d_stats, (size_t)(e - i) * 4, st));
            }
            i = e;
        }
        hipLaunchKernelGGL(select_kernel, dim3(sel_blocks < kSelectBlocks ? sel_blocks : kSelectBlocks, n), dim3(kThreads), 0, st, A);
        OFX_HIP(hipGetLastError());
    }
    return OFX_OK;
}

extern "C" int ofx_compact_features(const int32_t *d_cells, int n_cells, int max_points, float *d_points, int32_t *d_count, void *stream)
{
    const char *who = "ofx_compact_features";
    OFX_REQUIRE(d_cells && d_count, "%s: d_cells or d_count is null", who);
    OFX_REQUIRE(n_cells >= 1 && n_cells < (1 << 28), "%s: n_cells = %d is not in 1 .. 2^28 - 1", who, n_cells);
    OFX_REQUIRE(max_points >= 0, "%s: max_points = %d is negative", who, max_points);
    OFX_REQUIRE(d_points != nullptr || max_points == 0, "%s: d_points is null", who);
    OFX_REQUIRE((((uintptr_t)d_cells | (uintptr_t)d_points | (uintptr_t)d_count) & 3) == 0, "%s: the pointers must be 4-byte aligned", who);
    hipLaunchKernelGGL(compact_kernel, dim3(1), dim3(kThreads), 0, ofx_stream(stream), d_cells, n_cells, max_points, d_points, d_count);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}
