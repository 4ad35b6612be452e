// A TEXTUAL part of the frame interpolation kernels (interp_kernel, interp3_kernel): #include it as the last thing in the kernel
// (why text: interp_part_prologue.h).  No include guard.
//
// The per-time block reduction of the counts: quad_stage.h's rule, once per time and all times under ONE barrier.  A thread's
// packed counter of time ti (8 bits per class: at most 16 pixels a thread) is unpacked into three sums; thread 4 * ti + c then owns
// word c of time ti's four-word slot.
//
// Reads   stats, nt, w, h and the LDS arrays cnt, red of interp_part_prologue.h
// Defines nothing that outlives it; it returns from the kernel where the pair has no stats
if (!stats) return; // (block-uniform)
for (int ti = 0; ti < nt; ++ti) {
    const uint32_t pk = cnt[ti][threadIdx.x];
    uint32_t n1 = pk & 0xffu, n2 = (pk >> 8) & 0xffu, n3 = (pk >> 16) & 0xffu;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        n1 += __shfl_xor(n1, o);
        n2 += __shfl_xor(n2, o);
        n3 += __shfl_xor(n3, o);
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][ti][0] = n1, red[threadIdx.x >> 6][ti][1] = n2, red[threadIdx.x >> 6][ti][2] = n3;
}
__syncthreads();
const int ti = threadIdx.x >> 2, c = threadIdx.x & 3; // thread 4 * ti + c: word c of time ti
if (ti < nt) {
    if (c) {
        unsigned long long s = 0;
#pragma unroll
        for (int i = 0; i < kThreads / 64; ++i) s += red[i][ti][c - 1];
        if (s) atomicAdd(stats + 4 * ti + c, s);
    } else if (blockIdx.x == 0) {
        atomicAdd(stats + 4 * ti, (unsigned long long)w * (unsigned long long)h);
    }
}
