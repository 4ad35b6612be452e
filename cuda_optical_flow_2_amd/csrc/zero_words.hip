// The zeroing of a call's counters (stats slots, d_outside, d_counts) on its stream, as a launch of the library's own.
// It was hipMemsetAsync.  Recorded into a graph, a memset node of 32, 64 or 192 bytes wrote other values than zero at a replay
// that came after other copies, fills or memsets of the process (tests/test_gpu_graph_capture.py: the stats of ofx_texture_features
// at the second replay, of the quad stages at a replay after live calls), while every kernel node replayed as it was recorded: a
// kernel's arguments travel by value inside its node.  So the counters are zeroed by a kernel, live and captured alike.
#include "ofx_internal.h"

namespace {

constexpr unsigned kThreads = 256;

__global__ __launch_bounds__(kThreads) void zero_words_kernel(unsigned long long *words, unsigned n)
{
    const unsigned i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n) words[i] = 0ull;
}

} // namespace

int ofx_zero_words(void *d_words, size_t words, hipStream_t st)
{
    if (words == 0) return OFX_OK;
    OFX_REQUIRE(d_words != nullptr && ((uintptr_t)d_words & 7) == 0 && words <= (size_t)1 << 30, "ofx_zero_words: %zu words at %p", words, d_words);
    hipLaunchKernelGGL(zero_words_kernel, dim3((unsigned)((words + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, static_cast<unsigned long long *>(d_words),
                       (unsigned)words);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}
