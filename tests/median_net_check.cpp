// The flow median's selection networks (cuda_optical_flow_2_amd/csrc/median_net.h) on every 0-1 input: a network of min and max
// that selects the median of every 0-1 input selects it of every input.  T is a 64-bit word of 64 inputs, min is AND, max is OR.
// For each of a quad's four outputs, the 9 (25) wires of its window take all 2^9 (2^25) values while the other wires hold 0, then 1.
// Prints "ok <inputs tried>" and returns 0, or says which output failed.  Built and run by tests/test_median_abi.py.
#include <stdint.h>
#include <stdio.h>

typedef uint64_t W;
static inline W lo(W a, W b) { return a & b; }
static inline W hi(W a, W b) { return a | b; }
static inline W mid3(W a, W b, W c) { return (a & b) | (a & c) | (b & c); }
#define MEDNET_FN inline
#include "median_net.h"

// wire j of input number 64 * word + bit holds bit j of that number
static W wire(int j, uint64_t word)
{
    static const W low[6] = {0xAAAAAAAAAAAAAAAAull, 0xCCCCCCCCCCCCCCCCull, 0xF0F0F0F0F0F0F0F0ull, 0xFF00FF00FF00FF00ull, 0xFFFF0000FFFF0000ull, 0xFFFFFFFF00000000ull};
    return j < 6 ? low[j] : ((word >> (j - 6)) & 1u ? ~(W)0 : (W)0);
}

template <int R> static long long check()
{
    constexpr int NR = 2 * R + 1, NC = 4 + 2 * R, NW = NR * NR;
    long long tried = 0;
    for (int k = 0; k < 4; ++k)
        for (int others = 0; others < 2; ++others) {
            const uint64_t words = NW > 6 ? (uint64_t)1 << (NW - 6) : 1;
            for (uint64_t word = 0; word < words; ++word) {
                W col[NC][NR], out[4], want = 0;
                for (int c = 0; c < NC; ++c)
                    for (int j = 0; j < NR; ++j) col[c][j] = c >= k && c < k + NR ? wire((c - k) * NR + j, word) : (others ? ~(W)0 : (W)0);
                for (int b = 0; b < 64; ++b)
                    if (__builtin_popcountll((64 * word + b) & (((uint64_t)1 << NW) - 1)) > NW / 2) want |= (W)1 << b;
                if (R == 1) mednet::median9_quad(reinterpret_cast<W(*)[3]>(col), out);
                else mednet::median25_quad(reinterpret_cast<W(*)[5]>(col), out);
                if (out[k] != want) {
                    printf("radius %d: output %d is not the median (inputs %llu .., the other wires %d)\n", R, k, (unsigned long long)(64 * word), others);
                    return -1;
                }
                tried += 64;
            }
        }
    return tried;
}

int main()
{
    const long long a = check<1>(), b = a < 0 ? -1 : check<2>();
    if (a < 0 || b < 0) return 1;
    printf("ok %lld\n", a + b);
    return 0;
}
