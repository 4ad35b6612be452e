// The selection networks of the flow median (median.hip; the definition: "flow median" in include/ofx.h), written over a value
// type T and the three operations lo / hi / mid3 of the including unit, so that the kernel instantiates them on float (v_min_f32,
// v_max_f32, v_med3_f32) and tests/median_net_check.cpp on 64-bit words of 0-1 inputs (and / or): a network of min and max that
// selects the median of every 0-1 input selects it of every input (the zero-one principle), and 2^25 of them are quickly tried.
//
// A thread owns four adjacent pixels of a row, so its four windows share all but one column each.  A COLUMN of the window (2r + 1
// values, one component) is ordered once, for every output that contains it:
//   r = 1: the median of 9 from three ordered columns is med3(max of the three smallest, med3 of the three middles, min of the
//          three largest) -- the classic; six columns of three comparators, then six operations per output.
//   r = 2: the eight ordered columns c0 .. c7 are merged in pairs (Batcher's odd-even merge for any two lengths, Knuth 5.3.4):
//          P12, P34, P56 of 10, then Q = P12 + P34 and R = P34 + P56 of 20; output 0 is the median of c0 + Q, 1 of Q + c5, 2 of
//          c2 + R, 3 of R + c7.  The 13th smallest of an ordered A of 20 and an ordered B of 5 is
//              min(A13, max(A12, B1), max(A11, B2), max(A10, B3), max(A9, B4), max(A8, B5)),
//          because t has 13 values at or below it exactly when A_i <= t and B_j <= t for some i + j = 13.  Only A8 .. A13 of Q and
//          R are read: everything is straight-line code on registers, and the compiler drops the comparators nobody reads.
#pragma once

#ifndef MEDNET_FN
#define MEDNET_FN __device__ __forceinline__
#endif

namespace mednet {

template <class T> MEDNET_FN void cx(T &a, T &b)
{
    const T l = lo(a, b), h = hi(a, b);
    a = l, b = h;
}

template <class T> MEDNET_FN void sort3(T *c)
{
    cx(c[0], c[1]), cx(c[1], c[2]), cx(c[0], c[1]);
}

// nine comparators (the optimal count for five)
template <class T> MEDNET_FN void sort5(T *c)
{
    cx(c[0], c[1]), cx(c[3], c[4]), cx(c[2], c[4]), cx(c[2], c[3]), cx(c[1], c[4]);
    cx(c[0], c[3]), cx(c[0], c[2]), cx(c[1], c[3]), cx(c[1], c[2]);
}

// z[0 .. M + N) = the ordered union of the ordered x[0 .. M) and y[0 .. N); strides in elements
template <int M, int N, class T> struct Merge {
    static MEDNET_FN void run(const T *x, const T *y, T *z)
    {
        constexpr int MO = (M + 1) / 2, ME = M / 2, NO = (N + 1) / 2, NE = N / 2, NV = MO + NO, NW = ME + NE;
        T xo[MO > 0 ? MO : 1], xe[ME > 0 ? ME : 1], yo[NO > 0 ? NO : 1], ye[NE > 0 ? NE : 1], v[NV], w[NW > 0 ? NW : 1];
#pragma unroll
        for (int i = 0; i < M; ++i) {
            if (i & 1) xe[i >> 1] = x[i];
            else xo[i >> 1] = x[i];
        }
#pragma unroll
        for (int i = 0; i < N; ++i) {
            if (i & 1) ye[i >> 1] = y[i];
            else yo[i >> 1] = y[i];
        }
        Merge<MO, NO, T>::run(xo, yo, v);
        Merge<ME, NE, T>::run(xe, ye, w);
        // v1, then w_i against v_(i+1); what is left of v (none, one or two more than w) or of w (its last) follows as it is
        z[0] = v[0];
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            if (i + 1 < NV) {
                z[2 * i + 1] = lo(w[i], v[i + 1]);
                z[2 * i + 2] = hi(w[i], v[i + 1]);
            } else {
                z[2 * i + 1] = w[i];
            }
        }
#pragma unroll
        for (int i = NW + 1; i < NV; ++i) z[NW + i] = v[i];
    }
};
template <int N, class T> struct Merge<0, N, T> {
    static MEDNET_FN void run(const T *, const T *y, T *z)
    {
#pragma unroll
        for (int i = 0; i < N; ++i) z[i] = y[i];
    }
};
template <int M, class T> struct Merge<M, 0, T> {
    static MEDNET_FN void run(const T *x, const T *, T *z)
    {
#pragma unroll
        for (int i = 0; i < M; ++i) z[i] = x[i];
    }
};
template <class T> struct Merge<0, 0, T> {
    static MEDNET_FN void run(const T *, const T *, T *) {}
};
template <class T> struct Merge<1, 1, T> {
    static MEDNET_FN void run(const T *x, const T *y, T *z) { z[0] = lo(x[0], y[0]), z[1] = hi(x[0], y[0]); }
};

// the 13th smallest of the ordered a[0 .. 20) and the ordered b[0 .. 5)
template <class T> MEDNET_FN T select13(const T *a, const T *b)
{
    T m = a[12];
#pragma unroll
    for (int j = 0; j < 5; ++j) m = lo(m, hi(a[11 - j], b[j]));
    return m;
}

// r = 1: col[c][0 .. 3) = the window's column x0 - 1 + c, c = 0 .. 5 (any order inside a column); out[k] = the median of columns k .. k + 2
template <class T> MEDNET_FN void median9_quad(T col[6][3], T *out)
{
#pragma unroll
    for (int c = 0; c < 6; ++c) sort3(col[c]);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const T a = hi(hi(col[k][0], col[k + 1][0]), col[k + 2][0]);
        const T b = mid3(col[k][1], col[k + 1][1], col[k + 2][1]);
        const T c = lo(lo(col[k][2], col[k + 1][2]), col[k + 2][2]);
        out[k] = mid3(a, b, c);
    }
}

// r = 2: col[c][0 .. 5) = the window's column x0 - 2 + c, c = 0 .. 7; out[k] = the median of columns k .. k + 4
template <class T> MEDNET_FN void median25_quad(T col[8][5], T *out)
{
#pragma unroll
    for (int c = 0; c < 8; ++c) sort5(col[c]);
    T p12[10], p34[10], p56[10], q[20], r[20];
    Merge<5, 5, T>::run(col[1], col[2], p12);
    Merge<5, 5, T>::run(col[3], col[4], p34);
    Merge<5, 5, T>::run(col[5], col[6], p56);
    Merge<10, 10, T>::run(p12, p34, q);
    Merge<10, 10, T>::run(p34, p56, r);
    out[0] = select13(q, col[0]);
    out[1] = select13(q, col[5]);
    out[2] = select13(r, col[2]);
    out[3] = select13(r, col[7]);
}

} // namespace mednet
