// mgk_tail_dev.hpp -- what the kernels that keep the tail of the hierarchy in the LDS of ONE workgroup share (k_tail, k_tail_cheby, k_tail_fmg in
// mgk_tail.hip; k_tail_line in mgk_line_tail.hip): the index of a point in an (n+2)^DIM array, the deal of a level's points over the lanes,
// and the two transfers.  One definition of their arithmetic: every tail kernel restricts and prolongs with the same operations in the same order.
#pragma once
#include "mgk_dev.hpp"

#define MGK_TAIL_MAXLEV 8
// mgk_debug_tail_stamps (mgk_tail.hip): where the tail kernels this thread launches deposit their clock pairs; null in production
extern thread_local long long *g_tail_stamps;

template <typename T, int DIM>
__device__ __forceinline__ int tail_idx(int m, int k, int i, int j) {      // (k,i,j) interior coordinates -> index in an (n+2)^DIM array
    return (DIM == 3) ? ((k + 1) * m + (i + 1)) * m + (j + 1) : (i + 1) * m + (j + 1);
}
// Every interior point (k, i, j) of an n^DIM level once, dealt over the lanes of the workgroup.  With n + 1 a power of two (every level of
// a hierarchy with npts = 2^k + 1) the coordinates are shifts and masks of the lane number instead of two divisions and two remainders
// by n (~70 of the ~100 vector instructions per point; round 3, under rocprofv3: k_tail<double, 3> 43 -> 33 us, <double, 2> 45 -> 42 us).
// Which lane evaluates a point does not change its value.  What bounds the kernel (tools/tail_phases.py, stamps at every barrier): a step on
// a tiny level costs 0.36 us (850 clocks at 2.4 GHz: scalar loads of the level's constants, LDS round trip, the dependent fp64 chain, the
// barrier), a sweep of the largest level 1.7-2.3 us -- the instruction and LDS throughput of ONE CU for 4 points per lane (evaluating the
// four points of a lane before storing any of them, so that their latencies overlap, changed nothing: it is throughput, not latency).
template <int DIM, typename F>
__device__ __forceinline__ void tail_points(int n, F &&f) {
    const int t = threadIdx.x, B = blockDim.x;
    const int lg = 31 - __clz(n + 1);
    if (((n + 1) & n) == 0 && (B >> (DIM == 3 ? 2 * lg : lg)) >= 1) {
        const int j = t & n;
        if (DIM == 2) {
            const int step = B >> lg;
            if (j < n) for (int i = t >> lg; i < n; i += step) f(0, i, j);
        } else {
            const int i = (t >> lg) & n, step = B >> (2 * lg);
            if (j < n && i < n) for (int k = t >> (2 * lg); k < n; k += step) f(k, i, j);
        }
    } else {
        const int N = (DIM == 3) ? n * n * n : n * n;
        for (int p = t; p < N; p += B) f((DIM == 3) ? p / (n * n) : 0, (p / n) % n, p % n);
    }
}
// bc = R r (k_restrict: ascending fine index (dk, di, dj), weights w1[dk]*w2[di][dj])
template <typename T, int DIM>
__device__ void tail_restrict(int nf, int nc, const T *r, T *bc) {
    const int mf = nf + 2, mc = nc + 2;
    const T w2[3][3] = {{(T)0.0625, (T)0.125, (T)0.0625}, {(T)0.125, (T)0.25, (T)0.125}, {(T)0.0625, (T)0.125, (T)0.0625}};
    const T w1[3] = {(T)0.25, (T)0.5, (T)0.25};
    tail_points<DIM>(nc, [&](int kc, int ic, int jc) {
        T sum = (T)0;
        if (DIM == 3) {
#pragma unroll
            for (int dk = 0; dk < 3; dk++)
#pragma unroll
                for (int di = 0; di < 3; di++) {
                    const T *row = r + tail_idx<T, DIM>(mf, 2 * kc + dk, 2 * ic + di, 2 * jc);
                    sum += (w1[dk] * w2[di][0]) * row[0];
                    sum += (w1[dk] * w2[di][1]) * row[1];
                    sum += (w1[dk] * w2[di][2]) * row[2];
                }
        } else {
#pragma unroll
            for (int di = 0; di < 3; di++) {
                const T *row = r + tail_idx<T, DIM>(mf, 0, 2 * ic + di, 2 * jc);
                sum += w2[di][0] * row[0];
                sum += w2[di][1] * row[1];
                sum += w2[di][2] * row[2];
            }
        }
        bc[tail_idx<T, DIM>(mc, kc, ic, jc)] = sum;
    });
}
// uf += P uc (k_prolong_add / prolong_one: parents in ascending coarse index, weight wk*(wi*wj) each)
template <typename T, int DIM>
__device__ void tail_prolong_add(int nf, int nc, const T *uc, T *uf) {
    const int mf = nf + 2, mc = nc + 2;
    tail_points<DIM>(nf, [&](int k3, int i, int x) {
        const int k = (DIM == 3) ? k3 : 1;
        const int iodd = i & 1, kodd = k & 1, xodd = x & 1;
        const int ic0 = iodd ? (i - 1) / 2 : i / 2 - 1, nic = iodd ? 1 : 2;
        const int kc0 = (DIM == 3) ? (kodd ? (k - 1) / 2 : k / 2 - 1) : 0, nkc = (DIM == 3) ? (kodd ? 1 : 2) : 1;
        const int jc0 = xodd ? (x - 1) / 2 : x / 2 - 1, njc = xodd ? 1 : 2;
        const T wi = iodd ? (T)1 : (T)0.5, wk = (DIM == 3) ? (kodd ? (T)1 : (T)0.5) : (T)1, wj = xodd ? (T)1 : (T)0.5;
        const T w = (DIM == 3) ? wk * (wi * wj) : wi * wj;
        T s = (T)0;
        for (int qk = 0; qk < nkc; qk++)
            for (int qi = 0; qi < nic; qi++)
                for (int qj = 0; qj < njc; qj++) s += w * uc[tail_idx<T, DIM>(mc, kc0 + qk, ic0 + qi, jc0 + qj)];
        const int q = tail_idx<T, DIM>(mf, (DIM == 3) ? k : 0, i, x);
        uf[q] = uf[q] + s;
    });
}
