// cover_kernels.hip.h -- the cover separation of include/mipx_cover.h: one lifted cover cut from one point, one box and
// one row of the problem.
//
//   cover_separate  one workgroup of 256 threads (4 waves) per (point, row).  Threads stride the row's columns
//                   (coalesced reads of a_ij, x, l, u) and compact its binaries into LDS in column order: a ballot per
//                   wave and chunk of 256 columns, the 16 counts through LDS.  A row of k nonzeros costs k items from
//                   here on, whatever n is.  The two orders are produced by counting: an item's position is the number
//                   of keys below its own, every thread reading the keys from LDS at the same address (a broadcast),
//                   for at most 4 items of its own at a time; the orders are total, so there is no tie to surprise.
//                   A PREFIX SUM is 4 consecutive positions per thread, a shuffle scan in each wave and the waves'
//                   totals through LDS; the first position past the capacity is a workgroup minimum, not a serial
//                   walk.  Lifting counts the mu_h below each item's weight, again by broadcast reads.  The
//                   coefficients are scattered to a column-indexed LDS array, from which pi, pi0 and the efficacy
//                   follow in the BLOCK SUM order of mipx_mir.h.  About 40 KiB of LDS.  No atomics; the outputs are
//                   plain vector stores.  The first stage, the knapsack form up to the compacted items, is the device
//                   function cover_knapsack_form, which clique_graph (clique_kernels.hip.h) calls too.
//
// Products are not fused (the library is built with -ffp-contract=off); every sum runs in the order mipx_cover.h
// states, which tests/support/cover_reference.py follows bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace mipx {

constexpr int kCovNT = 256;        // threads per workgroup
constexpr int kCovMax = 1024;      // rows and columns at most
constexpr int kCovPer = kCovMax / kCovNT;   // items (or columns) per thread at most
constexpr double kCovMargin = 1e-9;         // relative margin of the cover test and of the lifting comparison
constexpr int kCovNone = 0x7fffffff;

struct CoverArgs {
    int m, n, n_int, R;
    double min_eff;
    const double *A, *b;              // the problem's rows A x >= b (m x n, row-major)
    const double *x, *l, *u;          // batch x n
    const int32_t *int_idx;           // the integer columns, n_int of them
    const int32_t *rows;              // nullable: R row indices (null: the m rows)
    double *pi, *pi0, *eff;           // batch x R x n, batch x R each
    int32_t *size, *status;           // batch x R
};

// The smallest of a value over the workgroup.  Called by every thread.
__device__ inline int cover_block_min(int v, int *red) {
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    __syncthreads();   // (the slots may still be read from the minimum before)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return min(min(red[0], red[1]), min(red[2], red[3]));
}

// PREFIX SUM of src[0..cnt-1]: P[k] is the prefix sum behind position 4 * tid + k.  Called by every thread.
__device__ inline void cover_prefix_sum(const double *src, int cnt, double (&P)[kCovPer], double *red) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < kCovPer; k++) {
        const int pos = kCovPer * tid + k;
        if (pos < cnt) t += src[pos];
        P[k] = t;
    }
    double inc = t;
    for (int off = 1; off < 64; off <<= 1) {
        const double below = __shfl_up(inc, off, 64);
        if (lane >= off) inc += below;
    }
    double exc = __shfl_up(inc, 1, 64);
    if (lane == 0) exc = 0.0;
    __syncthreads();   // (the slots may still be read from the sum before)
    if (lane == 63) red[wave] = inc;
    __syncthreads();
    const double T0 = red[0], T1 = red[1], T2 = red[2];
    const double base = wave == 0 ? 0.0 : wave == 1 ? T0 : wave == 2 ? T0 + T1 : (T0 + T1) + T2;
    const double start = base + exc;
#pragma unroll
    for (int k = 0; k < kCovPer; k++) P[k] = start + P[k];
}

// KNAPSACK FORM of one row (mipx_cover.h), shared by cover_separate and clique_graph (clique_kernels.hip.h): marks the
// integer columns in isint, compacts the row's items into wt, col (and key, where the caller has a point: x and key
// are null together) in column order, and returns their number; W is the capacity, skipped whether the row is skipped.
// Called by every thread; the arrays are LDS of kCovMax entries each, and the items are published behind the last barrier.
__device__ inline int cover_knapsack_form(int n, int n_int, const int32_t *int_idx, const double *ar, double bi,
                                          const double *x, const double *l, const double *u, double *wt, double *key,
                                          uint16_t *col, uint8_t *isint, double (*red)[kCovNT / 64],
                                          int (*cnt)[kCovNT / 64], int *sskip, double &W, bool &skipped) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double inf = __builtin_huge_val();
    for (int j = tid; j < kCovMax; j += kCovNT) isint[j] = 0;
    if (tid == 0) *sskip = 0;
    __syncthreads();
    for (int k = tid; k < n_int; k += kCovNT) isint[int_idx[k]] = 1;
    __syncthreads();

    // the columns, chunk c of a thread is column tid + 256 c; K; the binaries marked
    double kpart = 0.0, zero = 0.0;
    double cw[kCovPer], ck[kCovPer];       // the weight and the key of the item at this thread's chunk c
    bool cbin[kCovPer], ccomp[kCovPer];   // the column is an item; it is complemented
#pragma unroll
    for (int c = 0; c < kCovPer; c++) {
        const int j = tid + c * kCovNT;
        cbin[c] = false; ccomp[c] = false; cw[c] = 0.0; ck[c] = 0.0;
        if (j < n) {
            const double g = 0.0 - ar[j];
            if (g != 0.0) {
                const double lj = l[j], uj = u[j];
                const bool bin = isint[j] && uj < inf && floor(lj) == lj && floor(uj) == uj && uj - lj == 1.0;
                const double bnd = g > 0.0 ? lj : uj;
                if (!bin && !(bnd < inf)) {
                    *sskip = 1;
                } else {
                    kpart += g * bnd;
                    if (bin) {
                        cbin[c] = true; ccomp[c] = g < 0.0; cw[c] = fabs(g);
                        if (x) {
                            const double xj = x[j];
                            const double y = g > 0.0 ? xj - lj : uj - xj;
                            const double yc = y < 0.0 ? 0.0 : y > 1.0 ? 1.0 : y;
                            ck[c] = (1.0 - yc) / cw[c];   // (the key of the greedy order)
                        }
                    }
                }
            }
        }
        const unsigned long long mask = __ballot(cbin[c]);
        if (lane == 0) cnt[c][wave] = __popcll(mask);
    }
    mir_block_sum2(kpart, zero, red);   // (its barriers also publish cnt and sskip)
    W = (0.0 - bi) - kpart;
    skipped = *sskip != 0 || !(W >= 0.0);
    // the items in column order
    int nb = 0;
#pragma unroll
    for (int c = 0; c < kCovPer; c++) {
        const unsigned long long mask = __ballot(cbin[c]);
        int e = nb;
        for (int w = 0; w < wave; w++) e += cnt[c][w];
        e += __popcll(mask & ((1ull << lane) - 1ull));
        if (cbin[c]) {
            wt[e] = cw[c];
            if (key) key[e] = ck[c];
            col[e] = (uint16_t)((tid + c * kCovNT) | (ccomp[c] ? 0x8000 : 0));
        }
        nb += (cnt[c][0] + cnt[c][1]) + (cnt[c][2] + cnt[c][3]);
    }
    __syncthreads();
    return nb;
}

__global__ void __launch_bounds__(kCovNT) cover_separate(CoverArgs a) {
    __shared__ double wt[kCovMax];      // w_e, item order
    __shared__ double key[kCovMax];     // (1 - y*_e) / w_e, item order; then the weights of C0 in the minimal-cover order
    __shared__ double srt[kCovMax];     // the weights in the greedy order; then mu_h + margin
    __shared__ double pic[kCovMax];     // pi_j, column order
    __shared__ uint16_t col[kCovMax];   // the item's column, bit 15: complemented
    __shared__ uint16_t sidx[kCovMax];  // the item at each position of the greedy order
    __shared__ uint16_t midx[kCovMax];  // the item at each position of the minimal-cover order
    __shared__ uint8_t isint[kCovMax], inC[kCovMax];
    __shared__ double red[2][kCovNT / 64];
    __shared__ int cnt[kCovPer][kCovNT / 64], redi[kCovNT / 64], sskip;
    const int tid = threadIdx.x;
    const int n = a.n;
    const size_t blk = blockIdx.x;
    const int rr = (int)(blk % (size_t)a.R);
    const int row = a.rows ? a.rows[rr] : rr;
    const size_t pt = blk / (size_t)a.R;
    const double *x = a.x + pt * n, *l = a.l + pt * n, *u = a.u + pt * n;
    double *pi = a.pi + blk * n;

    for (int j = tid; j < kCovMax; j += kCovNT) { inC[j] = 0; pic[j] = 0.0; }   // (published by the barriers of the form)
    double W, zero = 0.0;
    bool skipped;
    const int nb = cover_knapsack_form(n, a.n_int, a.int_idx, a.A + (size_t)row * n, a.b[row], x, l, u, wt, key, col, isint,
                                       red, cnt, &sskip, W, skipped);
    const double tau = kCovMargin * fmax(1.0, fabs(W));

    int status = skipped ? 4 : nb < 2 ? 1 : 0;   // (uniform from here on)
    int c0 = 0, r = 0;
    if (status == 0) {
        // GREEDY COVER: the position of item e is the number of keys below (key_e, e)
        double kr[kCovPer];
        int rank[kCovPer];
#pragma unroll
        for (int c = 0; c < kCovPer; c++) {
            const int e = tid + c * kCovNT;
            kr[c] = e < nb ? key[e] : 0.0;
            rank[c] = 0;
        }
        for (int f = 0; f < nb; f++) {
            const double kf = key[f];
#pragma unroll
            for (int c = 0; c < kCovPer; c++) rank[c] += (kf < kr[c] || (kf == kr[c] && f < tid + c * kCovNT)) ? 1 : 0;
        }
#pragma unroll
        for (int c = 0; c < kCovPer; c++) {
            const int e = tid + c * kCovNT;
            if (e < nb) { srt[rank[c]] = wt[e]; sidx[rank[c]] = (uint16_t)e; }
        }
        __syncthreads();
        double P[kCovPer];
        cover_prefix_sum(srt, nb, P, red[0]);
        int first = kCovNone;
#pragma unroll
        for (int k = kCovPer - 1; k >= 0; k--)
            if (kCovPer * tid + k < nb && P[k] - W > tau) first = kCovPer * tid + k;
        first = cover_block_min(first, redi);
        if (first == kCovNone) status = 1;
        c0 = first + 1;
    }
    if (status == 0) {
        // MINIMAL COVER: the position of the item at greedy position p among C0, (w descending, e descending)
        double wr[kCovPer];
        int er[kCovPer], rank[kCovPer];
#pragma unroll
        for (int c = 0; c < kCovPer; c++) {
            const int p = tid + c * kCovNT;
            wr[c] = p < c0 ? srt[p] : 0.0;
            er[c] = p < c0 ? (int)sidx[p] : 0;
            rank[c] = 0;
        }
        for (int f = 0; f < c0; f++) {
            const double wf = srt[f];
            const int ef = sidx[f];
#pragma unroll
            for (int c = 0; c < kCovPer; c++) rank[c] += (wf > wr[c] || (wf == wr[c] && ef > er[c])) ? 1 : 0;
        }
        double *mw = key;   // (the keys are not read again)
#pragma unroll
        for (int c = 0; c < kCovPer; c++) {
            const int p = tid + c * kCovNT;
            if (p < c0) { mw[rank[c]] = wr[c]; midx[rank[c]] = (uint16_t)er[c]; }
        }
        __syncthreads();
        double P[kCovPer];
        cover_prefix_sum(mw, c0, P, red[0]);
        double *thr = srt;   // (the greedy order is not read again: every thread is behind the barriers of the sum)
        int first = kCovNone;
#pragma unroll
        for (int k = kCovPer - 1; k >= 0; k--) {
            const int pos = kCovPer * tid + k;
            if (pos < c0) {
                thr[pos] = P[k] + kCovMargin * fmax(1.0, P[k]);
                if (P[k] - W > tau) first = pos;
            }
        }
        first = cover_block_min(first, redi);
        if (first == kCovNone) status = 1;
        r = first + 1;
    }
    if (status != 0) {
        for (int j = tid; j < n; j += kCovNT) pi[j] = 0.0;
        if (tid == 0) { a.pi0[blk] = 0.0; a.eff[blk] = 0.0; a.size[blk] = 0; a.status[blk] = status; }
        return;
    }
    // LIFTING: the items of C, then every item's coefficient at its column
    for (int p = tid; p < r; p += kCovNT) inC[midx[p]] = 1;
    __syncthreads();   // (also: thr is written)
    {
        const double *thr = srt;
        double we[kCovPer];
        int al[kCovPer];
#pragma unroll
        for (int c = 0; c < kCovPer; c++) {
            const int e = tid + c * kCovNT;
            we[c] = e < nb ? wt[e] : 0.0;
            al[c] = 0;
        }
        for (int h = 0; h < r; h++) {
            const double th = thr[h];
#pragma unroll
            for (int c = 0; c < kCovPer; c++) al[c] += we[c] >= th ? 1 : 0;
        }
#pragma unroll
        for (int c = 0; c < kCovPer; c++) {
            const int e = tid + c * kCovNT;
            if (e < nb) {
                const double alpha = inC[e] ? 1.0 : (double)al[c];
                const int cj = col[e];
                pic[cj & 0x7fff] = (cj & 0x8000) ? alpha : 0.0 - alpha;
            }
        }
    }
    __syncthreads();
    // OUTPUT
    double V = 0.0, Q = 0.0, T = 0.0;
    zero = 0.0;
    for (int j = tid; j < n; j += kCovNT) {
        const double pj = pic[j];
        pi[j] = pj;
        V += pj * x[j];
        Q += pj * pj;
        T += pj > 0.0 ? pj * u[j] : pj < 0.0 ? pj * l[j] : 0.0;
    }
    mir_block_sum2(V, Q, red);
    mir_block_sum2(T, zero, red);
    if (tid == 0) {
        const double pi0 = T - (double)(r - 1);
        const double eff = (pi0 - V) / sqrt(Q);
        a.pi0[blk] = pi0; a.eff[blk] = eff; a.size[blk] = r;
        a.status[blk] = eff > a.min_eff ? 0 : 2;
    }
}

}  // namespace mipx
