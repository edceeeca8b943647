// clique_kernels.hip.h -- the conflict graph and the clique separation of include/mipx_clique.h.
//
//   clique_graph     one workgroup of 256 threads per row of the problem.  The row goes through cover_knapsack_form
//                    (cover_kernels.hip.h), the device code cover_separate uses, which leaves its items (column,
//                    complemented, weight) in LDS in column order.  Thread q takes the items q, q + 256, ... against
//                    every later item, the later item's weight read by all threads at the same LDS address (a
//                    broadcast), and sets both bits of a conflict with an integer atomicOr on the 32-bit word of the
//                    adjacency in global memory, which the entry zeroes on the stream before the launch.  OR has no
//                    order, so the matrix is the same on every run; there is no floating-point atomic.
//   clique_separate  one workgroup of 256 threads (4 waves) per (point, seed).  y* of the 2n literals sits in LDS
//                    (16 KiB), the candidate set C in Wd <= 64 words of LDS.  A round: thread q scans byte q of C
//                    (the literals 8q .. 8q + 7) for its best (y*, literal), a shuffle reduction in each wave, the
//                    four waves through LDS; then the lanes of wave 0 load the winner's row of the adjacency (one
//                    coalesced load of at most 64 words) and AND it into C.  |Q| - 1 rounds, never more than n.  pi,
//                    pi0 and the efficacy follow in the BLOCK SUM order of mipx_mir.h, as in cover_separate.
//
// Products are not fused (the library is built with -ffp-contract=off); tests/support/clique_reference.py restates both.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace mipx {

constexpr int kCliqueWords = 2 * kCovMax / 32;   // words of an adjacency row at most

struct CliqueGraphArgs {
    int m, n, n_int, Wd;
    const double *A, *b;              // the problem's rows A x >= b (m x n, row-major)
    const double *l, *u;              // n each: the box
    const int32_t *int_idx;           // the integer columns, n_int of them
    uint32_t *adj;                    // 2n x Wd, zeroed before the launch
    int32_t *row_status;              // m
};

struct CliqueArgs {
    int n, n_int, R, Wd;
    double min_eff;
    const double *x;                  // batch x n
    const double *l, *u;              // n each: the box
    const int32_t *int_idx;           // the integer columns, n_int of them
    const uint32_t *adj;              // 2n x Wd
    const int32_t *seeds;             // nullable: R literals (null: the 2n literals)
    double *pi, *pi0, *eff;           // batch x R x n, batch x R each
    int32_t *size, *status;           // batch x R
};

__global__ void __launch_bounds__(kCovNT) clique_graph(CliqueGraphArgs a) {
    __shared__ double wt[kCovMax];      // w_e, item order
    __shared__ uint16_t col[kCovMax];   // the item's column, bit 15: complemented
    __shared__ uint8_t isint[kCovMax];
    __shared__ double red[2][kCovNT / 64];
    __shared__ int cnt[kCovPer][kCovNT / 64], sskip;
    const int tid = threadIdx.x;
    const int n = a.n, row = blockIdx.x;
    double W;
    bool skipped;
    const int nb = cover_knapsack_form(n, a.n_int, a.int_idx, a.A + (size_t)row * n, a.b[row], nullptr, a.l, a.u, wt, nullptr,
                                       col, isint, red, cnt, &sskip, W, skipped);
    if (tid == 0) a.row_status[row] = skipped ? 4 : 0;
    if (skipped) return;
    const double tau = kCovMargin * fmax(1.0, fabs(W));
    double we[kCovPer];
    int le[kCovPer];   // the literal of this thread's item of chunk c
#pragma unroll
    for (int c = 0; c < kCovPer; c++) {
        const int e = tid + c * kCovNT;
        we[c] = e < nb ? wt[e] : 0.0;
        le[c] = e < nb ? 2 * (col[e] & 0x7fff) + (col[e] >> 15) : 0;
    }
    for (int f = 1; f < nb; f++) {
        const double wf = wt[f];
        const int cf = col[f];
        const int lf = 2 * (cf & 0x7fff) + (cf >> 15);
#pragma unroll
        for (int c = 0; c < kCovPer; c++) {
            const int e = tid + c * kCovNT;
            if (e < f && (we[c] + wf) - W > tau) {   // CONFLICT (e < f < nb)
                atomicOr(a.adj + (size_t)le[c] * a.Wd + (lf >> 5), 1u << (lf & 31));
                atomicOr(a.adj + (size_t)lf * a.Wd + (le[c] >> 5), 1u << (le[c] & 31));
            }
        }
    }
}

// The better of two candidates (y*, literal): the larger y*, ties to the smaller literal; kCovNone is no candidate.
__device__ inline void clique_better(double &y, int &lit, double y2, int lit2) {
    if (lit2 != kCovNone && (lit == kCovNone || y2 > y || (y2 == y && lit2 < lit))) { y = y2; lit = lit2; }
}

__global__ void __launch_bounds__(kCovNT) clique_separate(CliqueArgs a) {
    __shared__ double ys[2 * kCovMax];     // y*_k, 0 for a literal that is not live
    __shared__ double pic[kCovMax];        // pi_j, column order
    __shared__ uint32_t C[kCliqueWords];   // the candidates
    __shared__ uint32_t live[kCliqueWords];
    __shared__ uint8_t bin[kCovMax];       // the column is an integer column, then: it is binary
    __shared__ double red[2][kCovNT / 64];
    __shared__ double redy[kCovNT / 64];
    __shared__ int redl[kCovNT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.n, Wd = a.Wd;
    const size_t blk = blockIdx.x;
    const int rr = (int)(blk % (size_t)a.R);
    const int seed = a.seeds ? a.seeds[rr] : rr;
    const size_t pt = blk / (size_t)a.R;
    const double *x = a.x + pt * n, *l = a.l, *u = a.u;
    const double inf = __builtin_huge_val();
    double *pi = a.pi + blk * n;

    for (int j = tid; j < kCovMax; j += kCovNT) { bin[j] = 0; pic[j] = 0.0; }
    __syncthreads();
    for (int k = tid; k < a.n_int; k += kCovNT) bin[a.int_idx[k]] = 1;
    __syncthreads();
    // LITERALS: y* of both literals of every column (each thread reads and rewrites the marks of its own columns only)
    for (int j = tid; j < kCovMax; j += kCovNT) {
        double y0 = 0.0, y1 = 0.0;
        bool b = false;
        if (j < n) {
            const double xj = x[j], lj = l[j], uj = u[j];
            b = bin[j] && uj < inf && floor(lj) == lj && floor(uj) == uj && uj - lj == 1.0;
            if (b) {
                y0 = xj - lj; y1 = uj - xj;
                y0 = y0 < 0.0 ? 0.0 : y0 > 1.0 ? 1.0 : y0;
                y1 = y1 < 0.0 ? 0.0 : y1 > 1.0 ? 1.0 : y1;
            }
        }
        bin[j] = b ? 1 : 0;
        ys[2 * j] = y0; ys[2 * j + 1] = y1;
    }
    __syncthreads();
    if (tid < kCliqueWords) {   // the live literals of word tid: the two bits of each of its 16 columns
        uint32_t w = 0;
        for (int k = 0; k < 16; k++) w |= bin[16 * tid + k] ? 3u << (2 * k) : 0u;
        live[tid] = w;
        C[tid] = tid < Wd ? a.adj[(size_t)seed * Wd + tid] & w & ~(tid == (seed >> 5) ? 1u << (seed & 31) : 0u) : 0u;
    }
    __syncthreads();
    int status = !bin[seed >> 1] ? 4 : !(ys[seed] > 0.0) ? 1 : 0;   // (uniform from here on)
    int size = 1;
    if (status == 0) {
        if (tid == 0) pic[seed >> 1] = (seed & 1) ? 1.0 : 0.0 - 1.0;
        for (int round = 0; round < n; round++) {
            // every thread: the best of the literals 8 tid .. 8 tid + 7 of C
            double by = 0.0;
            int bl = kCovNone;
            uint32_t byte = (C[tid >> 2] >> (8 * (tid & 3))) & 0xffu;
            while (byte) {
                const int k = 8 * tid + __builtin_ctz(byte);
                byte &= byte - 1;
                clique_better(by, bl, ys[k], k);
            }
            for (int off = 32; off > 0; off >>= 1) {
                const double oy = __shfl_xor(by, off, 64);
                const int ol = __shfl_xor(bl, off, 64);
                clique_better(by, bl, oy, ol);
            }
            if (lane == 0) { redy[wave] = by; redl[wave] = bl; }
            __syncthreads();
            by = redy[0]; bl = redl[0];
            for (int w = 1; w < kCovNT / 64; w++) clique_better(by, bl, redy[w], redl[w]);
            if (bl == kCovNone) break;   // (C is empty; uniform)
            const int t = bl;
            if (tid < Wd) C[tid] &= a.adj[(size_t)t * Wd + tid] & ~(tid == (t >> 5) ? 1u << (t & 31) : 0u);
            if (tid == 0) pic[t >> 1] = (t & 1) ? 1.0 : 0.0 - 1.0;
            size++;
            __syncthreads();   // (C is written, and the slots of the reduction are read)
        }
        if (size < 2) status = 1;
    }
    if (status != 0) {
        for (int j = tid; j < n; j += kCovNT) pi[j] = 0.0;
        if (tid == 0) { a.pi0[blk] = 0.0; a.eff[blk] = 0.0; a.size[blk] = 0; a.status[blk] = status; }
        return;
    }
    __syncthreads();   // (pic is written)
    // OUTPUT
    double V = 0.0, Q = 0.0, T = 0.0, zero = 0.0;
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
        const double pi0 = T - 1.0;
        const double eff = (pi0 - V) / sqrt(Q);
        a.pi0[blk] = pi0; a.eff[blk] = eff; a.size[blk] = size;
        a.status[blk] = eff > a.min_eff ? 0 : 2;
    }
}

}  // namespace mipx
