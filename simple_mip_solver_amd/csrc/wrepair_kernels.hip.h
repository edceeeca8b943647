// wrepair_kernels.hip.h -- the weighted row repair of include/mipx_wrepair.h: round an LP point, then mend the rows
// the rounding broke by unit moves under row weights that grow where no move helps.
//
//   wrepair_steps   one workgroup of 256 threads (4 waves) per point.  The point x~, the row activities
//                   s = A x~ - b, the row weights and the rounded bounds of the integer columns live in LDS: four
//                   arrays of doubles and the weights as 32-bit integers (they are whole numbers of at most
//                   max_steps + 1, and turn into doubles, exactly, where a product takes them), 36 KiB at
//                   1024 x 1024, so four workgroups fit into a CU's 160 KiB.  Thread t owns the integer columns
//                   int_idx[t], int_idx[t + 256], ...; for a step it walks the rows in ascending order once, for all
//                   its columns and both directions at a time (row-major A: the threads of a wave read neighbouring
//                   columns of one row, s_i and w_i are LDS broadcasts), keeps its best key, and the workgroup
//                   takes the arg-min: __shfl_xor inside a wave, one LDS slot per wave across them.  A key ends in
//                   (column, direction), so no two compare equal and the winner depends on nothing else.
//                   V, and whether any row is violated at all, is taken by every thread for itself at the top of a
//                   step, from s and w in LDS behind the barrier that ended the last step: rows ascending, one
//                   product and one add per violated row, the reads broadcast.  All threads so hold the same bits,
//                   and "move or bump" and "go on or stop" are decided from them and from the arg-min alike in
//                   every thread, with no further exchange.  The move (s_i += d a_ij) or the bump (w_i += 1 on the
//                   violated rows) is applied by the threads striding the rows.  Plain vector stores, no atomics,
//                   no scratch.
//
// Every sum is taken in the order mipx_wrepair.h states (rows ascending, columns ascending, one add per term; the
// library is built with -ffp-contract=off), so that a restatement in the same order gives the same bits.  The
// rounding, the keys and the arg-min are the heuristic's (heur_kernels.hip.h), restated here so that
// heur_round_repair stays as it is.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace mipx {

constexpr int kWrNT = 256;     // threads per workgroup
constexpr int kWrMax = 1024;   // rows and columns at most (what the LP kernels take)
constexpr int kWrOwn = kWrMax / kWrNT;   // integer columns per thread at most
constexpr int kWrNone = 0x7fffffff;

struct WrepairArgs {
    int m, n, n_int, max_steps;
    int keep_gated;                 // 1: x_out holds the points of the heuristic that gate comes from; the slots of the
                                    // points the gate leaves out are not touched (nor are their obj_out)
    double tol;
    const double *A, *b, *c;        // the problem's rows A x >= b (m x n, row-major) and objective
    const double *l, *u;            // the root's bounds, n each
    const int32_t *int_idx;         // the integer columns, n_int of them
    const double *x;                // batch x n: the points
    const uint8_t *skip;            // nullable: a point whose entry is not 0 is skipped (x copied, obj 0)
    const int32_t *gate;            // nullable, the status of the heuristic that tried the point first: a point whose
                                    // entry is not 1 or 2 (stuck, capped) is skipped
    double *x_out, *obj_out;        // batch x n, batch
    int32_t *status_out, *counts_out;   // batch, 2 x batch (moves, bumps)
};

// (V', c_j d, 2 j + (d < 0)): compared in that order; kWrNone in the last field means "no candidate"
struct WrKey { double v, cd; int jd; };

__device__ inline bool wr_less(const WrKey &a, const WrKey &b) {
    if (a.jd == kWrNone) return false;
    if (b.jd == kWrNone) return true;
    if (a.v != b.v) return a.v < b.v;
    if (a.cd != b.cd) return a.cd < b.cd;
    return a.jd < b.jd;
}

// the smallest key of the workgroup, in every thread (slots: one per wave); behind it every thread has left the sweep
__device__ inline WrKey wr_block_min(WrKey k, WrKey *slots) {
    for (int off = 32; off > 0; off >>= 1) {
        WrKey o;
        o.v = __shfl_xor(k.v, off, 64);
        o.cd = __shfl_xor(k.cd, off, 64);
        o.jd = __shfl_xor(k.jd, off, 64);
        if (wr_less(o, k)) k = o;
    }
    if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = k;
    __syncthreads();
    WrKey r = slots[0];
    for (int w = 1; w < kWrNT / 64; w++)
        if (wr_less(slots[w], r)) r = slots[w];
    __syncthreads();   // (the slots are written again by the next step)
    return r;
}

__global__ void __launch_bounds__(kWrNT) wrepair_steps(WrepairArgs a) {
    __shared__ double s[kWrMax], xt[kWrMax], slo[kWrMax], shi[kWrMax];   // (slo, shi: by position in int_idx)
    __shared__ int32_t sw[kWrMax];
    __shared__ WrKey slots[kWrNT / 64];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int m = a.m, n = a.n;
    const double tol = a.tol;
    const double *x = a.x + (size_t)p * n;
    double *xo = a.x_out + (size_t)p * n;
    const bool gated = a.gate && a.gate[p] != 1 && a.gate[p] != 2;   // (uniform over the workgroup)
    if (gated || (a.skip && a.skip[p])) {
        if (!(gated && a.keep_gated)) {
            if (xo != x)
                for (int j = tid; j < n; j += kWrNT) xo[j] = x[j];
            if (tid == 0) a.obj_out[p] = 0.0;
        }
        if (tid == 0) {
            a.status_out[p] = 3;
            a.counts_out[2 * p] = 0;
            a.counts_out[2 * p + 1] = 0;
        }
        return;
    }
    // ROUND: the integer columns to the nearest integer inside the rounded bounds, the others as they are
    for (int j = tid; j < n; j += kWrNT) xt[j] = x[j];
    for (int i = tid; i < m; i += kWrNT) sw[i] = 1;
    __syncthreads();
    int oj[kWrOwn];
    double oc[kWrOwn];
#pragma unroll
    for (int q = 0; q < kWrOwn; q++) {
        const int k = tid + q * kWrNT;
        oj[q] = -1; oc[q] = 0.0;
        if (k < a.n_int) {
            const int j = a.int_idx[k];
            const double lo = ceil(a.l[j] - tol), hi = floor(a.u[j] + tol);
            oj[q] = j;
            oc[q] = a.c[j];
            slo[k] = lo;
            shi[k] = hi;
            xt[j] = fmin(fmax(floor(x[j] + 0.5), lo), hi) + 0.0;   // (+ 0.0: a zero result is +0 whatever max / min pick)
        }
    }
    __syncthreads();
    // s_i = a_i . x~ - b_i, columns ascending
    for (int i = tid; i < m; i += kWrNT) {
        const double *row = a.A + (size_t)i * n;
        double acc = 0.0;
        for (int j = 0; j < n; j++) acc += row[j] * xt[j];
        s[i] = acc - a.b[i];
    }
    __syncthreads();
    int moves = 0, bumps = 0, status = 0;
    for (;;) {
        // V = sum of w_i (-s_i) over the violated rows, rows ascending (every thread: the reads broadcast)
        double V = 0.0;
        int violated = 0;
        for (int i = 0; i < m; i++) {
            const double si = s[i];
            if (si < -tol) {
                V += (double)sw[i] * (-si);
                violated++;
            }
        }
        if (violated == 0) break;
        if (moves + bumps >= a.max_steps) { status = 2; break; }
        // the candidates of this thread's columns: which are inside the rounded bounds, then one walk down the rows
        bool up[kWrOwn], dn[kWrOwn];
        double vu[kWrOwn], vd[kWrOwn];
        bool any = false;
#pragma unroll
        for (int q = 0; q < kWrOwn; q++) {
            up[q] = false; dn[q] = false; vu[q] = 0.0; vd[q] = 0.0;
            if (oj[q] >= 0) {
                const int k = tid + q * kWrNT;
                const double xv = xt[oj[q]], lo = slo[k], hi = shi[k];
                up[q] = xv + 1.0 >= lo && xv + 1.0 <= hi;
                dn[q] = xv - 1.0 >= lo && xv - 1.0 <= hi;
                any = any || up[q] || dn[q];
            }
        }
        if (any) {
            for (int i = 0; i < m; i++) {
                const double si = s[i], wi = (double)sw[i];
                const double *row = a.A + (size_t)i * n;
#pragma unroll
                for (int q = 0; q < kWrOwn; q++) {
                    if (!(up[q] || dn[q])) continue;
                    const double aij = row[oj[q]];
                    const double tu = si + aij, td = si - aij;
                    if (tu < -tol) vu[q] += wi * (-tu);
                    if (td < -tol) vd[q] += wi * (-td);
                }
            }
        }
        WrKey best;
        best.v = 0.0; best.cd = 0.0; best.jd = kWrNone;
#pragma unroll
        for (int q = 0; q < kWrOwn; q++) {
            WrKey k;
            if (up[q]) {
                k.v = vu[q]; k.cd = oc[q]; k.jd = 2 * oj[q];
                if (wr_less(k, best)) best = k;
            }
            if (dn[q]) {
                k.v = vd[q]; k.cd = -oc[q]; k.jd = 2 * oj[q] + 1;
                if (wr_less(k, best)) best = k;
            }
        }
        best = wr_block_min(best, slots);
        if (best.jd != kWrNone && best.v < V) {   // a move
            const int j = best.jd >> 1;
            const double d = (best.jd & 1) ? -1.0 : 1.0;
            for (int i = tid; i < m; i += kWrNT) s[i] = s[i] + d * a.A[(size_t)i * n + j];
            if (tid == 0) xt[j] = xt[j] + d;
            moves++;
        } else {   // a bump
            for (int i = tid; i < m; i += kWrNT)
                if (s[i] < -tol) sw[i] = sw[i] + 1;
            bumps++;
        }
        __syncthreads();
    }
    if (status == 0) {
        for (int j = tid; j < n; j += kWrNT) xo[j] = xt[j];
    } else if (xo != x) {
        for (int j = tid; j < n; j += kWrNT) xo[j] = x[j];
    }
    if (tid == 0) {
        double obj = 0.0;
        if (status == 0)
            for (int j = 0; j < n; j++) obj += a.c[j] * xt[j];
        a.obj_out[p] = obj;
        a.status_out[p] = status;
        a.counts_out[2 * p] = moves;
        a.counts_out[2 * p + 1] = bumps;
    }
}

}  // namespace mipx
