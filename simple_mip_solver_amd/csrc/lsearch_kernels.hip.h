// lsearch_kernels.hip.h -- the pair-move local search of include/mipx_lsearch.h: from a feasible integral point,
// moves of one or two integer columns by one unit that lower the objective and keep every row.
//
//   ls_pair_search   one workgroup of 256 threads (4 waves) per point.  The slacks s = A x - b, the point and the
//                    rounded bounds live in LDS (about 33 KiB).  Thread t owns the columns k = t, t + 256, ... with
//                    their costs in registers.  For a move the workgroup walks the outer column j ascending, both
//                    dj at once: a_ij is a uniform load, s_i an LDS broadcast, a_ik a coalesced read of the
//                    row-major A, and a thread carries four live flags (dj, dk) per owned column.  A (k, dk) whose
//                    cost cannot make the pair improving never touches A, a wave leaves the row loop when its
//                    ballot shows no live flag, and an outer j with no room is skipped.  The singles of j ride
//                    along: their two flags depend on uniform values only, so every wave holds the same.  The
//                    workgroup takes the arg-min of the full key as heur_round_repair does: __shfl_xor inside a
//                    wave, one LDS slot per wave across them.  No atomics; the output may be the input.
//
// Every sum is taken in the order mipx_lsearch.h states and nothing is fused (-ffp-contract=off), so that a
// restatement in the same order gives the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace mipx {

constexpr int kLsNT = 256;     // threads per workgroup
constexpr int kLsMax = 1024;   // rows and columns at most (what the LP kernels take)
constexpr int kLsOwn = kLsMax / kLsNT;   // columns per thread at most
constexpr int kLsNone = 0x7fffffff;

struct LsArgs {
    int m, n, n_int, max_moves;
    double tol;
    const double *A, *b, *c;        // the problem's rows A x >= b (m x n, row-major) and objective
    const double *l, *u;            // the bounds, n each
    const int32_t *int_idx;         // the integer columns, n_int of them
    const double *x;                // batch x n: the points
    const uint8_t *skip;            // nullable: a point whose entry is not 0 is skipped (x copied, obj 0)
    const int32_t *gate;            // nullable: a point whose entry is not 0 is skipped and neither x_out nor obj_out is touched
    double *x_out, *obj_out;        // batch x n (may be x), batch
    int32_t *status_out, *moves_out;   // batch, 2 x batch (singles, pairs)
};

// (g, id) compared in that order; id = j * 8192 + (k + 1) * 4 + 2 * (dj < 0) + (dk < 0), k = -1 for a single: the
// order of (j, k, dj, dk) with +1 before -1.  kLsNone means "no candidate".
struct LsKey { double g; int id; };

__device__ inline bool ls_less(const LsKey &a, const LsKey &b) {
    if (a.id == kLsNone) return false;
    if (b.id == kLsNone) return true;
    if (a.g != b.g) return a.g < b.g;
    return a.id < b.id;
}

// the smallest key of the workgroup, in every thread (slots: one per wave)
__device__ inline LsKey ls_block_min(LsKey k, LsKey *slots) {
    for (int off = 32; off > 0; off >>= 1) {
        LsKey o;
        o.g = __shfl_xor(k.g, off, 64);
        o.id = __shfl_xor(k.id, off, 64);
        if (ls_less(o, k)) k = o;
    }
    if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = k;
    __syncthreads();
    LsKey r = slots[0];
    for (int w = 1; w < kLsNT / 64; w++)
        if (ls_less(slots[w], r)) r = slots[w];
    __syncthreads();   // (the slots are written again by the next move)
    return r;
}

__global__ void __launch_bounds__(kLsNT) ls_pair_search(LsArgs a) {
    __shared__ double s[kLsMax], xs[kLsMax], slo[kLsMax], shi[kLsMax];
    __shared__ uint8_t isint[kLsMax];
    __shared__ LsKey slots[kLsNT / 64];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int m = a.m, n = a.n;
    const double tol = a.tol;
    if (a.gate && a.gate[p] != 0) {   // (uniform over the workgroup)
        if (tid == 0) {
            a.status_out[p] = 3;
            a.moves_out[2 * p] = 0;
            a.moves_out[2 * p + 1] = 0;
        }
        return;
    }
    const double *x = a.x + (size_t)p * n;
    double *xo = a.x_out + (size_t)p * n;
    if (a.skip && a.skip[p]) {
        if (xo != x)
            for (int j = tid; j < n; j += kLsNT) xo[j] = x[j];
        if (tid == 0) {
            a.obj_out[p] = 0.0;
            a.status_out[p] = 3;
            a.moves_out[2 * p] = 0;
            a.moves_out[2 * p + 1] = 0;
        }
        return;
    }
    // the point and the rounded bounds; a column that is not integer has the empty range [1, 0]: no room either way
    for (int j = tid; j < n; j += kLsNT) { xs[j] = x[j]; slo[j] = 1.0; shi[j] = 0.0; isint[j] = 0; }
    __syncthreads();
    for (int k = tid; k < a.n_int; k += kLsNT) {
        const int j = a.int_idx[k];
        slo[j] = ceil(a.l[j] - tol);
        shi[j] = floor(a.u[j] + tol);
        isint[j] = 1;
    }
    __syncthreads();
    // check: s_i = a_i . x - b_i, columns ascending; integrality and the rounded bounds of the integer columns
    int bad = 0;
    for (int i = tid; i < m; i += kLsNT) {
        const double *row = a.A + (size_t)i * n;
        double acc = 0.0;
        for (int j = 0; j < n; j++) acc += row[j] * xs[j];
        const double si = acc - a.b[i];
        s[i] = si;
        if (si < -tol) bad = 1;
    }
    for (int j = tid; j < n; j += kLsNT) {
        const double xv = xs[j];
        if (isint[j] && (xv != floor(xv) || !(xv >= slo[j] && xv <= shi[j]))) bad = 1;
    }
    bad = __syncthreads_or(bad);
    int singles = 0, pairs = 0, status = 2;
    double oc[kLsOwn];
#pragma unroll
    for (int q = 0; q < kLsOwn; q++) {
        const int k = tid + q * kLsNT;
        oc[q] = k < n ? a.c[k] : 0.0;
    }
    while (!bad) {
        // room of the thread's columns at this point: bit 2q up, bit 2q + 1 down
        unsigned room = 0;
#pragma unroll
        for (int q = 0; q < kLsOwn; q++) {
            const int k = tid + q * kLsNT;
            if (k < n) {
                const double xv = xs[k], lo = slo[k], hi = shi[k];
                if (xv + 1.0 >= lo && xv + 1.0 <= hi) room |= 1u << (2 * q);
                if (xv - 1.0 >= lo && xv - 1.0 <= hi) room |= 2u << (2 * q);
            }
        }
        LsKey best;
        best.g = 0.0; best.id = kLsNone;
        for (int j = 0; j < n; j++) {   // (everything about j is uniform over the workgroup)
            const double xj = xs[j], lj = slo[j], hj = shi[j];
            const bool ju = xj + 1.0 >= lj && xj + 1.0 <= hj, jd = xj - 1.0 >= lj && xj - 1.0 <= hj;
            if (!ju && !jd) continue;
            const double gu = a.c[j], gd = -gu;   // c_j dj for dj = +1, -1
            bool su = ju && gu < 0.0, sd = jd && gd < 0.0;   // the singles of j still alive
            // live pairs of the thread's columns: bit 4q + 2 (dj < 0) + (dk < 0), killed by the cost test first
            unsigned live = 0;
#pragma unroll
            for (int q = 0; q < kLsOwn; q++) {
                const int k = tid + q * kLsNT;
                if (k > j && k < n) {
                    const bool ku = (room >> (2 * q)) & 1u, kd = (room >> (2 * q + 1)) & 1u;
                    const double cu = oc[q], cd = -oc[q];
                    if (ju && ku && gu + cu < 0.0) live |= 1u << (4 * q);
                    if (ju && kd && gu + cd < 0.0) live |= 2u << (4 * q);
                    if (jd && ku && gd + cu < 0.0) live |= 4u << (4 * q);
                    if (jd && kd && gd + cd < 0.0) live |= 8u << (4 * q);
                }
            }
            for (int i = 0; i < m; i++) {
                if (!su && !sd && __ballot(live != 0) == 0) break;   // (su, sd are uniform: the whole wave leaves)
                const double *row = a.A + (size_t)i * n;
                const double si = s[i], aij = row[j];
                const double tu = si + aij, td = si - aij;
                su = su && tu >= -tol;
                sd = sd && td >= -tol;
#pragma unroll
                for (int q = 0; q < kLsOwn; q++) {
                    const unsigned f = (live >> (4 * q)) & 15u;
                    if (f) {
                        const double aik = row[tid + q * kLsNT];
                        unsigned keep = 0;
                        if (tu + aik >= -tol) keep |= 1u;
                        if (tu - aik >= -tol) keep |= 2u;
                        if (td + aik >= -tol) keep |= 4u;
                        if (td - aik >= -tol) keep |= 8u;
                        live &= ~((f & ~keep) << (4 * q));
                    }
                }
            }
            // what is left is a candidate; a key of this j is below every key of a later j with the same g
            LsKey k;
            if (tid == 0) {
                if (su) { k.g = gu; k.id = j * 8192; if (ls_less(k, best)) best = k; }
                if (sd) { k.g = gd; k.id = j * 8192 + 2; if (ls_less(k, best)) best = k; }
            }
            if (live) {
#pragma unroll
                for (int q = 0; q < kLsOwn; q++) {
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        if ((live >> (4 * q + e)) & 1u) {
                            k.g = ((e & 2) ? gd : gu) + ((e & 1) ? -oc[q] : oc[q]);
                            k.id = j * 8192 + (tid + q * kLsNT + 1) * 4 + e;
                            if (ls_less(k, best)) best = k;
                        }
                    }
                }
            }
        }
        best = ls_block_min(best, slots);   // (its barriers: every wave is done reading s)
        if (best.id == kLsNone) { status = 0; break; }
        if (singles + pairs >= a.max_moves) { status = 1; break; }
        const int j = best.id / 8192, k = ((best.id % 8192) >> 2) - 1;
        const double dj = (best.id & 2) ? -1.0 : 1.0, dk = (best.id & 1) ? -1.0 : 1.0;
        for (int i = tid; i < m; i += kLsNT) {
            const double *row = a.A + (size_t)i * n;
            double t = s[i] + dj * row[j];
            if (k >= 0) t = t + dk * row[k];
            s[i] = t;
        }
        if (tid == 0) {
            xs[j] = xs[j] + dj;
            if (k >= 0) xs[k] = xs[k] + dk;
        }
        if (k >= 0) pairs++; else singles++;
        __syncthreads();
    }
    // (a point that failed the check comes back as it went in: xs holds it untouched)
    for (int j = tid; j < n; j += kLsNT) xo[j] = xs[j];
    if (tid == 0) {
        double obj = 0.0;
        for (int j = 0; j < n; j++) obj += a.c[j] * xs[j];
        a.obj_out[p] = obj;
        a.status_out[p] = status;
        a.moves_out[2 * p] = singles;
        a.moves_out[2 * p + 1] = pairs;
    }
}

}  // namespace mipx
