// heur_kernels.hip.h -- the primal heuristic of include/mipx_heur.h: round an LP point, repair the rows the
// rounding broke by unit moves, then lift the objective by unit moves that keep every row.
//
//   heur_round_repair   one workgroup of 256 threads (4 waves) per point.  The row activities s = A x~ - b, the
//                       point x~ and the rounded bounds of the integer columns live in LDS.  Thread t owns the
//                       integer columns int_idx[t], int_idx[t + 256], ...; for a move it walks the rows of its
//                       columns in ascending order (row-major A: the threads of a wave read neighbouring columns
//                       of one row), keeps its best candidate, and the workgroup takes the arg-min of the keys:
//                       __shfl_xor inside a wave, one LDS slot per wave across them.  A key ends in (column,
//                       direction), so no two candidates compare equal and the winner depends on nothing else.
//
// Every sum is taken in the order mipx_heur.h states (rows ascending, columns ascending, one add per term; the
// library is built with -ffp-contract=off), so that a restatement in the same order gives the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace mipx {

constexpr int kHeurNT = 256;     // threads per workgroup
constexpr int kHeurMax = 1024;   // rows and columns at most (what the LP kernels take)
constexpr int kHeurOwn = kHeurMax / kHeurNT;   // integer columns per thread at most
constexpr int kHeurNone = 0x7fffffff;

struct HeurArgs {
    int m, n, n_int, max_moves;
    double tol;
    const double *A, *b, *c;        // the problem's rows A x >= b (m x n, row-major) and objective
    const double *l, *u;            // the root's bounds, n each
    const int32_t *int_idx;         // the integer columns, n_int of them
    const double *x;                // batch x n: the points
    const int32_t *lp_status;       // nullable: a point whose entry is not 0 is skipped
    const uint8_t *skip;            // nullable: a point whose entry is not 0 is skipped
    double *x_out, *obj_out;        // batch x n, batch
    int32_t *status_out, *moves_out;   // batch, 2 x batch (repair, lift)
};

// (value, c_j d, 2 j + (d < 0)): compared in that order; kHeurNone in the last field means "no candidate"
struct HeurKey { double v, cd; int jd; };

__device__ inline bool heur_less(const HeurKey &a, const HeurKey &b) {
    if (a.jd == kHeurNone) return false;
    if (b.jd == kHeurNone) return true;
    if (a.v != b.v) return a.v < b.v;
    if (a.cd != b.cd) return a.cd < b.cd;
    return a.jd < b.jd;
}

// the smallest key of the workgroup, in every thread (slots: one per wave)
__device__ inline HeurKey heur_block_min(HeurKey k, HeurKey *slots) {
    for (int off = 32; off > 0; off >>= 1) {
        HeurKey o;
        o.v = __shfl_xor(k.v, off, 64);
        o.cd = __shfl_xor(k.cd, off, 64);
        o.jd = __shfl_xor(k.jd, off, 64);
        if (heur_less(o, k)) k = o;
    }
    if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = k;
    __syncthreads();
    HeurKey r = slots[0];
    for (int w = 1; w < kHeurNT / 64; w++)
        if (heur_less(slots[w], r)) r = slots[w];
    __syncthreads();   // (the slots are written again by the next move)
    return r;
}

__global__ void __launch_bounds__(kHeurNT) heur_round_repair(HeurArgs a) {
    __shared__ double s[kHeurMax], xt[kHeurMax];
    __shared__ HeurKey slots[kHeurNT / 64];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int m = a.m, n = a.n;
    const double tol = a.tol;
    const double *x = a.x + (size_t)p * n;
    double *xo = a.x_out + (size_t)p * n;
    if ((a.skip && a.skip[p]) || (a.lp_status && a.lp_status[p] != 0)) {   // (uniform over the workgroup)
        for (int j = tid; j < n; j += kHeurNT) xo[j] = x[j];
        if (tid == 0) {
            a.obj_out[p] = 0.0;
            a.status_out[p] = 3;
            a.moves_out[2 * p] = 0;
            a.moves_out[2 * p + 1] = 0;
        }
        return;
    }
    // round: the integer columns to the nearest integer inside the rounded bounds, the others as they are
    for (int j = tid; j < n; j += kHeurNT) xt[j] = x[j];
    __syncthreads();
    int oj[kHeurOwn];
    double olo[kHeurOwn], ohi[kHeurOwn], oc[kHeurOwn];
#pragma unroll
    for (int q = 0; q < kHeurOwn; q++) {
        const int k = tid + q * kHeurNT;
        oj[q] = -1; olo[q] = 0.0; ohi[q] = 0.0; oc[q] = 0.0;
        if (k < a.n_int) {
            const int j = a.int_idx[k];
            oj[q] = j;
            olo[q] = ceil(a.l[j] - tol);
            ohi[q] = floor(a.u[j] + tol);
            oc[q] = a.c[j];
            xt[j] = fmin(fmax(floor(x[j] + 0.5), olo[q]), ohi[q]) + 0.0;   // (+ 0.0: a zero result is +0 whatever max / min pick)
        }
    }
    __syncthreads();
    // s_i = a_i . x~ - b_i, columns ascending
    for (int i = tid; i < m; i += kHeurNT) {
        const double *row = a.A + (size_t)i * n;
        double acc = 0.0;
        for (int j = 0; j < n; j++) acc += row[j] * xt[j];
        s[i] = acc - a.b[i];
    }
    __syncthreads();
    // V = sum of the violations, rows ascending (every thread: the reads broadcast)
    double V = 0.0;
    for (int i = 0; i < m; i++) {
        const double si = s[i];
        if (si < -tol) V += -si;
    }
    int repair = 0, lift = 0, status = 0;
    // repair: the move that lowers V most, while a row is violated
    while (V > 0.0 && repair < a.max_moves) {
        HeurKey best;
        best.v = 0.0; best.cd = 0.0; best.jd = kHeurNone;
#pragma unroll
        for (int q = 0; q < kHeurOwn; q++) {
            const int j = oj[q];
            if (j < 0) continue;
            const double xv = xt[j];
            const bool up = xv + 1.0 >= olo[q] && xv + 1.0 <= ohi[q], dn = xv - 1.0 >= olo[q] && xv - 1.0 <= ohi[q];
            if (!up && !dn) continue;
            double vu = 0.0, vd = 0.0;
            const double *col = a.A + j;
            for (int i = 0; i < m; i++) {
                const double aij = col[(size_t)i * n], si = s[i];
                const double tu = si + aij, td = si - aij;
                if (tu < -tol) vu += -tu;
                if (td < -tol) vd += -td;
            }
            HeurKey k;
            if (up && vu < V) {
                k.v = vu; k.cd = oc[q]; k.jd = 2 * j;
                if (heur_less(k, best)) best = k;
            }
            if (dn && vd < V) {
                k.v = vd; k.cd = -oc[q]; k.jd = 2 * j + 1;
                if (heur_less(k, best)) best = k;
            }
        }
        best = heur_block_min(best, slots);
        if (best.jd == kHeurNone) { status = 1; break; }
        const int j = best.jd >> 1;
        const double d = (best.jd & 1) ? -1.0 : 1.0;
        for (int i = tid; i < m; i += kHeurNT) s[i] = s[i] + d * a.A[(size_t)i * n + j];
        if (tid == 0) xt[j] = xt[j] + d;
        V = best.v;
        repair++;
        __syncthreads();
    }
    if (V > 0.0 && status == 0) status = 2;
    // lift: the move that lowers the objective most and keeps every row
    while (status == 0 && repair + lift < a.max_moves) {
        HeurKey best;
        best.v = 0.0; best.cd = 0.0; best.jd = kHeurNone;
#pragma unroll
        for (int q = 0; q < kHeurOwn; q++) {
            const int j = oj[q];
            if (j < 0 || oc[q] == 0.0) continue;
            const double d = oc[q] < 0.0 ? 1.0 : -1.0;   // (the one direction with c_j d < 0)
            const double xv = xt[j] + d;
            if (!(xv >= olo[q] && xv <= ohi[q])) continue;
            const double *col = a.A + j;
            bool ok = true;
            for (int i = 0; i < m && ok; i++) ok = s[i] + d * col[(size_t)i * n] >= -tol;
            if (!ok) continue;
            HeurKey k;
            k.v = 0.0; k.cd = oc[q] * d; k.jd = 2 * j + (d < 0.0 ? 1 : 0);
            if (heur_less(k, best)) best = k;
        }
        best = heur_block_min(best, slots);
        if (best.jd == kHeurNone) break;
        const int j = best.jd >> 1;
        const double d = (best.jd & 1) ? -1.0 : 1.0;
        for (int i = tid; i < m; i += kHeurNT) s[i] = s[i] + d * a.A[(size_t)i * n + j];
        if (tid == 0) xt[j] = xt[j] + d;
        lift++;
        __syncthreads();
    }
    for (int j = tid; j < n; j += kHeurNT) xo[j] = xt[j];
    if (tid == 0) {
        double obj = 0.0;
        for (int j = 0; j < n; j++) obj += a.c[j] * xt[j];
        a.obj_out[p] = obj;
        a.status_out[p] = status;
        a.moves_out[2 * p] = repair;
        a.moves_out[2 * p + 1] = lift;
    }
}

}  // namespace mipx
