// lpdive_kernels.hip.h -- the kernels of include/mipx_lpdive.h around the node-LP launches of an LP dive: fix one
// integer column per point, re-solve the batch, repeat.
//
//   lpdive_locks     once per problem: for the integer column at position k of int_idx the number of rows with a
//                    positive and with a negative coefficient (rule 1's down_j and up_j); one thread per column.
//   lpdive_prepare   one workgroup of 256 threads per point: PREPARE.  The point's first box (L, U), its row of basis
//                    codes (the caller's, or all 0), the per-point state, and the point itself copied to x_out (what
//                    every point that does not end FEASIBLE returns).  A skipped point gets L = U = L0.
//   lpdive_step      one workgroup of ONE wave per point: STEP of round r.  It reads the LP's outputs for its point,
//                    copies the n + m basis codes forward only where the LP ended optimal, flips or selects -- the
//                    argmin over int_idx is a wave reduction by __shfl_xor on the key (lock count, fractionality,
//                    position), no LDS, no barrier -- and writes the one changed column, or all columns on FINAL or
//                    for a point that ends.  A point that has ended returns at once.
//   lpdive_finish    one workgroup of 256 threads per point: FINISH and the outputs, through the completion's
//                    complete_finish_point (complete_kernels.hip.h) on the FINAL LP's point.
//
// Between them the node-LP kernels run unchanged (K1 / K1b through launch_lp_any, on the same stream).  Plain vector
// stores only; the one atomic is a vector atomicAdd on the round's counter of live points, which only the batch entry
// reads.  No scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "complete_kernels.hip.h"
#include "step_layout.h"

namespace mipx {

constexpr int kLpdiveNT = kCompNT;      // threads per workgroup of prepare and finish (the completion's: its FINISH is shared)
constexpr int kLpdiveWave = 64;         // threads per workgroup of the step: one wave
constexpr int kLpdiveMax = kCompMax;    // rows and columns at most (what the LP kernels take)
constexpr int kLpdiveMaxRounds = 1024;
// phases of a point
constexpr int kLpdiveActive = 0, kLpdiveFinal = 1, kLpdivePending = 2, kLpdiveEnded = 3;

// The dive's workspace for `batch` points of n columns and m rows: [L | U | the LP's x] (f64, batch x n each), [the
// codes the LP starts from | the codes it ends on] (i8, batch x (n + m) each), per point the LP's [objective] (f64) and
// [status | pivots] (i32), the record of the last fixing [old L | old U | v | x_j] (f64) and [column] (i32), the [phase]
// (i32), and the counter of live points per round (i32, kLpdiveMaxRounds + 2); every block 256-byte aligned.
struct LpdiveWs {
    size_t L, U, x, vin, vout, lp_obj, lp_status, lp_pivots, rec, rec_j, phase, live, end;
    static size_t up(size_t v) { return (v + 255) / 256 * 256; }
    LpdiveWs(size_t batch, size_t m, size_t n)
        : L(0), U(up(L + 8 * batch * n)), x(up(U + 8 * batch * n)), vin(up(x + 8 * batch * n)),
          vout(up(vin + batch * (n + m))), lp_obj(up(vout + batch * (n + m))), lp_status(up(lp_obj + 8 * batch)),
          lp_pivots(up(lp_status + 4 * batch)), rec(up(lp_pivots + 4 * batch)), rec_j(up(rec + 32 * batch)),
          phase(up(rec_j + 4 * batch)), live(up(phase + 4 * batch)), end(up(live + 4 * (kLpdiveMaxRounds + 2))) {}
    size_t bytes() const { return end; }
};

// What comes down with a step of the search, cap points: [obj] (f64) [status | rounds | fixings | flips | pivots] (i32);
// view(base) as the layouts of step_layout.h have it (host-usable: no device code).
struct LpdiveOut {
    size_t obj, status, rounds, fixings, flips, pivots, end;
    explicit LpdiveOut(size_t cap)
        : obj(0), status(8 * cap), rounds(status + 4 * cap), fixings(rounds + 4 * cap), flips(fixings + 4 * cap),
          pivots(flips + 4 * cap), end(pivots + 4 * cap) {}
    size_t bytes() const { return end; }
    template <class Base> struct View {
        step_layout::Like<double, Base> *obj;
        step_layout::Like<int32_t, Base> *status, *rounds, *fixings, *flips, *pivots;
    };
    template <class Base> View<Base> view(Base *b) const {
        using step_layout::at;
        return {at<double>(b, obj), at<int32_t>(b, status), at<int32_t>(b, rounds), at<int32_t>(b, fixings),
                at<int32_t>(b, flips), at<int32_t>(b, pivots)};
    }
};

struct LpdiveArgs {
    int m, n, n_int;
    int rule, round, max_rounds;    // round: 1 .. max_rounds + 1 (step)
    double cutoff, ftol, ctol;
    const double *A, *b, *c;        // the problem's rows A x >= b (m x n, row-major) and objective
    const int32_t *int_idx;         // the integer columns, n_int of them
    const int32_t *locks;           // [down (n_int) | up (n_int)], by position in int_idx (lpdive_locks)
    const double *x0;               // the points, batch x n
    const double *l0, *u0;          // the boxes: row (slot ? slot[q] : q) of n columns each
    const int32_t *slot;            // nullable: the pool row of point q's box
    const uint8_t *skip;            // nullable: a point whose entry is not 0 is skipped
    const int32_t *gate;            // nullable: the status of the node LP a point came from; not 0: skipped
    const int8_t *vstat;            // nullable: n + m basis codes per point
    double *ws_L, *ws_U;
    double *ws_x;
    int8_t *ws_vin;
    const int8_t *ws_vout;
    const double *ws_lp_obj;
    const int32_t *ws_lp_status, *ws_lp_pivots;
    double *ws_rec;
    int32_t *ws_rec_j, *ws_phase, *ws_live;
    double *x_out, *obj_out;        // batch x n, batch
    int32_t *status_out, *rounds_out, *fixings_out, *flips_out, *pivots_out;
};

__global__ void __launch_bounds__(256) lpdive_locks(int m, int n, int n_int, const double *A, const int32_t *int_idx, int32_t *locks) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n_int) return;
    const int j = int_idx[k];
    int down = 0, up = 0;
    for (int i = 0; i < m; i++) {
        const double v = A[(size_t)i * n + j];
        down += v > 0.0 ? 1 : 0;
        up += v < 0.0 ? 1 : 0;
    }
    locks[k] = down;
    locks[n_int + k] = up;
}

__global__ void __launch_bounds__(kLpdiveNT) lpdive_prepare(LpdiveArgs a) {
    const int q = blockIdx.x, tid = threadIdx.x, n = a.n, nv = a.n + a.m;
    const size_t g = (size_t)q, row = a.slot ? (size_t)a.slot[q] : g;
    const double *x = a.x0 + g * n, *l0 = a.l0 + row * n, *u0 = a.u0 + row * n;
    double *L = a.ws_L + g * n, *U = a.ws_U + g * n, *xo = a.x_out + g * n;
    int bad = ((a.skip && a.skip[q]) || (a.gate && a.gate[q] != 0)) ? 1 : 0;   // (uniform over the workgroup)
    for (int j = tid; j < n; j += kLpdiveNT)
        if (!isfinite(x[j])) bad = 1;
    for (int k = tid; k < a.n_int; k += kLpdiveNT) {
        const int j = a.int_idx[k];
        const double lo = l0[j], hi = u0[j];
        if (!isfinite(lo) || !isfinite(hi) || fabs(lo - rint(lo)) > a.ctol || fabs(hi - rint(hi)) > a.ctol) bad = 1;
    }
    bad = __syncthreads_or(bad);
    for (int j = tid; j < n; j += kLpdiveNT) {
        const double lj = l0[j];
        L[j] = lj;
        U[j] = bad ? lj : u0[j];
        xo[j] = x[j];
    }
    __syncthreads();   // (the integer columns over the rows just written: the same threads need not own them)
    if (!bad)
        for (int k = tid; k < a.n_int; k += kLpdiveNT) {
            const int j = a.int_idx[k];
            L[j] = rint(l0[j]);
            U[j] = rint(u0[j]);
        }
    int8_t *vo = a.ws_vin + g * (size_t)nv;
    const int8_t *vi = (a.vstat && !bad) ? a.vstat + g * (size_t)nv : nullptr;
    for (int v = tid; v < nv; v += kLpdiveNT) vo[v] = vi ? vi[v] : (int8_t)0;
    if (tid == 0) {
        a.ws_phase[g] = bad ? kLpdiveEnded : kLpdiveActive;
        a.ws_rec_j[g] = -1;
        a.status_out[g] = bad ? 3 : 2;   // (SKIPPED; any other point is LIMIT until STEP says otherwise)
        a.obj_out[g] = 0.0;
        a.rounds_out[g] = 0; a.fixings_out[g] = 0; a.flips_out[g] = 0; a.pivots_out[g] = 0;
    }
}

// The smaller of two keys (lock, frac, pos) in that order; pos < 0: no candidate.
__device__ __forceinline__ void lpdive_key_min(int &lock, double &frac, int &pos, int lock2, double frac2, int pos2) {
    const bool take = pos2 >= 0 && (pos < 0 || lock2 < lock || (lock2 == lock && (frac2 < frac || (frac2 == frac && pos2 < pos))));
    if (take) { lock = lock2; frac = frac2; pos = pos2; }
}

__global__ void __launch_bounds__(kLpdiveWave) lpdive_step(LpdiveArgs a) {
    const int q = blockIdx.x, lane = threadIdx.x, n = a.n, nv = a.n + a.m, n_int = a.n_int;
    const size_t g = (size_t)q;
    int phase = a.ws_phase[g];
    if (phase >= kLpdivePending) return;   // (ended, or waiting for FINISH: its box is fixed at L0)
    const size_t row = a.slot ? (size_t)a.slot[q] : g;
    double *L = a.ws_L + g * n, *U = a.ws_U + g * n;
    const double *x = a.round == 1 ? a.x0 + g * n : a.ws_x + g * n;
    const bool last = a.round > a.max_rounds;
    int end = -1;          // the status the point ends with (-1: it goes on)
    bool select = true;
    if (a.round > 1) {
        const int lp = a.ws_lp_status[g];
        if (lane == 0) a.pivots_out[g] += a.ws_lp_pivots[g];
        if (lp == 0) {
            int8_t *vi = a.ws_vin + g * (size_t)nv;
            const int8_t *vo = a.ws_vout + g * (size_t)nv;
            for (int v = lane; v < nv; v += kLpdiveWave) vi[v] = vo[v];
            if (!(a.ws_lp_obj[g] < a.cutoff)) end = 5;
            else if (phase == kLpdiveFinal) {
                // to FINISH: the candidate is the LP's point with the integer columns exactly as they were fixed
                double *xo = a.x_out + g * n;
                for (int j = lane; j < n; j += kLpdiveWave) xo[j] = x[j];
                __syncthreads();
                for (int k = lane; k < n_int; k += kLpdiveWave) { const int j = a.int_idx[k]; xo[j] = L[j]; }
                phase = kLpdivePending;
                select = false;
            }
        } else if (lp != 1) end = 2;
        else {
            const int rj = a.ws_rec_j[g];
            if (rj < 0) end = 1;
            else if (last) end = 2;
            else {   // FLIP (every lane computes it; lane 0 writes)
                const double *rec = a.ws_rec + 4 * g;
                const double oldL = rec[0], oldU = rec[1], v = rec[2], xj = rec[3];
                const double lo = v <= xj ? v + 1.0 : oldL, hi = v <= xj ? oldU : v - 1.0;
                if (lo > hi) end = 1;
                else if (lane == 0) {
                    L[rj] = lo; U[rj] = hi;
                    a.ws_rec_j[g] = -1;
                    a.flips_out[g] += 1;
                }
                select = false;
            }
        }
    }
    if (end < 0 && select && last) end = 2;
    if (end < 0 && select) {
        // SELECT: the wave's argmin over the candidates
        int lock = 0, pos = -1;
        double frac = 0.0;
        for (int k = lane; k < n_int; k += kLpdiveWave) {
            const int j = a.int_idx[k];
            if (!(L[j] < U[j])) continue;
            const double f = fabs(x[j] - rint(x[j]));
            if (!(f > a.ftol)) continue;
            const int down = a.locks[k], up = a.locks[n_int + k];
            lpdive_key_min(lock, frac, pos, a.rule == 1 ? (down < up ? down : up) : 0, f, k);
        }
        for (int off = kLpdiveWave / 2; off > 0; off >>= 1) {
            const int lock2 = __shfl_xor(lock, off, kLpdiveWave), pos2 = __shfl_xor(pos, off, kLpdiveWave);
            const double frac2 = __shfl_xor(frac, off, kLpdiveWave);
            lpdive_key_min(lock, frac, pos, lock2, frac2, pos2);
        }
        if (pos < 0) {   // every integer column is integral: fix them all, the next LP is the completion's
            for (int k = lane; k < n_int; k += kLpdiveWave) {
                const int j = a.int_idx[k];
                const double lo = L[j], hi = U[j];
                if (!(lo < hi)) continue;
                double v = floor(x[j] + 0.5);
                v = v < lo ? lo : v > hi ? hi : v;
                L[j] = v; U[j] = v;
            }
            phase = kLpdiveFinal;
            if (lane == 0) a.ws_rec_j[g] = -1;
        } else if (lane == 0) {
            const int j = a.int_idx[pos];
            const double xj = x[j], lo = L[j], hi = U[j];
            double v = floor(xj + 0.5);
            if (a.rule == 1) {
                const int down = a.locks[pos], up = a.locks[n_int + pos];
                if (down < up) v = floor(xj);
                else if (up < down) v = ceil(xj);
            }
            v = v < lo ? lo : v > hi ? hi : v;
            double *rec = a.ws_rec + 4 * g;
            rec[0] = lo; rec[1] = hi; rec[2] = v; rec[3] = xj;
            a.ws_rec_j[g] = j;
            L[j] = v; U[j] = v;
            a.fixings_out[g] += 1;
        }
    }
    if (end >= 0 || phase == kLpdivePending) {
        // the point ends, or waits for FINISH: every column fixed at L0, no basis -- its remaining LPs end without a pivot
        const double *l0 = a.l0 + row * n;
        for (int j = lane; j < n; j += kLpdiveWave) { const double lj = l0[j]; L[j] = lj; U[j] = lj; }
        int8_t *vi = a.ws_vin + g * (size_t)nv;
        for (int v = lane; v < nv; v += kLpdiveWave) vi[v] = 0;
        if (lane == 0) {
            a.ws_phase[g] = end >= 0 ? kLpdiveEnded : kLpdivePending;
            if (end >= 0) a.status_out[g] = end;
        }
        return;
    }
    if (lane == 0) {
        a.ws_phase[g] = phase;
        a.rounds_out[g] += 1;
        atomicAdd(a.ws_live + a.round, 1);
    }
}

__global__ void __launch_bounds__(kLpdiveNT) lpdive_finish(LpdiveArgs a) {
    __shared__ double xt[kLpdiveMax];
    __shared__ uint8_t isint[kLpdiveMax];
    const int q = blockIdx.x, tid = threadIdx.x, n = a.n;
    const size_t g = (size_t)q, row = a.slot ? (size_t)a.slot[q] : g;
    if (a.ws_phase[g] != kLpdivePending) return;   // (uniform; status_out holds the verdict, x_out the input point)
    double *xo = a.x_out + g * n;
    double obj = 0.0;
    const int bad = complete_finish_point(a.m, n, a.n_int, a.ctol, a.A, a.b, a.c, a.l0 + row * n, a.u0 + row * n, a.int_idx,
                                          xo, xo, xo, &obj, xt, isint);
    if (bad) {
        const double *x = a.x0 + g * n;
        for (int j = tid; j < n; j += kLpdiveNT) xo[j] = x[j];
    }
    if (tid == 0) {
        a.obj_out[g] = obj;
        a.status_out[g] = bad ? 4 : 0;
    }
}

}  // namespace mipx
