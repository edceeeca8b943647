// fixprop_kernels.hip.h -- the fix-and-propagate dive of include/mipx_fixprop.h: fix the integer columns of an LP
// point one after the other, each to the nearest value the bound propagation does not refuse.
//
//   fixprop_dive   one workgroup of 256 threads (4 waves) per point.  The working box, the trial box, the guide x,
//                  the rows' right-hand sides, activities and infinite-term counts and the integer mask live in LDS
//                  (about 61 KiB at 1024 x 1024: two workgroups per CU).  A fixing copies the working box into the
//                  trial box with the column fixed and runs the rounds of prop_bounds on it (fixprop_rounds: the
//                  same two phases and the same arithmetic, restated here so that prop_bounds stays as it is); a
//                  trial that ends infeasible is simply dropped, one that does not is copied back.  The column to
//                  fix is an arg-min over the integer columns (__shfl_xor inside a wave, one LDS slot per wave
//                  across them); the walk over its values is the same few scalar operations in every thread.
//                  Every branch is taken from values in LDS behind a barrier, so the whole workgroup takes it.
//                  Plain vector stores, no atomics, no scratch.
//
// Products are not fused (the library is built with -ffp-contract=off); the sums of END and obj run in the order
// mipx_fixprop.h states, the activity of a row in prop_bounds' order.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace mipx {

constexpr int kFpNT = 256;     // threads per workgroup
constexpr int kFpMax = 1024;   // rows and columns at most (what the LP kernels take)
constexpr int kFpNone = 0x7fffffff;
constexpr int kFpRows = 4;     // rows a wave sums at once in the activity phase

struct FixpropArgs {
    int m, n, n_int, max_rounds, max_tries;
    int cut;                        // 1: the row (-c) x >= -cutoff takes part as row m
    double tol, cutoff;
    const double *A, *b, *c;        // the problem's rows A x >= b (m x n, row-major) and objective
    const double *l, *u;            // the root's bounds, n each
    const int32_t *int_idx;         // the integer columns, n_int of them
    const double *x;                // batch x n: the points
    const uint8_t *skip;            // nullable: a point whose entry is not 0 is skipped (x copied, obj 0)
    const int32_t *gate;            // nullable, the status of the heuristic that tried the point first: a point whose
                                    // entry is not 1 or 2 (stuck, capped) is skipped and neither x_out nor obj_out is touched
    double *x_out, *obj_out;        // batch x n, batch
    int32_t *status_out, *counts_out;   // batch, 2 x batch (fixings, tries)
};

// what the rounds of a propagation share: the rows' right-hand sides, activities and infinite-term counts, the
// integer mask, and the slots the round's counts and flags go through
struct FixpropLds {
    double *sb, *sS;
    int32_t *sninf;
    const uint8_t *isint;
    int32_t *wcnt, *wconf, *rowconf;
};

// The rounds of prop_bounds (ONE ROUND to STOP of mipx_prop.h) on the box bl, bu in LDS, in place.  Returns 2 when
// the box is infeasible (its contents are then of no use), else 0; the same value in every thread.  On return the
// box is visible to the whole workgroup.
__device__ inline int fixprop_rounds(const FixpropArgs &a, const FixpropLds &s, double *bl, double *bu) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = a.m, n = a.n, mt = a.m + (a.cut ? 1 : 0);
    const double tol = a.tol;
    for (int r = 0; r < a.max_rounds; r++) {
        __syncthreads();   // (the box is in place, and the flag of the last round or call has been read)
        if (tid == 0) *s.rowconf = 0;
        __syncthreads();
        // activity: S_i and ninf_i of every row from the bounds the round starts with.  A wave takes four of its rows
        // at once (rows i0, i0 + 4, i0 + 8, i0 + 12), so that their loads are in flight together; each row's sum keeps
        // prop_bounds' order (lanes stride the columns, then the butterfly)
        for (int i0 = wave; i0 < mt; i0 += kFpRows * (kFpNT / 64)) {
            double sum[kFpRows];
            int ni[kFpRows];
#pragma unroll
            for (int q = 0; q < kFpRows; q++) { sum[q] = 0.0; ni[q] = 0; }
            for (int j = lane; j < n; j += 64) {
                const double lj = bl[j], uj = bu[j];
#pragma unroll
                for (int q = 0; q < kFpRows; q++) {
                    const int i = i0 + q * (kFpNT / 64);
                    if (i >= mt) continue;
                    const double aij = i < m ? a.A[(size_t)i * n + j] : -1.0 * a.c[j];
                    if (aij == 0.0) continue;
                    const double h = aij > 0.0 ? aij * uj : aij * lj;
                    if (isinf(h)) ni[q]++;
                    else sum[q] += h;
                }
            }
#pragma unroll
            for (int q = 0; q < kFpRows; q++) {
                const int i = i0 + q * (kFpNT / 64);
                for (int off = 32; off > 0; off >>= 1) {
                    sum[q] += __shfl_xor(sum[q], off, 64);
                    ni[q] += __shfl_xor(ni[q], off, 64);
                }
                if (lane == 0 && i < mt) {
                    s.sS[i] = sum[q];
                    s.sninf[i] = ni[q];
                    if (ni[q] == 0 && sum[q] < s.sb[i] - tol) *s.rowconf = 1;
                }
            }
        }
        __syncthreads();
        if (*s.rowconf) return 2;
        // candidates: the thread's columns against every row; the new bounds go straight to LDS, which no other
        // thread reads before the next round
        int cnt = 0, conf = 0;
        for (int j = tid; j < n; j += kFpNT) {
            if (!s.isint[j]) continue;
            const double lj = bl[j], uj = bu[j];
            double nl = lj, nu = uj;
            for (int i = 0; i < mt; i++) {
                const int ni = s.sninf[i];
                if (ni > 1) continue;
                const double aij = i < m ? a.A[(size_t)i * n + j] : -a.c[j];
                if (aij == 0.0) continue;
                const double h = aij > 0.0 ? aij * uj : aij * lj;
                const bool hinf = isinf(h);
                if (ni == 1 && !hinf) continue;
                const double rest = hinf ? s.sS[i] : s.sS[i] - h;
                const double num = s.sb[i] - rest;
                // the candidate is ceil(q - tol) < q + 1 or floor(q + tol) > q - 1 with q = num / a_ij: a q two units
                // on the far side of the bound held so far cannot move it, and is not divided out (the test's own
                // rounding is some 1e-16 of that bound against a whole unit of room)
                if (aij > 0.0) {
                    if (num <= aij * (nl - 2.0)) continue;
                    const double cand = ceil(num / aij - tol) + 0.0;   // (+ 0.0: a zero candidate is +0)
                    if (cand > nl) nl = cand;
                } else {
                    if (num <= aij * (nu + 2.0)) continue;
                    const double cand = floor(num / aij + tol) + 0.0;
                    if (cand < nu) nu = cand;
                }
            }
            cnt += (nl != lj) + (nu != uj);
            if (nl > nu) conf = 1;
            bl[j] = nl;
            bu[j] = nu;
        }
        for (int off = 32; off > 0; off >>= 1) {
            cnt += __shfl_xor(cnt, off, 64);
            conf |= __shfl_xor(conf, off, 64);
        }
        if (lane == 0) { s.wcnt[wave] = cnt; s.wconf[wave] = conf; }
        __syncthreads();
        cnt = 0; conf = 0;
        for (int w = 0; w < kFpNT / 64; w++) { cnt += s.wcnt[w]; conf |= s.wconf[w]; }
        // (the slots are written again behind the next round's three barriers)
        if (conf) return 2;
        if (cnt == 0) break;
    }
    return 0;
}

__global__ void __launch_bounds__(kFpNT) fixprop_dive(FixpropArgs a) {
    __shared__ double wl[kFpMax], wu[kFpMax], tl[kFpMax], tu[kFpMax], sx[kFpMax], sb[kFpMax + 1], sS[kFpMax + 1];
    __shared__ int32_t sninf[kFpMax + 1];
    __shared__ uint8_t isint[kFpMax];
    __shared__ int32_t wcnt[kFpNT / 64], wconf[kFpNT / 64], rowconf;
    __shared__ double pickf[kFpNT / 64];
    __shared__ int32_t pickj[kFpNT / 64];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = a.m, n = a.n;
    const double tol = a.tol;
    const double *x = a.x + (size_t)p * n;
    double *xo = a.x_out + (size_t)p * n;
    if (a.gate && a.gate[p] != 1 && a.gate[p] != 2) {   // (uniform over the workgroup)
        if (tid == 0) {
            a.status_out[p] = 3;
            a.counts_out[2 * p] = 0;
            a.counts_out[2 * p + 1] = 0;
        }
        return;
    }
    if (a.skip && a.skip[p]) {
        if (xo != x)
            for (int j = tid; j < n; j += kFpNT) xo[j] = x[j];
        if (tid == 0) {
            a.obj_out[p] = 0.0;
            a.status_out[p] = 3;
            a.counts_out[2 * p] = 0;
            a.counts_out[2 * p + 1] = 0;
        }
        return;
    }
    const FixpropLds s{sb, sS, sninf, isint, wcnt, wconf, &rowconf};
    // START: the root box with the integer columns' bounds rounded, into the trial box, and propagated
    for (int j = tid; j < n; j += kFpNT) { sx[j] = x[j]; tl[j] = a.l[j]; tu[j] = a.u[j]; isint[j] = 0; }
    for (int i = tid; i < m; i += kFpNT) sb[i] = a.b[i];
    if (tid == 0 && a.cut) sb[m] = -a.cutoff;
    __syncthreads();
    for (int k = tid; k < a.n_int; k += kFpNT) {
        const int j = a.int_idx[k];
        isint[j] = 1;
        tl[j] = ceil(a.l[j] - tol) + 0.0;
        tu[j] = floor(a.u[j] + tol) + 0.0;
    }
    int status = 0, fixings = 0, tries = 0;
    if (fixprop_rounds(a, s, tl, tu) == 2) status = 4;
    while (status == 0) {
        // the trial box is the working box from here on
        __syncthreads();
        for (int j = tid; j < n; j += kFpNT) { wl[j] = tl[j]; wu[j] = tu[j]; }
        __syncthreads();
        // PICK: the smallest (|x^_j - rint(x^_j)|, j) over the integer columns that are not fixed
        double bf = 0.0;
        int bj = kFpNone;
        for (int k = tid; k < a.n_int; k += kFpNT) {
            const int j = a.int_idx[k];
            const double L = wl[j], U = wu[j];
            if (!(L < U)) continue;
            const double xh = fmin(fmax(sx[j], L), U);
            const double f = fabs(xh - rint(xh));
            if (bj == kFpNone || f < bf || (f == bf && j < bj)) { bf = f; bj = j; }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const double of = __shfl_xor(bf, off, 64);
            const int oj = __shfl_xor(bj, off, 64);
            if (oj != kFpNone && (bj == kFpNone || of < bf || (of == bf && oj < bj))) { bf = of; bj = oj; }
        }
        if (lane == 0) { pickf[wave] = bf; pickj[wave] = bj; }
        __syncthreads();
        bf = pickf[0]; bj = pickj[0];
        for (int w = 1; w < kFpNT / 64; w++) {
            const double of = pickf[w];
            const int oj = pickj[w];
            if (oj != kFpNone && (bj == kFpNone || of < bf || (of == bf && oj < bj))) { bf = of; bj = oj; }
        }
        // (the slots are written again behind the barriers of the propagation below)
        if (bj == kFpNone) break;   // every integer column is fixed: END
        // VALUES: the integers of [L_j, U_j] in ascending (|w - x^_j|, w), the first the propagation does not refuse
        const int j = bj;
        const double L = wl[j], U = wu[j];
        const double xh = fmin(fmax(sx[j], L), U);
        double dn = floor(xh), up = dn + 1.0;
        for (;;) {
            const bool dn_ok = dn >= L, up_ok = up <= U;
            if (!dn_ok && !up_ok) { status = 1; break; }
            double w;
            if (dn_ok && (!up_ok || xh - dn <= up - xh)) { w = dn; dn = dn - 1.0; }
            else { w = up; up = up + 1.0; }
            if (tries == a.max_tries) { status = 2; break; }
            tries++;
            __syncthreads();   // (the trial box of the last try has been read by its last round)
            for (int q = tid; q < n; q += kFpNT) {
                const bool fix = q == j;
                tl[q] = fix ? w + 0.0 : wl[q];
                tu[q] = fix ? w + 0.0 : wu[q];
            }
            if (fixprop_rounds(a, s, tl, tu) != 2) { fixings++; break; }
        }
    }
    if (status != 0) {
        if (xo != x)
            for (int j = tid; j < n; j += kFpNT) xo[j] = sx[j];
        if (tid == 0) {
            a.obj_out[p] = 0.0;
            a.status_out[p] = status;
            a.counts_out[2 * p] = fixings;
            a.counts_out[2 * p + 1] = tries;
        }
        return;
    }
    // END: the point of the final box (in wl, wu), its rows in the heuristic's order
    __syncthreads();
    for (int j = tid; j < n; j += kFpNT) tl[j] = isint[j] ? wl[j] : fmin(fmax(sx[j], wl[j]), wu[j]);
    if (tid == 0) rowconf = 0;
    __syncthreads();
    int bad = 0;
    for (int i = tid; i < m; i += kFpNT) {
        const double *row = a.A + (size_t)i * n;
        double acc = 0.0;
        for (int j = 0; j < n; j++) acc += row[j] * tl[j];
        if (!(acc - sb[i] >= -tol)) bad = 1;
    }
    if (bad) rowconf = 1;   // (every writer stores the same value)
    __syncthreads();
    status = rowconf ? 5 : 0;
    for (int j = tid; j < n; j += kFpNT) xo[j] = tl[j];
    if (tid == 0) {
        double obj = 0.0;
        for (int j = 0; j < n; j++) obj += a.c[j] * tl[j];
        a.obj_out[p] = obj;
        a.status_out[p] = status;
        a.counts_out[2 * p] = fixings;
        a.counts_out[2 * p + 1] = tries;
    }
}

}  // namespace mipx
