// prop_kernels.hip.h -- the bound propagation of include/mipx_prop.h: tighten the bounds of a node's integer
// columns from the row activities, the objective cutoff as one more row.
//
//   prop_bounds   one workgroup of 256 threads (4 waves) per node.  The node's l and u, the rows' right-hand
//                 sides, their activities S_i and infinite-term counts ninf_i and the integer mask live in LDS
//                 (about 37 KiB at 1024 x 1024).  A round has two phases.  Activity: one wave per row in turn, the
//                 lanes stride the columns (row-major A: coalesced), the sum is reduced inside the wave.
//                 Candidates: one thread per column (columns above 256: in turn), each walks the rows (neighbouring
//                 threads read neighbouring a_ij: coalesced) with its running max and min in registers.  A thread
//                 reads and writes the bounds of its own columns only in that phase, so the round is a Jacobi
//                 round without a second copy.  The round's change count and conflict flag go through LDS; the
//                 kernel uses no atomics.
//
// Products are not fused (the library is built with -ffp-contract=off); the sum of a row runs in the kernel's own
// order, which gives the same bits as any other on integer data (mipx_prop.h).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace mipx {

constexpr int kPropNT = 256;     // threads per workgroup
constexpr int kPropMax = 1024;   // rows and columns at most (what the LP kernels take)
constexpr int kPropOwn = kPropMax / kPropNT;   // columns per thread at most

struct PropArgs {
    int m, n, n_int, max_rounds;
    int cut;                        // 1: the row (-c) x >= -cutoff takes part as row m
    double tol, cutoff;
    const double *A, *b, *c;        // the problem's rows A x >= b (m x n, row-major) and objective
    const int32_t *int_idx;         // the integer columns, n_int of them
    const int32_t *slot;            // nullable: node k's bounds are row slot[k] of l, u (else row k)
    const double *l, *u;            // the boxes, n per row
    double *l_out, *u_out;          // where the bounds go, rows as in l, u (may be l, u themselves)
    int32_t *status_out, *changed_out, *rounds_out;   // batch each
    int32_t *capped_out;            // nullable, batch: 1 where max_rounds ended a node whose last round changed a bound
};

__global__ void __launch_bounds__(kPropNT) prop_bounds(PropArgs a) {
    __shared__ double sl[kPropMax], su[kPropMax], sb[kPropMax + 1], sS[kPropMax + 1];
    __shared__ int32_t sninf[kPropMax + 1];
    __shared__ uint8_t isint[kPropMax];
    __shared__ int32_t wcnt[kPropNT / 64], wconf[kPropNT / 64], rowconf;
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = a.m, n = a.n, mt = a.m + (a.cut ? 1 : 0);
    const double tol = a.tol;
    const size_t row = a.slot ? (size_t)a.slot[p] : (size_t)p;
    const double *l = a.l + row * n, *u = a.u + row * n;
    double *lo = a.l_out + row * n, *uo = a.u_out + row * n;
    for (int j = tid; j < n; j += kPropNT) { sl[j] = l[j]; su[j] = u[j]; isint[j] = 0; }
    for (int i = tid; i < m; i += kPropNT) sb[i] = a.b[i];
    if (tid == 0 && a.cut) sb[m] = -a.cutoff;
    __syncthreads();
    for (int k = tid; k < a.n_int; k += kPropNT) isint[a.int_idx[k]] = 1;
    int status = 0, changed = 0, rounds = 0, capped = 0;
    for (int r = 0; r < a.max_rounds; r++) {
        rounds++;
        if (tid == 0) rowconf = 0;
        __syncthreads();   // (the mask, the flag and the bounds of the last round are in place)
        // activity: S_i and ninf_i of every row from the bounds the round starts with
        for (int i = wave; i < mt; i += kPropNT / 64) {
            const double *ar = i < m ? a.A + (size_t)i * n : a.c;
            const double sg = i < m ? 1.0 : -1.0;
            double s = 0.0;
            int ni = 0;
            for (int j = lane; j < n; j += 64) {
                const double aij = sg * ar[j];
                if (aij == 0.0) continue;
                const double h = aij > 0.0 ? aij * su[j] : aij * sl[j];
                if (isinf(h)) ni++;
                else s += h;
            }
            for (int off = 32; off > 0; off >>= 1) {
                s += __shfl_xor(s, off, 64);
                ni += __shfl_xor(ni, off, 64);
            }
            if (lane == 0) {
                sS[i] = s;
                sninf[i] = ni;
                if (ni == 0 && s < sb[i] - tol) rowconf = 1;
            }
        }
        __syncthreads();
        if (rowconf) { status = 2; break; }   // (uniform over the workgroup)
        // candidates: the thread's columns against every row; the new bounds go straight to LDS, which no other
        // thread reads before the next round
        int cnt = 0, conf = 0;
        for (int j = tid; j < n; j += kPropNT) {
            if (!isint[j]) continue;
            const double lj = sl[j], uj = su[j];
            double nl = lj, nu = uj;
            for (int i = 0; i < mt; i++) {
                const double aij = i < m ? a.A[(size_t)i * n + j] : -a.c[j];
                if (aij == 0.0) continue;
                const int ni = sninf[i];
                if (ni > 1) continue;
                const double h = aij > 0.0 ? aij * uj : aij * lj;
                const bool hinf = isinf(h);
                if (ni == 1 && !hinf) continue;
                const double rest = hinf ? sS[i] : sS[i] - h;
                const double q = (sb[i] - rest) / aij;
                if (aij > 0.0) {
                    const double cand = ceil(q - tol) + 0.0;   // (+ 0.0: a zero candidate is +0)
                    if (cand > nl) nl = cand;
                } else {
                    const double cand = floor(q + tol) + 0.0;
                    if (cand < nu) nu = cand;
                }
            }
            cnt += (nl != lj) + (nu != uj);
            if (nl > nu) conf = 1;
            sl[j] = nl;
            su[j] = nu;
        }
        for (int off = 32; off > 0; off >>= 1) {
            cnt += __shfl_xor(cnt, off, 64);
            conf |= __shfl_xor(conf, off, 64);
        }
        if (lane == 0) { wcnt[wave] = cnt; wconf[wave] = conf; }
        __syncthreads();
        cnt = 0; conf = 0;
        for (int w = 0; w < kPropNT / 64; w++) { cnt += wcnt[w]; conf |= wconf[w]; }
        // (the slots are written again behind the next round's two barriers)
        if (conf) { status = 2; break; }
        changed += cnt;
        if (cnt == 0) break;
        if (r == a.max_rounds - 1) capped = 1;
    }
    if (status == 2) {   // an infeasible node keeps the bounds it came with
        if (lo != l)
            for (int j = tid; j < n; j += kPropNT) { lo[j] = l[j]; uo[j] = u[j]; }
    } else {
        __syncthreads();
        if (changed > 0 || lo != l)
            for (int j = tid; j < n; j += kPropNT) { lo[j] = sl[j]; uo[j] = su[j]; }
        status = changed > 0 ? 1 : 0;
    }
    if (tid == 0) {
        a.status_out[p] = status;
        a.changed_out[p] = changed;
        a.rounds_out[p] = rounds;
        if (a.capped_out) a.capped_out[p] = capped;
    }
}

}  // namespace mipx
