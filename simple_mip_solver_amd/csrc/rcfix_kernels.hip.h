// rcfix_kernels.hip.h -- the reduced-cost bound tightening of include/mipx_rcfix.h: from a node's row duals and an
// objective cutoff, tighter bounds for its integer columns.
//
//   rc_tighten    one workgroup of 256 threads (4 waves) per node.  yp, b, the box and the integer mask live in
//                 LDS (about 35 KiB).  Reduced costs: one thread per column (columns above 256: the thread owns
//                 columns tid, tid + 256, ..., their d_j in registers), walking the rows ascending; neighbouring
//                 threads read neighbouring a_ij of the row-major A (coalesced), yp_i is an LDS broadcast, and a
//                 row with yp_i = 0 is skipped by the whole workgroup.  yp . b is summed by one thread, rows
//                 ascending; the terms t_j by 256 partial sums and a fixed fold in LDS (mipx_rcfix.h states the
//                 order).  A thread reads and writes the bounds of its own columns only, so the output may be the
//                 input; a node whose bounds do not change writes nothing back.  No atomics.
//
// Products are not fused (the library is built with -ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace mipx {

constexpr int kRcNT = 256;     // threads per workgroup
constexpr int kRcMax = 1024;   // rows and columns at most (what the LP kernels take)
constexpr int kRcOwn = kRcMax / kRcNT;   // columns per thread at most

struct RcArgs {
    int m, n, n_int;
    double cutoff, tol, dtol;
    const double *A, *b, *c;        // the problem's rows A x >= b (m x n, row-major) and objective
    const int32_t *int_idx;         // the integer columns, n_int of them
    const int32_t *slot;            // nullable: node k's bounds are row slot[k] of l, u (else row k)
    const int32_t *pos;             // nullable: node k's duals are row pos[k] of y (else row k)
    const double *l, *u;            // the boxes, n per row
    const double *y;                // the duals, m per row
    double *l_out, *u_out;          // where the bounds go, rows as in l, u (may be l, u themselves)
    double *z_out;                  // nullable, batch: the bound z
    int32_t *status_out, *changed_out;   // batch each
};

__global__ void __launch_bounds__(kRcNT) rc_tighten(RcArgs a) {
    __shared__ double sy[kRcMax], sb[kRcMax], sl[kRcMax], su[kRcMax], red[kRcNT], syb;
    __shared__ uint8_t isint[kRcMax];
    __shared__ int32_t wcnt[kRcNT / 64];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = a.m, n = a.n;
    const double tol = a.tol, dtol = a.dtol, U = a.cutoff;
    const size_t row = a.slot ? (size_t)a.slot[p] : (size_t)p;
    const size_t yrow = a.pos ? (size_t)a.pos[p] : (size_t)p;
    const double *l = a.l + row * n, *u = a.u + row * n, *y = a.y + yrow * m;
    double *lo = a.l_out + row * n, *uo = a.u_out + row * n;
    for (int i = tid; i < m; i += kRcNT) {
        const double yi = y[i];
        sy[i] = yi > 0.0 ? yi : 0.0;   // (a NaN compares false: +0)
        sb[i] = a.b[i];
    }
    for (int j = tid; j < n; j += kRcNT) { sl[j] = l[j]; su[j] = u[j]; isint[j] = 0; }
    __syncthreads();
    for (int k = tid; k < a.n_int; k += kRcNT) isint[a.int_idx[k]] = 1;   // (read behind the fold's barriers)
    if (tid == kRcNT - 1) {   // yp . b, rows ascending from +0
        double s = 0.0;
        for (int i = 0; i < m; i++) {
            const double yi = sy[i];
            if (yi == 0.0) continue;
            s = s + yi * sb[i];
        }
        syb = s;
    }
    // reduced costs of the thread's columns, rows ascending
    double d[kRcOwn];
#pragma unroll
    for (int q = 0; q < kRcOwn; q++) {
        const int j = tid + q * kRcNT;
        d[q] = j < n ? a.c[j] : 0.0;
    }
    for (int i = 0; i < m; i++) {
        const double yi = sy[i];
        if (yi == 0.0) continue;   // (uniform over the workgroup)
        const double *ar = a.A + (size_t)i * n;
#pragma unroll
        for (int q = 0; q < kRcOwn; q++) {
            const int j = tid + q * kRcNT;
            if (j < n) d[q] = d[q] - ar[j] * yi;
        }
    }
    // the terms: the thread's columns ascending from +0, then the fixed fold
    double part = 0.0;
#pragma unroll
    for (int q = 0; q < kRcOwn; q++) {
        const int j = tid + q * kRcNT;
        if (j < n) {
            const double tj = d[q] > 0.0 ? d[q] * sl[j] : d[q] < 0.0 ? d[q] * su[j] : 0.0;
            part = part + tj;
        }
    }
    red[tid] = part;
    __syncthreads();
    for (int s = kRcNT / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const double z = syb + red[0];
    // (everything below is uniform over the workgroup until the bounds)
    int status, changed = 0;
    if (!isfinite(U) || z != z || z == -__builtin_huge_val()) {
        status = 3;
    } else {
        double g = U - z;
        if (g < -1e-6 * fmax(1.0, fabs(U))) {
            status = 2;
        } else {
            if (!(g > 0.0)) g = 0.0;
            int cnt = 0;
#pragma unroll
            for (int q = 0; q < kRcOwn; q++) {
                const int j = tid + q * kRcNT;
                if (j < n && isint[j]) {
                    const double lj = sl[j], uj = su[j];
                    double nl = lj, nu = uj;
                    if (d[q] > dtol) {
                        const double v = lj + floor(g / d[q] + tol);
                        if (v < uj) nu = v;
                    } else if (d[q] < -dtol && isfinite(uj)) {
                        const double v = uj - floor(g / (-d[q]) + tol);
                        if (v > lj) nl = v;
                    }
                    cnt += (nl != lj) + (nu != uj);
                    sl[j] = nl;   // (the thread's own columns: nobody else reads them)
                    su[j] = nu;
                }
            }
            for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
            if (lane == 0) wcnt[wave] = cnt;
            __syncthreads();   // (U and z are uniform: every thread of the workgroup is here)
            for (int w = 0; w < kRcNT / 64; w++) changed += wcnt[w];
            status = changed > 0 ? 1 : 0;
        }
    }
    // a thread wrote sl, su of its own columns and reads only those back; statuses 2 and 3 left them as they came
    if (changed > 0 || lo != l)
        for (int j = tid; j < n; j += kRcNT) { lo[j] = sl[j]; uo[j] = su[j]; }
    if (tid == 0) {
        if (a.z_out) a.z_out[p] = z;
        a.status_out[p] = status;
        a.changed_out[p] = changed;
    }
}

}  // namespace mipx
