// dualfn_kernels.hip.h -- the dual function of a frontier-engine search (include/mipx_dualfn.h).
//   dualfn_record   per solved node: d = c - A^T y, t = sum max(d,0) l + min(d,0) u; (y, t) into the store
//   dualfn_save     per infeasible node: its bounds and final basis codes (the penalised re-solve's input)
//   dualfn_gemm     V = Y W^T + t over a tile of right-hand sides (f64 FMA, i ascending per output)
//   dualfn_lineage  per right-hand side: the lineage maximum level by level, then the minimum over leaves
// No atomics and no order that depends on the launch shape: every output is the same bits whatever the
// batch, the tile or the number of right-hand sides.  Included by mipx.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mipx {

constexpr int kDfRecRB = 4;     // records per workgroup of dualfn_record (A is read once for all of them)
constexpr int kDfNT = 256;

struct DfRecordArgs {
    int m = 0, n = 0;               // rows of y, columns of A
    const double *A = nullptr;      // m x n, row-major
    const double *c = nullptr;      // n
    int count = 0;
    const int32_t *src = nullptr;   // per entry: its row of y_src
    const int32_t *lrow = nullptr;  // per entry: its row of l / u
    const int64_t *dst = nullptr;   // per entry: its record in the store
    const double *y_src = nullptr;  // rows of m
    const double *l = nullptr, *u = nullptr;   // rows of n
    double *store_y = nullptr;      // rows of m
    double *store_t = nullptr;
};

// infinite bounds as the reference's LP reports them (COIN_INFINITY = DBL_MAX): 0 x bound is 0, not NaN
__device__ inline double df_finite(double v) {
    return v == __builtin_inf() ? 1.7976931348623157e308 : v == -__builtin_inf() ? -1.7976931348623157e308 : v;
}

__global__ void __launch_bounds__(kDfNT) dualfn_record(DfRecordArgs a) {
    __shared__ double red[kDfRecRB][kDfNT];
    const int tid = threadIdx.x;
    const int e0 = blockIdx.x * kDfRecRB;
    const int ne = a.count - e0 < kDfRecRB ? a.count - e0 : kDfRecRB;
    const double *y[kDfRecRB];
    const double *lr[kDfRecRB], *ur[kDfRecRB];
    for (int r = 0; r < kDfRecRB; r++) {
        const int e = e0 + (r < ne ? r : 0);
        y[r] = a.y_src + (size_t)a.src[e] * a.m;
        lr[r] = a.l + (size_t)a.lrow[e] * a.n;
        ur[r] = a.u + (size_t)a.lrow[e] * a.n;
    }
    double part[kDfRecRB];
    for (int r = 0; r < kDfRecRB; r++) part[r] = 0.0;
    for (int j = tid; j < a.n; j += kDfNT) {
        double acc[kDfRecRB];
        for (int r = 0; r < kDfRecRB; r++) acc[r] = 0.0;
        for (int i = 0; i < a.m; i++) {   // column j of A once for the workgroup's records
            const double aij = a.A[(size_t)i * a.n + j];
            for (int r = 0; r < kDfRecRB; r++) acc[r] = fma(aij, y[r][i], acc[r]);
        }
        const double cj = a.c[j];
        for (int r = 0; r < kDfRecRB; r++) {
            const double d = cj - acc[r];
            part[r] += fmax(d, 0.0) * df_finite(lr[r][j]) + fmin(d, 0.0) * df_finite(ur[r][j]);
        }
    }
    for (int r = 0; r < kDfRecRB; r++) red[r][tid] = part[r];
    __syncthreads();
    for (int s = kDfNT / 2; s > 0; s >>= 1) {   // fixed tree: the same bits in every launch
        if (tid < s)
            for (int r = 0; r < kDfRecRB; r++) red[r][tid] += red[r][tid + s];
        __syncthreads();
    }
    for (int r = 0; r < ne; r++) {
        const int64_t d = a.dst[e0 + r];
        double *out = a.store_y + (size_t)d * a.m;
        for (int i = tid; i < a.m; i += kDfNT) out[i] = y[r][i];
        if (tid == 0) a.store_t[d] = red[r][0];
    }
}

struct DfSaveArgs {
    int n = 0, nv = 0, count = 0;
    const int32_t *lrow = nullptr;   // per entry: its row of l / u
    const int32_t *vpos = nullptr;   // per entry: its row of vstat (nv codes)
    const int64_t *dst = nullptr;    // per entry: its row of the infeasible-leaf store
    const double *l = nullptr, *u = nullptr;
    const int8_t *vstat = nullptr;
    double *out_l = nullptr, *out_u = nullptr;
    int8_t *out_v = nullptr;
};

__global__ void __launch_bounds__(kDfNT) dualfn_save(DfSaveArgs a) {
    const int e = blockIdx.x;
    if (e >= a.count) return;
    const size_t d = (size_t)a.dst[e], s = (size_t)a.lrow[e], v = (size_t)a.vpos[e];
    for (int j = threadIdx.x; j < a.n; j += kDfNT) {
        a.out_l[d * a.n + j] = a.l[s * a.n + j];
        a.out_u[d * a.n + j] = a.u[s * a.n + j];
    }
    for (int j = threadIdx.x; j < a.nv; j += kDfNT) a.out_v[d * a.nv + j] = a.vstat[v * a.nv + j];
}

// V[k R + r] = t[r] + sum_{i = 0 .. m-1} Y[r, i] W[k, i], the sum in ascending i from 0.0 (one FMA chain
// per output): a 64-record x 16-rhs tile per workgroup, 32 rows of Y and W at a time through LDS.
constexpr int kDfTR = 64, kDfTK = 16, kDfTI = 32;

struct DfGemmArgs {
    int R = 0, m = 0, K = 0;
    const double *Y = nullptr;   // R x m
    const double *T = nullptr;   // R
    const double *W = nullptr;   // K x m
    double *V = nullptr;         // K x R
};

__global__ void __launch_bounds__(kDfNT) dualfn_gemm(DfGemmArgs a) {
    __shared__ double ys[kDfTR][kDfTI + 1];
    __shared__ double ws[kDfTK][kDfTI + 1];
    const int tid = threadIdx.x;
    const int kx = tid & (kDfTK - 1), ry = tid >> 4;   // 16 x 16 threads, 4 records each
    const int r0 = blockIdx.x * kDfTR, k0 = blockIdx.y * kDfTK;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i0 = 0; i0 < a.m; i0 += kDfTI) {
        for (int q = tid; q < kDfTR * kDfTI; q += kDfNT) {
            const int rr = q / kDfTI, ii = q % kDfTI;
            const int r = r0 + rr, i = i0 + ii;
            ys[rr][ii] = (r < a.R && i < a.m) ? a.Y[(size_t)r * a.m + i] : 0.0;
        }
        for (int q = tid; q < kDfTK * kDfTI; q += kDfNT) {
            const int kk = q / kDfTI, ii = q % kDfTI;
            const int k = k0 + kk, i = i0 + ii;
            ws[kk][ii] = (k < a.K && i < a.m) ? a.W[(size_t)k * a.m + i] : 0.0;
        }
        __syncthreads();
        const int ni = a.m - i0 < kDfTI ? a.m - i0 : kDfTI;   // (the padding is never summed: bits as an untiled loop)
        for (int ii = 0; ii < ni; ii++) {
            const double w = ws[kx][ii];
            for (int q = 0; q < 4; q++) acc[q] = fma(ys[ry + 16 * q][ii], w, acc[q]);
        }
        __syncthreads();
    }
    const int k = k0 + kx;
    if (k >= a.K) return;
    for (int q = 0; q < 4; q++) {
        const int r = r0 + ry + 16 * q;
        if (r < a.R) a.V[(size_t)k * a.R + r] = a.T[r] + acc[q];
    }
}

struct DfLineageArgs {
    int R = 0, K = 0;
    double *V = nullptr;              // K x R, turned into the lineage maxima in place
    const int32_t *prec = nullptr;    // per record: the record of its nearest recorded ancestor (-1: none)
    const int32_t *order = nullptr;   // records by level (level 0: prec -1), ascending within a level
    const int32_t *lvl_off = nullptr; // nlvl + 1 offsets into order
    int nlvl = 0;
    const int32_t *leaf = nullptr;    // per leaf the record whose lineage maximum bounds it
    int nleaf = 0;
    int bare = 0;                     // leaves without any recorded ancestor: the bound is -inf
    double *out = nullptr;            // K
};

// one workgroup per right-hand side: the columns are independent, so the levels need no grid barrier
__global__ void __launch_bounds__(kDfNT) dualfn_lineage(DfLineageArgs a) {
    __shared__ double red[kDfNT];
    const int k = blockIdx.x, tid = threadIdx.x;
    double *v = a.V + (size_t)k * a.R;
    for (int L = 1; L < a.nlvl; L++) {
        for (int q = a.lvl_off[L] + tid; q < a.lvl_off[L + 1]; q += kDfNT) {
            const int r = a.order[q];
            v[r] = fmax(v[r], v[a.prec[r]]);
        }
        __syncthreads();
    }
    double mn = __builtin_inf();
    for (int q = tid; q < a.nleaf; q += kDfNT) mn = fmin(mn, v[a.leaf[q]]);
    red[tid] = mn;
    __syncthreads();
    for (int s = kDfNT / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = fmin(red[tid], red[tid + s]);
        __syncthreads();
    }
    if (tid == 0) a.out[k] = a.bare ? -__builtin_inf() : red[0];
}

}  // namespace mipx
