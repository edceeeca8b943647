// complete_kernels.hip.h -- the two kernels of include/mipx_complete.h around the node-LP launch: the points of the
// heuristics completed over the continuous columns by one batched LP.
//
//   complete_prepare   one workgroup of 256 threads per point: PREPARE.  The point's rows of the launch's bounds
//                      (L, U), its row of basis codes (the caller's, or all 0: a cold start), its skip flag, and the
//                      point itself copied to x_out (what every point that does not end COMPLETED returns).  A
//                      skipped point gets L = U = l: an LP that ends without a pivot.  The integrality test is one
//                      pass over the integer columns and one __syncthreads_or.
//   complete_finish    one workgroup of 256 threads per point: FINISH and STATUS.  x^ in LDS; thread t takes the
//                      rows t, t + 256, ... of A (row-major, as the heuristic's kernel reads them) and the columns
//                      t, t + 256, ... of the bound test; one __syncthreads_or decides; thread 0 sums the objective.
//
// Between the two the node-LP kernels run unchanged (K1 / K1b through launch_lp_any, on the same stream).  Plain
// vector stores only, no atomics, no scratch.  Every sum is taken in the order mipx_complete.h states (columns
// ascending, one add per term; the library is built with -ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace mipx {

constexpr int kCompNT = 256;     // threads per workgroup
constexpr int kCompMax = 1024;   // rows and columns at most (what the LP kernels take)

// The launch's workspace for `batch` points of n columns and m rows: [L | U | the LP's x] (f64, batch x n each),
// [the LP's status | its pivots | the skip flags] (i32, batch each), [basis codes] (i8, batch x (n + m)); every
// block 256-byte aligned.
struct CompWs {
    size_t L, U, x, lp_status, pivots, skipped, vstat, end;
    static size_t up(size_t v) { return (v + 255) / 256 * 256; }
    CompWs(size_t batch, size_t m, size_t n)
        : L(0), U(up(L + 8 * batch * n)), x(up(U + 8 * batch * n)), lp_status(up(x + 8 * batch * n)),
          pivots(up(lp_status + 4 * batch)), skipped(up(pivots + 4 * batch)), vstat(up(skipped + 4 * batch)),
          end(up(vstat + batch * (n + m))) {}
    size_t bytes() const { return end; }
};

struct CompArgs {
    int m, n, n_int;
    int p0;                         // position of this launch's first point in the workspace and the outputs
    double ctol;
    const double *A, *b, *c;        // the problem's rows A x >= b (m x n, row-major) and objective
    const double *l, *u;            // the root's bounds, n each
    const int32_t *int_idx;         // the integer columns, n_int of them
    const double *x;                // the launch's points (prepare): row 0 is point p0
    const uint8_t *skip;            // nullable, indexed like x: a point whose entry is not 0 is skipped
    const int32_t *gate;            // nullable, indexed like x: a heuristic's status per point; a point whose entry is 3
    int gate_strict;                // (SKIPPED) is skipped, and with gate_strict every point whose entry is not 0
    const int8_t *vstat;            // nullable, indexed like x: n + m basis codes per point
    double *ws_L, *ws_U;            // the workspace, indexed by position
    const double *ws_x;
    int32_t *ws_skipped;
    const int32_t *ws_lp_status, *ws_pivots;
    int8_t *ws_vstat;
    double *x_out, *obj_out;        // indexed by position: batch x n, batch
    int32_t *status_out, *pivots_out;
};

__global__ void __launch_bounds__(kCompNT) complete_prepare(CompArgs a) {
    const int q = blockIdx.x, tid = threadIdx.x, n = a.n, nv = a.n + a.m;
    const size_t g = (size_t)a.p0 + (size_t)q;
    const double *x = a.x + (size_t)q * n;
    double *L = a.ws_L + g * n, *U = a.ws_U + g * n, *xo = a.x_out + g * n;
    int bad = ((a.skip && a.skip[q]) || (a.gate && (a.gate_strict ? a.gate[q] != 0 : a.gate[q] == 3))) ? 1 : 0;   // (uniform over the workgroup)
    for (int k = tid; k < a.n_int; k += kCompNT) {
        const int j = a.int_idx[k];
        const double v = x[j];
        if (!(v == floor(v)) || v < ceil(a.l[j] - a.ctol) || v > floor(a.u[j] + a.ctol)) bad = 1;
    }
    bad = __syncthreads_or(bad);
    for (int j = tid; j < n; j += kCompNT) {
        const double lj = a.l[j];
        L[j] = lj;
        U[j] = bad ? lj : a.u[j];
        xo[j] = x[j];
    }
    __syncthreads();   // (the integer columns over the rows just written: the same threads need not own them)
    if (!bad)
        for (int k = tid; k < a.n_int; k += kCompNT) {
            const int j = a.int_idx[k];
            const double v = x[j];
            L[j] = v;
            U[j] = v;
        }
    int8_t *vo = a.ws_vstat + g * (size_t)nv;
    const int8_t *vi = (a.vstat && !bad) ? a.vstat + (size_t)q * nv : nullptr;
    for (int v = tid; v < nv; v += kCompNT) vo[v] = vi ? vi[v] : (int8_t)0;
    if (tid == 0) a.ws_skipped[g] = bad;
}

// FINISH of include/mipx_complete.h for one point, by the kCompNT threads of a workgroup (xt, isint: kCompMax entries
// of LDS each): x^ is xl with the integer columns taken from `fixed`; l, u are the bounds the other columns are held
// to.  Returns whether the point fails (uniform); a point that holds is written to xo (which may be xl) and thread 0
// returns its objective in *obj (0 for one that fails).  Shared with lpdive_finish (lpdive_kernels.hip.h).
__device__ __forceinline__ int complete_finish_point(int m, int n, int n_int, double ctol, const double *A, const double *b,
                                                     const double *c, const double *l, const double *u, const int32_t *int_idx,
                                                     const double *xl, const double *fixed, double *xo, double *obj,
                                                     double *xt, uint8_t *isint) {
    const int tid = threadIdx.x;
    for (int j = tid; j < n; j += kCompNT) { xt[j] = xl[j]; isint[j] = 0; }
    __syncthreads();
    for (int k = tid; k < n_int; k += kCompNT) {
        const int j = int_idx[k];
        xt[j] = fixed[j];   // (x~_j, to the bit)
        isint[j] = 1;
    }
    __syncthreads();
    int bad = 0;
    for (int i = tid; i < m; i += kCompNT) {
        const double *row = A + (size_t)i * n;
        double acc = 0.0;
        for (int j = 0; j < n; j++) acc += row[j] * xt[j];
        if (!(acc - b[i] >= -ctol)) bad = 1;
    }
    for (int j = tid; j < n; j += kCompNT)
        if (!isint[j] && !(xt[j] >= l[j] - ctol && xt[j] <= u[j] + ctol)) bad = 1;
    bad = __syncthreads_or(bad);
    if (!bad)
        for (int j = tid; j < n; j += kCompNT) xo[j] = xt[j];
    if (tid == 0) {
        double v = 0.0;
        if (!bad)
            for (int j = 0; j < n; j++) v += c[j] * xt[j];
        *obj = v;
    }
    return bad;
}

__global__ void __launch_bounds__(kCompNT) complete_finish(CompArgs a) {
    __shared__ double xt[kCompMax];
    __shared__ uint8_t isint[kCompMax];
    const int tid = threadIdx.x, n = a.n;
    const size_t g = (size_t)a.p0 + (size_t)blockIdx.x;
    const int lp = a.ws_lp_status[g];
    int status = a.ws_skipped[g] ? 3 : lp == 0 ? 0 : lp == 1 ? 1 : 2;   // (uniform over the workgroup)
    if (status != 0) {
        if (tid == 0) {
            a.obj_out[g] = 0.0;
            a.status_out[g] = status;
            a.pivots_out[g] = status == 3 ? 0 : a.ws_pivots[g];
        }
        return;   // (x_out holds x~ since complete_prepare)
    }
    double obj = 0.0;
    const int bad = complete_finish_point(a.m, n, a.n_int, a.ctol, a.A, a.b, a.c, a.l, a.u, a.int_idx, a.ws_x + g * n,
                                          a.ws_L + g * n, a.x_out + g * n, &obj, xt, isint);
    if (tid == 0) {
        a.obj_out[g] = obj;
        a.status_out[g] = bad ? 4 : 0;
        a.pivots_out[g] = a.ws_pivots[g];
    }
}

}  // namespace mipx
