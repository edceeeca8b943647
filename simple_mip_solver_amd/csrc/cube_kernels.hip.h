// cube_kernels.hip.h -- the cube search of include/mipx_cube.h: choose the k most fractional integer columns of an
// LP point, hold every other column where the rounding puts it, and try all 2^k ways to round the k up or down.
//
//   cube_prepare     one workgroup of 256 threads per point: SELECT and BASE.  The candidates' fractionalities live
//                    in LDS by position in int_idx (21 KiB with the point itself, whatever the size); a candidate's rank
//                    is the count of candidates that go before it (larger f, then lower column), its place in F the
//                    count of chosen columns below it -- counting, no sort, n_int <= 1024.  It writes x~ to x_out
//                    and s, obj0, k and F to the point's block of the workspace (CubeWs).
//   cube_enumerate   a grid of chunks x points, 256 threads; the points lie in the grid's y, 65535 to a launch, and a
//                    larger batch takes several launches (p0).  A thread owns a run of R consecutive codes, a
//                    workgroup a chunk of 256 R: R = 1 up to k = 8, 2^(k - 8) up to k = 12, 16 above, so a point
//                    has one chunk up to k = 12 and 2^(k - 12) above (256 at k = 20); workgroups past a point's
//                    last chunk exit at once.  LDS: s (8 KiB), c_F and F, and the k chosen columns of A as an
//                    m x k block while m k <= 4096 doubles (32 KiB; 41 KiB in all, three workgroups to a CU's
//                    160 KiB).  FALLBACK: with m k > 4096 (1024 rows from k = 5 on) the entries a_{i,F_t} are read
//                    from A itself, which the launch before has left in L2; s, c_F and F stay in LDS.  Either way
//                    the threads of a wave read the same (i, t) at a time: a broadcast.  A code's objective is
//                    formed first; a code that is not improving, or not below the thread's best so far (codes
//                    ascend within a run, so it could not win), reads no row; the row loop takes four rows at a
//                    time, a term of a bit that is not set being +0 (no branch in the loop), and leaves at the
//                    first four with a violated row.  The workgroup takes the min of its threads' keys (obj, code) -- a total
//                    order, so the shape of the reduction does not matter -- and writes one partial per
//                    (point, chunk).
//   cube_pick        one workgroup per point: the min over the chunks' partials, then x_out, obj, status, counts.
//
// No atomics, no scratch, plain vector stores; nothing depends on which workgroup finishes first.  Every sum is
// taken in the order mipx_cube.h states (one add per term from s_i or obj0, t ascending; the library is built with
// -ffp-contract=off), so that a restatement in the same order gives the same bits.  A sum that starts from +0 is
// never -0, so leaving a term out and adding +0 are the same.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace mipx {

constexpr int kCubeNT = 256;        // threads per workgroup
constexpr int kCubeMax = 1024;      // rows and columns at most (what the LP kernels take)
constexpr int kCubeMaxK = 20;       // columns enumerated at most
constexpr int kCubeRunLog = 4;      // a thread's run is 2^4 codes at most
constexpr int kCubeChunkLog = 8 + kCubeRunLog;            // a chunk is 2^12 codes at most
constexpr int kCubeLdsCols = 4096;  // doubles of LDS for the chosen columns of A (the fallback rule above)
constexpr int kCubeKF = 24;         // int32 per point in the workspace: k (-1: skipped), then F_0 .. F_{k-1}
constexpr int kCubeNoCode = 0x7fffffff;
constexpr int kCubeGridY = 65535;   // points per launch of cube_enumerate (a grid's y extent); a larger batch is split

// chunks of a point with k columns, and the grid's width for a cap of K
__host__ __device__ inline int cube_chunks(int k) { return k <= kCubeChunkLog ? 1 : 1 << (k - kCubeChunkLog); }
// log2 of the codes a thread owns
__host__ __device__ inline int cube_run_log(int k) { return k <= 8 ? 0 : (k >= kCubeChunkLog ? kCubeRunLog : k - 8); }

// The workspace of one launch over `batch` points with the cap K, one block: [s: batch x m] [obj0: batch]
// [pobj: batch x chunks(K)] (f64) [kf: batch x kCubeKF] [pcode: batch x chunks(K)] (i32).
struct CubeWs {
    size_t s, obj0, pobj, kf, pcode, end;
    CubeWs(size_t batch, size_t m, int K)
        : s(0), obj0(8 * batch * m), pobj(obj0 + 8 * batch), kf(pobj + 8 * batch * (size_t)cube_chunks(K)),
          pcode(kf + 4 * batch * kCubeKF), end(pcode + 4 * batch * (size_t)cube_chunks(K)) {}
    size_t bytes() const { return end; }
};

struct CubeArgs {
    int m, n, n_int, K, nchunks;    // nchunks: cube_chunks(K), the stride of the partials
    int p0;                         // cube_enumerate: the point of blockIdx.y == 0 (a launch takes kCubeGridY points)
    double tol, ftol, cutoff;
    const double *A, *b, *c;        // the problem's rows A x >= b (m x n, row-major) and objective
    const double *l, *u;            // the root's bounds, n each
    const int32_t *int_idx;         // the integer columns, n_int of them
    const double *x;                // batch x n: the points
    const uint8_t *skip;            // nullable: a point whose entry is not 0 is skipped
    const int32_t *lp_status;       // nullable: a point whose entry is not 0 is skipped
    double *ws_s, *ws_obj0, *ws_pobj;   // the workspace (CubeWs)
    int32_t *ws_kf, *ws_pcode;
    double *x_out, *obj_out;        // batch x n (not x itself), batch
    int32_t *status_out, *counts_out;   // batch, 2 x batch (k, code)
};

__global__ void __launch_bounds__(kCubeNT) cube_prepare(CubeArgs a) {
    __shared__ double xt[kCubeMax], sf[kCubeMax];   // (sf: by position in int_idx; -1: no candidate)
    __shared__ int32_t scol[kCubeMax];
    __shared__ uint8_t ssel[kCubeMax];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int m = a.m, n = a.n, n_int = a.n_int;
    const double tol = a.tol;
    const double *x = a.x + (size_t)p * n;
    int32_t *kf = a.ws_kf + (size_t)p * kCubeKF;
    if ((a.skip && a.skip[p]) || (a.lp_status && a.lp_status[p] != 0)) {   // (uniform over the workgroup)
        if (tid == 0) kf[0] = -1;
        return;
    }
    for (int j = tid; j < n; j += kCubeNT) xt[j] = x[j];
    __syncthreads();
    // SELECT: the candidates and their fractionalities; every integer column takes its ROUND for now
    for (int q = tid; q < n_int; q += kCubeNT) {
        const int j = a.int_idx[q];
        const double lo = ceil(a.l[j] - tol), hi = floor(a.u[j] + tol);
        const double xv = x[j], fl = floor(xv), nr = floor(xv + 0.5);
        const double f = fabs(xv - nr);
        sf[q] = (f > a.ftol && lo <= fl && fl + 1.0 <= hi) ? f : -1.0;
        scol[q] = j;
        xt[j] = fmin(fmax(nr, lo), hi) + 0.0;   // (+ 0.0: a zero result is +0 whatever max / min pick)
    }
    __syncthreads();
    for (int q = tid; q < n_int; q += kCubeNT) {
        const double f = sf[q];
        int rank = 0;
        if (f >= 0.0) {
            const int j = scol[q];
            for (int r = 0; r < n_int; r++) {
                const double g = sf[r];
                rank += (g > f || (g == f && scol[r] < j)) ? 1 : 0;
            }
        }
        ssel[q] = (f >= 0.0 && rank < a.K) ? 1 : 0;
    }
    __syncthreads();
    // BASE: a chosen column goes to its floor and takes its place in F (ascending column order)
    for (int q = tid; q < n_int; q += kCubeNT) {
        if (!ssel[q]) continue;
        const int j = scol[q];
        int pos = 0;
        for (int r = 0; r < n_int; r++) pos += (ssel[r] && scol[r] < j) ? 1 : 0;
        kf[1 + pos] = j;
        xt[j] = floor(x[j]) + 0.0;
    }
    if (tid == 0) {
        int k = 0;
        for (int r = 0; r < n_int; r++) k += ssel[r];
        kf[0] = k;
    }
    __syncthreads();
    double *xo = a.x_out + (size_t)p * n;
    for (int j = tid; j < n; j += kCubeNT) xo[j] = xt[j];
    // s_i = a_i . x~ - b_i, columns ascending
    for (int i = tid; i < m; i += kCubeNT) {
        const double *row = a.A + (size_t)i * n;
        double acc = 0.0;
        for (int j = 0; j < n; j++) acc += row[j] * xt[j];
        a.ws_s[(size_t)p * m + i] = acc - a.b[i];
    }
    if (tid == 0) {
        double obj = 0.0;
        for (int j = 0; j < n; j++) obj += a.c[j] * xt[j];
        a.ws_obj0[p] = obj;
    }
}

// (obj, code): compared in that order; kCubeNoCode means "no code"
struct CubeKey { double obj; int code; };

__device__ inline bool cube_less(const CubeKey &a, const CubeKey &b) {
    if (a.code == kCubeNoCode) return false;
    if (b.code == kCubeNoCode) return true;
    if (a.obj != b.obj) return a.obj < b.obj;
    return a.code < b.code;
}

// the smallest key of the workgroup, in every thread (slots: one per wave)
__device__ inline CubeKey cube_block_min(CubeKey k, CubeKey *slots) {
    for (int off = 32; off > 0; off >>= 1) {
        CubeKey o;
        o.obj = __shfl_xor(k.obj, off, 64);
        o.code = __shfl_xor(k.code, off, 64);
        if (cube_less(o, k)) k = o;
    }
    if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = k;
    __syncthreads();
    CubeKey r = slots[0];
    for (int w = 1; w < kCubeNT / 64; w++)
        if (cube_less(slots[w], r)) r = slots[w];
    return r;
}

// Whether code e keeps every row: s_i plus a_{i,F_t} over the set bits of e, t ascending, four rows at a time (four
// independent chains of adds; a term of a bit that is not set is +0, which changes no bit of a sum that cannot be -0),
// left at the first group with a violated row.  entry(i, t) is a_{i,F_t}.
template <class Entry>
__device__ inline bool cube_rows_hold(int e, int k, int m, double tol, const double *ss, Entry entry) {
    int i = 0;
    for (; i + 4 <= m; i += 4) {
        double a0 = ss[i], a1 = ss[i + 1], a2 = ss[i + 2], a3 = ss[i + 3];
        for (int t = 0; t < k; t++) {
            const double v0 = entry(i, t), v1 = entry(i + 1, t), v2 = entry(i + 2, t), v3 = entry(i + 3, t);
            const bool on = (e >> t) & 1;
            a0 += on ? v0 : 0.0;
            a1 += on ? v1 : 0.0;
            a2 += on ? v2 : 0.0;
            a3 += on ? v3 : 0.0;
        }
        if (!(a0 >= -tol && a1 >= -tol && a2 >= -tol && a3 >= -tol)) return false;
    }
    for (; i < m; i++) {
        double acc = ss[i];
        for (int t = 0; t < k; t++) {
            const double v = entry(i, t);
            acc += ((e >> t) & 1) ? v : 0.0;
        }
        if (!(acc >= -tol)) return false;
    }
    return true;
}

__global__ void __launch_bounds__(kCubeNT) cube_enumerate(CubeArgs a) {
    __shared__ double cols[kCubeLdsCols], ss[kCubeMax], sc[kCubeMaxK];
    __shared__ int32_t sF[kCubeMaxK];
    __shared__ CubeKey slots[kCubeNT / 64];
    const int p = a.p0 + (int)blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    const int m = a.m, n = a.n;
    const int32_t *kf = a.ws_kf + (size_t)p * kCubeKF;
    const int k = kf[0];
    if (k < 0 || chunk >= cube_chunks(k)) return;   // (uniform over the workgroup: a skipped point, or past its 2^k)
    const bool in_lds = m * k <= kCubeLdsCols;
    if (tid < k) {
        sF[tid] = kf[1 + tid];
        sc[tid] = a.c[kf[1 + tid]];
    }
    for (int i = tid; i < m; i += kCubeNT) ss[i] = a.ws_s[(size_t)p * m + i];
    if (in_lds)
        for (int e = tid; e < m * k; e += kCubeNT) cols[e] = a.A[(size_t)(e / k) * n + kf[1 + e % k]];
    __syncthreads();
    const double tol = a.tol, U = a.cutoff, obj0 = a.ws_obj0[p];
    const int ncodes = 1 << k, rl = cube_run_log(k);
    const int first = (chunk << (8 + rl)) + (tid << rl);
    CubeKey best;
    best.obj = 0.0; best.code = kCubeNoCode;
    for (int r = 0; r < (1 << rl); r++) {
        const int e = first + r;
        if (e >= ncodes) break;
        double obj = obj0;
        for (int t = 0; t < k; t++) {
            const double ct = sc[t];
            obj += ((e >> t) & 1) ? ct : 0.0;
        }
        if (!(obj < U)) continue;                                   // not improving
        if (best.code != kCubeNoCode && !(obj < best.obj)) continue;   // cannot beat this thread's earlier code
        const bool ok = in_lds ? cube_rows_hold(e, k, m, tol, ss, [&](int i, int t) { return cols[i * k + t]; })
                               : cube_rows_hold(e, k, m, tol, ss, [&](int i, int t) { return a.A[(size_t)i * n + sF[t]]; });
        if (ok) { best.obj = obj; best.code = e; }
    }
    best = cube_block_min(best, slots);
    if (tid == 0) {
        a.ws_pobj[(size_t)p * a.nchunks + chunk] = best.obj;
        a.ws_pcode[(size_t)p * a.nchunks + chunk] = best.code;
    }
}

__global__ void __launch_bounds__(kCubeNT) cube_pick(CubeArgs a) {
    __shared__ CubeKey slots[kCubeNT / 64];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int n = a.n;
    const int32_t *kf = a.ws_kf + (size_t)p * kCubeKF;
    const int k = kf[0];
    const double *x = a.x + (size_t)p * n;
    double *xo = a.x_out + (size_t)p * n;
    if (k < 0) {   // SKIPPED
        for (int j = tid; j < n; j += kCubeNT) xo[j] = x[j];
        if (tid == 0) {
            a.obj_out[p] = 0.0;
            a.status_out[p] = 3;
            a.counts_out[2 * p] = 0;
            a.counts_out[2 * p + 1] = -1;
        }
        return;
    }
    CubeKey best;
    best.obj = 0.0; best.code = kCubeNoCode;
    const int chunks = cube_chunks(k);
    for (int q = tid; q < chunks; q += kCubeNT) {
        CubeKey o;
        o.obj = a.ws_pobj[(size_t)p * a.nchunks + q];
        o.code = a.ws_pcode[(size_t)p * a.nchunks + q];
        if (cube_less(o, best)) best = o;
    }
    best = cube_block_min(best, slots);
    if (best.code == kCubeNoCode) {   // NONE
        for (int j = tid; j < n; j += kCubeNT) xo[j] = x[j];
    } else if (tid < k && ((best.code >> tid) & 1)) {   // FOUND: x_out holds x~
        xo[kf[1 + tid]] = xo[kf[1 + tid]] + 1.0;
    }
    if (tid == 0) {
        const bool found = best.code != kCubeNoCode;
        a.obj_out[p] = found ? best.obj : 0.0;
        a.status_out[p] = found ? 0 : 1;
        a.counts_out[2 * p] = k;
        a.counts_out[2 * p + 1] = found ? best.code : -1;
    }
}

}  // namespace mipx
