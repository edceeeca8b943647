// cglp_screen_kernels.hip.h -- the dual screen of a support evaluation (include/mipx_cglp_screen.h): which leaves
// need no LP for this direction, and the leaf LPs over the packed rest.
//   support_screen      per leaf with duals on record: the weak-duality bound L_t(pi; y+) and whether it screens
//   support_pack_count  per segment of 2048 leaves: how many go into the launch (and the smallest screened margin)
//   support_pack        the positions of those leaves in ascending order, and their count
//   support_gather      bounds and basis codes of the packed leaves into the launch buffers
//   support_scatter     what the launch wrote, back to the leaves' positions
//   support_mark        after a launch over every leaf: whose duals are on record
// The bound's arithmetic is fixed (the header states it; tests/support/cglp_screen_reference.py restates it in NumPy):
// one wave per leaf, lane q takes the columns q, q + 64, ...; a column's (A' y+)_j is an fma chain over the rows in
// ascending order, rows with y+ = 0 left out; the lane adds its columns' terms in ascending order; the 64 partial sums
// meet in a butterfly of xor-shuffles (offsets 32, 16, ..., 1: a + b is b + a, every lane ends on the same bits); y+.b
// the same way over the rows, product then sum; L = columns + rows.  The packed order comes from a block scan and the
// segments' counts: no atomic, no order among workgroups.  Plain vector loads and stores.  Included by
// tree_engine.hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mipx {

constexpr int kScrNT = 256;                  // threads of every kernel here
constexpr int kScrWaves = kScrNT / 64;       // leaves per workgroup of support_screen
constexpr int kScrMax = 1024;                // rows and columns at most (y+ of a leaf waits in LDS)
constexpr int kScrItems = 8;                 // consecutive leaves per thread of the pack kernels
constexpr int kScrSeg = kScrNT * kScrItems;  // leaves per workgroup of the pack kernels

__device__ __forceinline__ double scr_wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
    return v;
}

struct SupScreenArgs {
    int T = 0, m = 0, n = 0;
    double pi0 = 0.0, screen_tol = 0.0;
    const double *A = nullptr, *b = nullptr, *pi = nullptr;   // shared: m x n row-major, m, n
    const double *l = nullptr, *u = nullptr, *y = nullptr;    // per leaf: T x n, T x n, T x m
    const uint8_t *has_y = nullptr;                           // T: duals on record
    double *bound = nullptr;                                  // T: L_t (-inf without duals)
    uint8_t *screened = nullptr;                              // T
    // a session's record of a screened leaf, as the selection reads it (null on a caller's data): the bound in the
    // place of h_t, verdict optimal, no iterations in this evaluation
    double *obj = nullptr;
    int32_t *status = nullptr, *iters = nullptr, *npivots = nullptr;
};

__global__ void __launch_bounds__(kScrNT) support_screen(SupScreenArgs a) {
    __shared__ double yp[kScrWaves][kScrMax];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int t = blockIdx.x * kScrWaves + w;
    const int m = a.m, n = a.n;
    const bool have = t < a.T && a.has_y[t] != 0;
    double *ys = yp[w];
    if (have)
        for (int i = lane; i < m; i += 64) {
            const double v = a.y[(size_t)t * m + i];
            ys[i] = v > 0.0 ? v : 0.0;   // (NaN reads as 0)
        }
    __syncthreads();
    if (t >= a.T) return;
    double L = -__builtin_inf();
    if (have) {
        const double *lo = a.l + (size_t)t * n, *up = a.u + (size_t)t * n;
        double cols = 0.0;
        for (int j = lane; j < n; j += 64) {
            double s = 0.0;
            for (int i = 0; i < m; i++) {
                const double yi = ys[i];   // (the same word in every lane: the branch is the wave's)
                if (yi > 0.0) s = fma(a.A[(size_t)i * n + j], yi, s);
            }
            const double r = a.pi[j] - s;
            const double p1 = r * lo[j], p2 = r * up[j];
            cols = cols + (p2 < p1 ? p2 : p1);
        }
        cols = scr_wave_sum(cols);
        double rows = 0.0;
        for (int i = lane; i < m; i += 64) rows = rows + ys[i] * a.b[i];
        rows = scr_wave_sum(rows);
        L = cols + rows;
    }
    if (lane == 0) {
        const bool scr = have && __builtin_isfinite(L) && (L - a.pi0 >= -a.screen_tol);
        a.bound[t] = L;
        a.screened[t] = scr ? 1 : 0;
        if (scr && a.obj) { a.obj[t] = L; a.status[t] = 0; a.iters[t] = 0; a.npivots[t] = 0; }
    }
}

struct SupPackInfo {
    int32_t count;       // leaves packed
    int32_t pad;
    double min_margin;   // the smallest bound - pi0 over the leaves marked in `skip` (+inf without any)
};

struct SupPackArgs {
    int T = 0, G = 0;                    // leaves, segments
    const uint8_t *skip = nullptr;       // T: 1 = not packed (the screened leaves) ...
    const int32_t *status = nullptr;     // ... or, if given: a leaf is packed iff its verdict is not `optimal`
    const double *bound = nullptr;       // T, with skip: for min_margin (may be null)
    double pi0 = 0.0;
    int32_t *seg_count = nullptr;        // G
    double *seg_min = nullptr;           // G
    int32_t *packed = nullptr;           // T: the first `count` entries are written
    SupPackInfo *info = nullptr;
};

__device__ __forceinline__ bool scr_takes(const SupPackArgs &a, int t) {
    return a.status ? a.status[t] != 0 : a.skip[t] == 0;
}

__global__ void __launch_bounds__(kScrNT) support_pack_count(SupPackArgs a) {
    __shared__ int cnt[kScrWaves];
    __shared__ double mn[kScrWaves];
    const int tid = threadIdx.x, g = blockIdx.x;
    const int base = g * kScrSeg + tid * kScrItems;
    int c = 0;
    double lo = __builtin_inf();
    for (int i = 0; i < kScrItems; i++) {
        const int t = base + i;
        if (t >= a.T) break;
        if (scr_takes(a, t)) c++;
        else if (!a.status && a.bound) {
            const double mg = a.bound[t] - a.pi0;
            lo = mg < lo ? mg : lo;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        c += __shfl_xor(c, off, 64);
        const double o = __shfl_xor(lo, off, 64);
        lo = o < lo ? o : lo;
    }
    if ((tid & 63) == 0) { cnt[tid >> 6] = c; mn[tid >> 6] = lo; }
    __syncthreads();
    if (tid == 0) {
        int s = 0;
        double q = __builtin_inf();
        for (int w = 0; w < kScrWaves; w++) { s += cnt[w]; q = mn[w] < q ? mn[w] : q; }
        a.seg_count[g] = s;
        a.seg_min[g] = q;
    }
}

__global__ void __launch_bounds__(kScrNT) support_pack(SupPackArgs a) {
    __shared__ int red[kScrWaves];
    __shared__ int wsum[kScrWaves];
    __shared__ double mn[kScrWaves];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = blockIdx.x;
    // the leaves packed by the segments before this one
    int before = 0;
    for (int h = tid; h < g; h += kScrNT) before += a.seg_count[h];
    for (int off = 32; off > 0; off >>= 1) before += __shfl_xor(before, off, 64);
    if (lane == 0) red[w] = before;
    // this segment: a thread's leaves are consecutive, so ranks in thread order are ranks in leaf order
    const int base = g * kScrSeg + tid * kScrItems;
    bool take[kScrItems];
    int c = 0;
#pragma unroll
    for (int i = 0; i < kScrItems; i++) {
        const int t = base + i;
        take[i] = t < a.T && scr_takes(a, t);
        c += take[i] ? 1 : 0;
    }
    int incl = c;   // inclusive scan over the wave
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
    }
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    int start = 0, own = 0;
    for (int v = 0; v < kScrWaves; v++) {
        start += red[v];
        if (v < w) start += wsum[v];
        own += wsum[v];
    }
    int at = start + incl - c;
#pragma unroll
    for (int i = 0; i < kScrItems; i++)
        if (take[i]) a.packed[at++] = base + i;
    if (g != a.G - 1) return;   // (the block's: the last segment also writes the totals)
    double lo = __builtin_inf();
    for (int h = tid; h < a.G; h += kScrNT) lo = a.seg_min[h] < lo ? a.seg_min[h] : lo;
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(lo, off, 64);
        lo = o < lo ? o : lo;
    }
    if (lane == 0) mn[w] = lo;
    __syncthreads();
    if (tid == 0) {
        int before_all = 0;
        for (int v = 0; v < kScrWaves; v++) { before_all += red[v]; lo = mn[v] < lo ? mn[v] : lo; }
        a.info->count = before_all + own;
        a.info->pad = 0;
        a.info->min_margin = lo;
    }
}

struct SupMoveArgs {
    int count = 0, T = 0, n = 0, m = 0;   // packed leaves, leaves of the session, columns, rows
    const int32_t *packed = nullptr;      // count positions
    // per leaf (position t) ...
    double *l = nullptr, *u = nullptr, *x = nullptr, *obj = nullptr, *y = nullptr;
    int8_t *v = nullptr;                  // basis codes, n + m per leaf (gather: may be null, a cold launch needs none)
    int32_t *status = nullptr, *iters = nullptr, *npivots = nullptr;
    uint8_t *has_y = nullptr;
    // ... and per packed leaf (position k of the launch)
    double *pl = nullptr, *pu = nullptr, *px = nullptr, *pobj = nullptr, *py = nullptr;
    int8_t *pv_in = nullptr, *pv_out = nullptr;
    int32_t *pstatus = nullptr, *piters = nullptr, *pnpivots = nullptr;
    int add = 0;                          // scatter: iterations and pivots are added to the leaf's (a second LP of this evaluation)
};

__global__ void __launch_bounds__(kScrNT) support_gather(SupMoveArgs a) {
    const int k = blockIdx.x, tid = threadIdx.x;
    if (k >= a.count) return;
    const int t = a.packed[k];
    if (t < 0 || t >= a.T) return;   // (cannot happen: a packed entry is a leaf's position)
    const size_t n = (size_t)a.n, nv = n + (size_t)a.m;
    for (size_t j = tid; j < n; j += kScrNT) {
        a.pl[(size_t)k * n + j] = a.l[(size_t)t * n + j];
        a.pu[(size_t)k * n + j] = a.u[(size_t)t * n + j];
    }
    if (a.v)
        for (size_t q = tid; q < nv; q += kScrNT) a.pv_in[(size_t)k * nv + q] = a.v[(size_t)t * nv + q];
}

__global__ void __launch_bounds__(kScrNT) support_scatter(SupMoveArgs a) {
    const int k = blockIdx.x, tid = threadIdx.x;
    if (k >= a.count) return;
    const int t = a.packed[k];
    if (t < 0 || t >= a.T) return;
    const size_t n = (size_t)a.n, m = (size_t)a.m, nv = n + m;
    const int st = a.pstatus[k];
    for (size_t j = tid; j < n; j += kScrNT) a.x[(size_t)t * n + j] = a.px[(size_t)k * n + j];
    for (size_t q = tid; q < nv; q += kScrNT) a.v[(size_t)t * nv + q] = a.pv_out[(size_t)k * nv + q];
    if (st == 0)   // the duals of an LP that did not end optimal are not kept: the leaf's last optimal ones stay
        for (size_t i = tid; i < m; i += kScrNT) a.y[(size_t)t * m + i] = a.py[(size_t)k * m + i];
    if (tid == 0) {
        a.status[t] = st;
        a.obj[t] = a.pobj[k];
        a.iters[t] = (a.add ? a.iters[t] : 0) + a.piters[k];
        a.npivots[t] = (a.add ? a.npivots[t] : 0) + a.pnpivots[k];
        if (st == 0) a.has_y[t] = 1;
    }
}

__global__ void __launch_bounds__(kScrNT) support_mark(int T, const int32_t *status, uint8_t *has_y) {
    const int t = blockIdx.x * kScrNT + threadIdx.x;
    if (t < T) has_y[t] = status[t] == 0 ? 1 : 0;
}

}  // namespace mipx
