// cglp_kernels.hip.h -- the selection behind a support evaluation (include/mipx_cglp.h).
//   support_select        per segment of 2048 leaves: the margins h_t - pi0, the count below -tol, the sums of
//                         iterations and pivots, and the segment's P leaves of smallest (margin, node id)
//   support_select_merge  one workgroup: the P smallest over the segments' candidates, the totals, and the rows
//                         [node id, h_t, x_t] of the selected leaves gathered into the output block
// A leaf's key is the pair (margin, node id): node ids are distinct, so the keys are strictly ordered and the
// p-th smallest is "the smallest key above the (p-1)-th".  The selection needs no flag, no atomic and no order
// among workgroups: the block is the same bits however the launch is scheduled.  Reductions are wave-wide
// shuffles, then one LDS slot per wave.  Included by tree_engine.hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mipx {

constexpr int kSupNT = 256;                 // threads of both kernels
constexpr int kSupItems = 8;                // leaves per thread of support_select
constexpr int kSupSeg = kSupNT * kSupItems; // leaves per workgroup
constexpr int kSupMaxP = 1024;
constexpr int kSupHead = 8;                 // doubles in front of the rows of the output block
constexpr int kSupNone = 0x7fffffff;        // the node id of "no leaf"

struct SupKey {
    double m;    // margin
    int id;      // node id (kSupNone: none)
    int t;       // position in the session
};

__device__ __forceinline__ bool sup_less(double am, int aid, double bm, int bid) {
    return am < bm || (am == bm && aid < bid);
}

__device__ __forceinline__ SupKey sup_wave_min(SupKey k) {
    for (int off = 32; off > 0; off >>= 1) {
        const double om = __shfl_xor(k.m, off, 64);
        const int oid = __shfl_xor(k.id, off, 64);
        const int ot = __shfl_xor(k.t, off, 64);
        if (sup_less(om, oid, k.m, k.id)) { k.m = om; k.id = oid; k.t = ot; }
    }
    return k;
}

// the smallest key of the workgroup, in every thread (red: one slot per wave; two barriers)
__device__ __forceinline__ SupKey sup_block_min(SupKey k, SupKey *red) {
    const int tid = threadIdx.x;
    k = sup_wave_min(k);
    if ((tid & 63) == 0) red[tid >> 6] = k;
    __syncthreads();
    SupKey b = red[0];
    for (int w = 1; w < kSupNT / 64; w++)
        if (sup_less(red[w].m, red[w].id, b.m, b.id)) b = red[w];
    __syncthreads();
    return b;
}

__device__ __forceinline__ double sup_wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

struct SupSelectArgs {
    int T = 0, n = 0, P = 0, G = 0;     // leaves, columns, rows asked for, segments (workgroups of stage one)
    double pi0 = 0.0, tol = 0.0;
    const int64_t *ids = nullptr;        // T node ids
    const int32_t *status = nullptr;     // T verdicts of the launch
    const double *obj = nullptr;         // T: h_t
    const double *x = nullptr;           // T x n
    const int32_t *iters = nullptr, *npivots = nullptr;   // T
    double *margin = nullptr;            // T: h_t - pi0 (+inf where the LP did not end optimal)
    // per segment: P candidates in ascending order, and [below, not optimal, iterations, pivots]
    double *cand_m = nullptr;
    int32_t *cand_id = nullptr, *cand_t = nullptr;
    double *seg_sum = nullptr;           // G x 4
    double *block = nullptr;             // kSupHead + P (n + 2)
};

__global__ void __launch_bounds__(kSupNT) support_select(SupSelectArgs a) {
    __shared__ SupKey red[kSupNT / 64];
    __shared__ double sums[kSupNT / 64][4];
    const int tid = threadIdx.x, g = blockIdx.x;
    const int base = g * kSupSeg;
    const double inf = __builtin_inf();
    double km[kSupItems];
    int kid[kSupItems];
    double below = 0.0, bad = 0.0, its = 0.0, piv = 0.0;
#pragma unroll
    for (int i = 0; i < kSupItems; i++) {
        const int t = base + i * kSupNT + tid;   // (coalesced: consecutive threads, consecutive leaves)
        km[i] = inf;
        kid[i] = kSupNone;
        if (t < a.T) {
            const bool ok = a.status[t] == 0 && a.obj[t] == a.obj[t];
            const double mg = ok ? a.obj[t] - a.pi0 : inf;
            a.margin[t] = mg;
            km[i] = mg;
            kid[i] = ok ? (int)a.ids[t] : kSupNone;
            below += (ok && mg < -a.tol) ? 1.0 : 0.0;
            bad += ok ? 0.0 : 1.0;
            its += (double)a.iters[t];
            piv += (double)a.npivots[t];
        }
    }
    // (counts below 2^53: the sums are exact in any order)
    below = sup_wave_sum(below); bad = sup_wave_sum(bad); its = sup_wave_sum(its); piv = sup_wave_sum(piv);
    if ((tid & 63) == 0) { sums[tid >> 6][0] = below; sums[tid >> 6][1] = bad; sums[tid >> 6][2] = its; sums[tid >> 6][3] = piv; }
    __syncthreads();
    if (tid < 4) {
        double s = 0.0;
        for (int w = 0; w < kSupNT / 64; w++) s += sums[w][tid];
        a.seg_sum[(size_t)g * 4 + tid] = s;
    }
    double lm = -inf;
    int lid = -1;   // the last key taken: below every key
    for (int p = 0; p < a.P; p++) {
        SupKey k;
        k.m = inf; k.id = kSupNone; k.t = -1;
#pragma unroll
        for (int i = 0; i < kSupItems; i++) {
            const bool above = kid[i] != kSupNone && sup_less(lm, lid, km[i], kid[i]);
            if (above && sup_less(km[i], kid[i], k.m, k.id)) { k.m = km[i]; k.id = kid[i]; k.t = base + i * kSupNT + tid; }
        }
        k = sup_block_min(k, red);
        if (tid == 0) {
            const size_t o = (size_t)g * a.P + p;
            a.cand_m[o] = k.m; a.cand_id[o] = k.id; a.cand_t[o] = k.t;
        }
        lm = k.m; lid = k.id;   // (none left: kSupNone is above every id, nothing passes `above` again)
    }
}

__global__ void __launch_bounds__(kSupNT) support_select_merge(SupSelectArgs a) {
    __shared__ SupKey red[kSupNT / 64];
    __shared__ double sums[kSupNT / 64][4];
    __shared__ int sel_t[kSupMaxP];
    const int tid = threadIdx.x;
    const double inf = __builtin_inf();
    const int C = a.G * a.P;
    double s4[4] = {0.0, 0.0, 0.0, 0.0};
    for (int g = tid; g < a.G; g += kSupNT)
        for (int q = 0; q < 4; q++) s4[q] += a.seg_sum[(size_t)g * 4 + q];
    for (int q = 0; q < 4; q++) s4[q] = sup_wave_sum(s4[q]);
    if ((tid & 63) == 0)
        for (int q = 0; q < 4; q++) sums[tid >> 6][q] = s4[q];
    __syncthreads();
    double lm = -inf;
    int lid = -1, nsel = 0;
    double min_m = inf;
    int min_id = -1;
    for (int p = 0; p < a.P; p++) {
        SupKey k;
        k.m = inf; k.id = kSupNone; k.t = -1;
        for (int q = tid; q < C; q += kSupNT) {
            const double cm = a.cand_m[q];
            const int cid = a.cand_id[q];
            if (cid != kSupNone && sup_less(lm, lid, cm, cid) && sup_less(cm, cid, k.m, k.id)) { k.m = cm; k.id = cid; k.t = a.cand_t[q]; }
        }
        k = sup_block_min(k, red);
        if (k.id == kSupNone) break;   // (uniform: every thread holds the same k)
        if (p == 0) { min_m = k.m; min_id = k.id; }
        if (tid == 0) sel_t[p] = k.t;
        lm = k.m; lid = k.id;
        nsel = p + 1;
    }
    __syncthreads();
    if (tid == 0) {
        double tot[4];
        for (int q = 0; q < 4; q++) {
            tot[q] = 0.0;
            for (int w = 0; w < kSupNT / 64; w++) tot[q] += sums[w][q];
        }
        a.block[0] = min_m; a.block[1] = (double)min_id; a.block[2] = tot[0]; a.block[3] = (double)nsel;
        a.block[4] = tot[1]; a.block[5] = tot[2]; a.block[6] = tot[3]; a.block[7] = (double)a.T;
    }
    const size_t row = (size_t)a.n + 2;
    for (int p = 0; p < nsel; p++) {
        const int t = sel_t[p];
        if (t < 0 || t >= a.T) continue;   // (cannot happen: a candidate's position is a leaf's)
        double *out = a.block + kSupHead + (size_t)p * row;
        if (tid == 0) { out[0] = (double)a.ids[t]; out[1] = a.obj[t]; }
        const double *xr = a.x + (size_t)t * a.n;
        for (int j = tid; j < a.n; j += kSupNT) out[2 + j] = xr[j];
    }
}

}  // namespace mipx
