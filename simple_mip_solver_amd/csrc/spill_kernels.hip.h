// spill_kernels.hip.h -- compact node records (include/mipx_spill.h): count, scan, pack, unpack.
// Bandwidth kernels, one wave64 per record: a wave walks its row 64 columns at a time (coalesced 512 B
// reads of l and u), finds the columns that differ from the root's bounds with a ballot and places them
// with a popcount of the lower lanes.  They run on their own stream, off the node-LP critical path.
// Included by mipx.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mipx {

struct SpillArgs {
    int n = 0, nv = 0, kc = 0, count = 0;   // kc > 0: cut mode
    const double *root_l = nullptr, *root_u = nullptr;
    double *l = nullptr, *u = nullptr;      // rows of n (the pool, or a staging block)
    int8_t *v = nullptr;                    // rows of nv basis codes
    int32_t *ncut = nullptr, *ids = nullptr;   // cut mode: per row the count and kc ids
    const int32_t *slot = nullptr;          // record r <-> row slot[r] (nullptr: row r)
    const int64_t *node_id = nullptr;       // header ids (nullptr: r)
    int64_t *off = nullptr;                 // count + 1: record sizes (spill_count), then byte offsets (spill_scan)
    char *rec = nullptr;                    // the records
};

__host__ __device__ inline int64_t spill_pad8(int64_t b) { return (b + 7) & ~(int64_t)7; }
__host__ __device__ inline int64_t spill_record_bytes(int ndiff, int ncut, int nv, int kc) {
    return 16 + spill_pad8(4 * (int64_t)ndiff) + 16 * (int64_t)ndiff + spill_pad8((nv + 1) / 2) +
           (kc > 0 ? spill_pad8(4 * (int64_t)ncut) : 0);
}

__device__ inline bool spill_differs(double a, double b) {
    return __double_as_longlong(a) != __double_as_longlong(b);
}
__device__ inline uint64_t spill_lanes_below() {
    const unsigned lane = threadIdx.x & 63;
    return lane == 0 ? 0ull : (~0ull >> (64 - lane));
}

// one wave per record: its size, from the diff count
__global__ void __launch_bounds__(256) spill_count(SpillArgs a) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= a.count) return;
    const size_t row = a.slot ? (size_t)a.slot[r] : (size_t)r;
    const double *l = a.l + row * a.n, *u = a.u + row * a.n;
    int nd = 0;
    for (int c0 = 0; c0 < a.n; c0 += 64) {
        const int j = c0 + lane;
        const bool d = j < a.n && (spill_differs(l[j], a.root_l[j]) || spill_differs(u[j], a.root_u[j]));
        nd += __popcll(__ballot(d));
    }
    if (lane == 0) a.off[r] = spill_record_bytes(nd, a.kc > 0 ? a.ncut[row] : 0, a.nv, a.kc);
}

// sizes -> exclusive offsets in place, off[count] = total.  One block: each thread scans a run of count / 1024
// records serially (a spill event moves 10^4..10^6 records; this reads and writes 8 bytes of each)
__global__ void __launch_bounds__(1024) spill_scan(SpillArgs a) {
    __shared__ int64_t part[1024];
    const int t = threadIdx.x, N = a.count;
    const int per = (N + 1023) / 1024, b = t * per, e = min(N, b + per);
    int64_t s = 0;
    for (int k = b; k < e; k++) s += a.off[k];
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {   // inclusive Hillis-Steele scan of the per-thread sums
        const int64_t v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int64_t run = part[t] - s;
    for (int k = b; k < e; k++) {
        const int64_t sz = a.off[k];
        a.off[k] = run;
        run += sz;
    }
    if (t == 1023) a.off[N] = part[1023];
}

__global__ void __launch_bounds__(256) spill_pack(SpillArgs a) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= a.count) return;
    const size_t row = a.slot ? (size_t)a.slot[r] : (size_t)r;
    const double *l = a.l + row * a.n, *u = a.u + row * a.n;
    const int ncut = a.kc > 0 ? a.ncut[row] : 0;
    char *p = a.rec + a.off[r];
    const int nd = (int)((a.off[r + 1] - a.off[r] - 16 - spill_pad8((a.nv + 1) / 2) -
                          (a.kc > 0 ? spill_pad8(4 * (int64_t)ncut) : 0)) / 20);   // (16 + 4 nd + pad = size: pad < 8)
    const int64_t o_l = 16 + spill_pad8(4 * (int64_t)nd), o_u = o_l + 8 * (int64_t)nd, o_v = o_u + 8 * (int64_t)nd;
    int32_t *col = (int32_t *)(p + 16);
    double *dl = (double *)(p + o_l), *du = (double *)(p + o_u);
    if (lane == 0) {
        *(int64_t *)p = a.node_id ? a.node_id[r] : (int64_t)r;
        ((int32_t *)p)[2] = nd;
        ((int32_t *)p)[3] = ncut;
        if (nd & 1) col[nd] = 0;   // (pad of the column list)
    }
    int base = 0;
    for (int c0 = 0; c0 < a.n; c0 += 64) {
        const int j = c0 + lane;
        double lj = 0.0, uj = 0.0;
        bool d = false;
        if (j < a.n) {
            lj = l[j]; uj = u[j];
            d = spill_differs(lj, a.root_l[j]) || spill_differs(uj, a.root_u[j]);
        }
        const uint64_t mask = __ballot(d);
        if (d) {
            const int k = base + __popcll(mask & spill_lanes_below());
            col[k] = j; dl[k] = lj; du[k] = uj;
        }
        base += __popcll(mask);
    }
    // basis codes, two per byte; the section's zero pad included
    const int8_t *v = a.v + row * a.nv;
    uint8_t *code = (uint8_t *)(p + o_v);
    const int nb = (int)spill_pad8((a.nv + 1) / 2);
    for (int b = lane; b < nb; b += 64) {
        const int j = 2 * b;
        uint8_t c = 0;
        if (j < a.nv) c = (uint8_t)(v[j] & 0xF);
        if (j + 1 < a.nv) c |= (uint8_t)((v[j + 1] & 0xF) << 4);
        code[b] = c;
    }
    if (a.kc > 0) {
        int32_t *cid = (int32_t *)(p + o_v + nb);
        const int32_t *ids = a.ids + row * a.kc;
        const int nc = (int)(spill_pad8(4 * (int64_t)ncut) / 4);
        for (int k = lane; k < nc; k += 64) cid[k] = k < ncut ? ids[k] : 0;
    }
}

__global__ void __launch_bounds__(256) spill_unpack(SpillArgs a) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= a.count) return;
    const size_t row = a.slot ? (size_t)a.slot[r] : (size_t)r;
    double *l = a.l + row * a.n, *u = a.u + row * a.n;
    const char *p = a.rec + a.off[r];
    const int nd = ((const int32_t *)p)[2], ncut = ((const int32_t *)p)[3];
    const int64_t o_l = 16 + spill_pad8(4 * (int64_t)nd), o_u = o_l + 8 * (int64_t)nd, o_v = o_u + 8 * (int64_t)nd;
    const int32_t *col = (const int32_t *)(p + 16);
    const double *dl = (const double *)(p + o_l), *du = (const double *)(p + o_u);
    // 64 columns at a time: the diffs that fall into them are the next <= 64 of the ascending list; a lane
    // writes its column once, the diff's value or the root's
    int k0 = 0;
    for (int c0 = 0; c0 < a.n; c0 += 64) {
        const int k = k0 + lane;
        const int c = k < nd ? col[k] : a.n;
        const bool in = k < nd && c < c0 + 64;   // (ascending, and >= c0: the earlier ones were consumed)
        const uint64_t inmask = __ballot(in);
        // which columns of the chunk have a diff, and from which list entry: a wave-wide OR of one bit each
        uint64_t have = in ? (1ull << (c - c0)) : 0ull;
        for (int s = 1; s < 64; s <<= 1) have |= (uint64_t)__shfl_xor((long long)have, s);
        const int j = c0 + lane;
        if (j < a.n) {
            if ((have >> lane) & 1) {
                const int kk = k0 + __popcll(have & spill_lanes_below());   // the list is ascending
                l[j] = dl[kk]; u[j] = du[kk];
            } else {
                l[j] = a.root_l[j]; u[j] = a.root_u[j];
            }
        }
        k0 += __popcll(inmask);
    }
    int8_t *v = a.v + row * a.nv;
    const uint8_t *code = (const uint8_t *)(p + o_v);
    const int nb = (a.nv + 1) / 2;
    for (int b = lane; b < nb; b += 64) {
        const uint8_t c = code[b];
        const int j = 2 * b;
        v[j] = (int8_t)((int8_t)(c << 4) >> 4);   // (sign-extended 4 bits)
        if (j + 1 < a.nv) v[j + 1] = (int8_t)((int8_t)c >> 4);
    }
    if (a.kc > 0) {
        if (lane == 0) a.ncut[row] = ncut;
        const int32_t *cid = (const int32_t *)(p + o_v + spill_pad8(nb));
        int32_t *ids = a.ids + row * a.kc;
        for (int k = lane; k < ncut; k += 64) ids[k] = cid[k];
    }
}

// rows slot[k] of a pool into rows k of a block shaped like it (rows with slot < 0 are left alone): mipx_tree_reanchor
// gathers resident nodes beside the spilled ones it decodes
__global__ void __launch_bounds__(256) spill_gather_rows(SpillArgs a, const double *src_l, const double *src_u,
                                                         const int8_t *src_v) {
    const int k = blockIdx.x;
    if (k >= a.count || a.slot[k] < 0) return;
    const size_t s = (size_t)a.slot[k];
    for (int j = threadIdx.x; j < a.n; j += 256) {
        a.l[(size_t)k * a.n + j] = src_l[s * a.n + j];
        a.u[(size_t)k * a.n + j] = src_u[s * a.n + j];
    }
    for (int j = threadIdx.x; j < a.nv; j += 256) a.v[(size_t)k * a.nv + j] = src_v[s * a.nv + j];
}

}  // namespace mipx
