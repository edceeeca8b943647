// cutmig_kernels.hip.h -- the cut rows of migrated nodes (include/mipx_cutmig.h): the donor's cut lists
// for the host, store rows -> the message's cut table, the table -> the receiver's migration region, and
// the receiver's cut lists.  Bandwidth kernels, one wave64 per record or row, four per block: the 64 lanes
// walk a row of n f64 64 columns at a time (coalesced 512 B loads and stores).  The rows and basis codes of
// the nodes travel through pack_nodes / unpack_nodes as without cut rounds.  Included by tree_engine.hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mipx {

struct CutMigArgs {
    int n = 0, kc = 0, count = 0;            // count: records (list kernels) or table rows (row kernels)
    const int32_t *slot = nullptr;           // record k <-> pool row slot[k]
    int32_t *pool_ncut = nullptr, *pool_ids = nullptr;   // the node pool's cut lists
    int32_t *lists = nullptr;                // count x (1 + kc): [ncut, store ids (donor) | table refs (message)]
    const int32_t *src = nullptr;            // gather: store id of table row r
    double *store_pi = nullptr, *store_pi0 = nullptr;    // the cut store
    double *tab_pi = nullptr, *tab_pi0 = nullptr;        // the message's cut table: count x n, count
    int64_t base = 0;                        // scatter / unpack: the first region row this message fills
    int ctab = 0;                            // unpack: table rows in the message (every ref is below)
    int32_t *bad = nullptr;                  // unpack: counts the records whose list does not fit
};

// donor: the cut lists of the candidates' pool rows, [ncut, id_0 .. id_{kc-1}] per record (ids past ncut 0)
__global__ __launch_bounds__(256) void cutmig_lists(CutMigArgs a) {
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= a.count) return;
    const size_t s = (size_t)a.slot[k];
    const int nc = a.pool_ncut[s];
    int32_t *out = a.lists + (size_t)k * (1 + a.kc);
    if (lane == 0) out[0] = nc;
    for (int j = lane; j < a.kc; j += 64) out[1 + j] = j < nc ? a.pool_ids[s * a.kc + j] : 0;
}

// donor: table row r <- store row src[r]
__global__ __launch_bounds__(256) void cutmig_gather(CutMigArgs a) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= a.count) return;
    const size_t id = (size_t)a.src[r];
    const double *s = a.store_pi + id * a.n;
    double *d = a.tab_pi + (size_t)r * a.n;
    for (int j = lane; j < a.n; j += 64) d[j] = s[j];
    if (lane == 0) a.tab_pi0[r] = a.store_pi0[id];
}

// receiver: store row base + r <- table row r
__global__ __launch_bounds__(256) void cutmig_scatter(CutMigArgs a) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= a.count) return;
    const size_t id = (size_t)(a.base + r);
    const double *s = a.tab_pi + (size_t)r * a.n;
    double *d = a.store_pi + id * a.n;
    for (int j = lane; j < a.n; j += 64) d[j] = s[j];
    if (lane == 0) a.store_pi0[id] = a.tab_pi0[r];
}

// receiver: the records' lists into their new pool rows, refs -> region rows (base + ref), in list order.
// A list that does not fit (ncut outside 0..kc, a ref outside the table) is counted in *bad and the node gets
// no cut row, so that no id can point outside what this message filled.  kc <= 64: one lane per entry.
__global__ __launch_bounds__(256) void cutmig_unpack_lists(CutMigArgs a) {
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= a.count) return;
    const size_t s = (size_t)a.slot[k];
    const int32_t *in = a.lists + (size_t)k * (1 + a.kc);
    const int nc = in[0];
    const bool nc_ok = nc >= 0 && nc <= a.kc;
    const int ref = (nc_ok && lane < nc) ? in[1 + lane] : 0;
    const bool ok = __all(nc_ok && (lane >= nc || (ref >= 0 && ref < a.ctab)));   // (every lane of the wave is here)
    if (ok && lane < nc) a.pool_ids[s * a.kc + lane] = (int32_t)(a.base + ref);
    if (lane == 0) {
        a.pool_ncut[s] = ok ? nc : 0;
        if (!ok) atomicAdd(a.bad, 1);
    }
}

}  // namespace mipx
