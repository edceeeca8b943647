// restart_kernels.hip.h -- seeding a restarted search (include/mipx_restart.h).
//   restart_seed  per seed: its pool row -- the root's bounds with the branchings of its lineage applied, and
//                 the root's basis codes (zeros, the slack basis, where there are none)
// One workgroup per seed, as treerec_bounds, with the same walk (tr_apply_lineage): column j belongs to
// thread j % 256 from its first store to its last, so the kernel needs no barrier and no atomic.  The rows
// are written straight into the pool in the pool's own layout (l, u: capacity x n; codes: capacity x nv); only
// the seeds' ids and rows come from the host.  Included by tree_engine.hip.h behind treerec_kernels.hip.h.
#pragma once
#include "treerec_kernels.hip.h"

namespace mipx {

struct RestartSeedArgs {
    int n = 0, nv = 0;
    int count = 0;                    // seeds of this launch
    int64_t nodes_count = 0;          // entries of the mirror
    int64_t capacity = 0;             // rows of the pool
    const TrNode *nodes = nullptr;
    const int64_t *ids = nullptr;     // count
    const int32_t *slots = nullptr;   // count: the seeds' pool rows
    const double *root_l = nullptr, *root_u = nullptr;   // n
    const int8_t *root_v = nullptr;   // nv basis codes, or null: a cold start
    double *pool_l = nullptr, *pool_u = nullptr;
    int8_t *pool_v = nullptr;
};

__global__ void __launch_bounds__(kTrNT) restart_seed(RestartSeedArgs g) {
    extern __shared__ uint8_t rs_seen[];   // n bytes: bit 0 an upper bound, bit 1 a lower bound was set
    const int k = blockIdx.x;
    if (k >= g.count) return;
    const int64_t slot = g.slots[k];
    if (slot < 0 || slot >= g.capacity) return;   // (the host hands out rows of the pool only)
    const int tid = threadIdx.x, n = g.n;
    double *lo = g.pool_l + (size_t)slot * n, *up = g.pool_u + (size_t)slot * n;
    for (int j = tid; j < n; j += kTrNT) {
        lo[j] = g.root_l[j];
        up[j] = g.root_u[j];
        rs_seen[j] = 0;
    }
    int8_t *codes = g.pool_v + (size_t)slot * g.nv;
    for (int j = tid; j < g.nv; j += kTrNT) codes[j] = g.root_v != nullptr ? g.root_v[j] : (int8_t)0;
    tr_apply_lineage(g.nodes, g.nodes_count, g.ids[k], n, tid, lo, up, rs_seen);
}

}  // namespace mipx
