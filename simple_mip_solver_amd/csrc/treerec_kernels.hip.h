// treerec_kernels.hip.h -- the tree record of a frontier-engine search (include/mipx_treerec.h).
//   treerec_bounds  per requested node: the root's bounds with the branchings of its lineage applied
// One workgroup per node.  Column j belongs to thread j % 256 from the first store to the last, so the
// kernel needs no barrier and no atomic: the lineage is walked by every thread (uniform loads of one
// 16-byte entry per level), and only the owner of the branched column acts.  The walk goes from the node
// up to the root; the search applied the branchings the other way round, each one overwriting the bound
// (make_children / finish_write), so the first branching met on a column's side is the one that stands --
// one LDS byte per column remembers which sides have been met.  Included by tree_engine.hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mipx {

constexpr int kTrNT = 256;

// the device mirror of a record: what the walk needs, one aligned 16-byte load per level
struct TrNode {
    int32_t parent;   // -1 at the root
    int32_t vd;       // 2 * variable + direction (0 left, 1 right)
    double val;       // the parent's x[variable]
};

struct TrBoundsArgs {
    int n = 0, nv = 0;
    int count = 0;                    // nodes of this launch
    int64_t nodes_count = 0;          // entries of the mirror
    const TrNode *nodes = nullptr;
    const int64_t *ids = nullptr;     // count
    const double *root_l = nullptr, *root_u = nullptr;   // n
    const int8_t *root_v = nullptr;   // nv basis codes, copied to out_v where both are given
    double *out_l = nullptr, *out_u = nullptr;           // count x n
    int8_t *out_v = nullptr;          // count x nv
};

// The walk of node `id`'s lineage over rows lo / up that hold the root's bounds, `seen` zeroed: thread tid acts
// on the columns j with j % kTrNT == tid only (it must be the thread that initialised them).  Shared by
// treerec_bounds and restart_seed (restart_kernels.hip.h), so that the two write the same bits.
__device__ __forceinline__ void tr_apply_lineage(const TrNode *nodes, int64_t nodes_count, int64_t id, int n, int tid,
                                                 double *lo, double *up, uint8_t *seen) {
    while (id > 0 && id < nodes_count) {   // (a parent's id is below its child's: the walk ends at 0)
        const TrNode r = nodes[id];
        const int var = r.vd >> 1, right = r.vd & 1;
        // (the ownership test is what "no barrier, no atomic" rests on; without it the outputs differ only when a store
        // overtakes the owner's initialisation, so tests/test_node_rows_abi.py reads it here:
        // test_the_lineage_walk_keeps_its_ownership_rule)
        if (var >= 0 && var < n && (var % kTrNT) == tid) {
            const uint8_t bit = (uint8_t)(1 << right);
            if (!(seen[var] & bit)) {
                seen[var] |= bit;
                if (right) lo[var] = ceil(r.val);
                else up[var] = floor(r.val);
            }
        }
        id = r.parent < id ? r.parent : -1;
    }
}

__global__ void __launch_bounds__(kTrNT) treerec_bounds(TrBoundsArgs g) {
    extern __shared__ uint8_t tr_seen[];   // n bytes: bit 0 an upper bound, bit 1 a lower bound was set
    const int k = blockIdx.x;
    if (k >= g.count) return;
    const int tid = threadIdx.x, n = g.n;
    double *lo = g.out_l + (size_t)k * n, *up = g.out_u + (size_t)k * n;
    for (int j = tid; j < n; j += kTrNT) {
        lo[j] = g.root_l[j];
        up[j] = g.root_u[j];
        tr_seen[j] = 0;
    }
    if (g.out_v != nullptr && g.root_v != nullptr)
        for (int j = tid; j < g.nv; j += kTrNT) g.out_v[(size_t)k * g.nv + j] = g.root_v[j];
    tr_apply_lineage(g.nodes, g.nodes_count, g.ids[k], n, tid, lo, up, tr_seen);
}

}  // namespace mipx
