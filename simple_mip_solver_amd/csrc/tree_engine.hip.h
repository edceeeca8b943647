// tree_engine.hip.h -- native frontier engine: the BranchAndBound.solve() loop of the reference
// (simple_mip_solver/algorithms/branch_and_bound.py:215-266) with the stock node classes
// (BaseNode / PseudoCostBranchNode, best-first or depth-first), processing a BATCH of open nodes
// per step on the GPU.  Node records (bounds + warm-start basis) live in a device-resident pool;
// the host keeps only the priority queue and 48 bytes of bookkeeping per node.
//
// frontier_batch = 1 reproduces the reference's node order exactly (the queue is a re-statement of
// CPython's heapq, which queue.PriorityQueue uses), including pseudo-cost table evolution; larger
// batches evaluate the B best open nodes per step against the table as of the start of the step.
// Included by mipx.hip (needs mipx_ctx, mipx_problem, pick_cfg, HIP_TRY, fail).
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <limits>
#include <memory>
#include <queue>
#include <unordered_map>

#include "tree_kernels.hip.h"
#include "finish_kernels.hip.h"
#include "cutmig_kernels.hip.h"
#include "dualfn_kernels.hip.h"
#include "treerec_kernels.hip.h"
#include "restart_kernels.hip.h"
#include "heur_kernels.hip.h"
#include "lsearch_kernels.hip.h"
#include "fixprop_kernels.hip.h"
#include "wrepair_kernels.hip.h"
#include "cube_kernels.hip.h"
#include "complete_kernels.hip.h"
#include "lpdive_kernels.hip.h"
#include "prop_kernels.hip.h"
#include "rcfix_kernels.hip.h"
#include "cglp_kernels.hip.h"
#include "cglp_screen_kernels.hip.h"
#include "step_layout.h"

// The one launch site of each kernel that moves node rows (make_children, the message kernels, the lineage kernels,
// the cut-migration kernels, the spill kernels): grid, block and LDS rule live here.  `count` -- records, rows or
// (parent, variable) pairs -- is set into the args here and nowhere else: the callers leave a.count alone.  The engine and the entries of include/mipx_noderows.h
// (noderows_api.hip.h) both launch through these, so the tests of those entries run the engine's launches.
namespace {
inline unsigned rows_grid4(int count) { return (unsigned)(((int64_t)count + 3) / 4); }   // one wave64 per record, four per block

void enqueue_make_children(mipx::ChildArgs a, int count, hipStream_t st) {
    a.count = count;
    hipLaunchKernelGGL(mipx::make_children, dim3(2 * (unsigned)count), dim3(256), 0, st, a);
}
void enqueue_pack_nodes(mipx::PackArgs a, int count, hipStream_t st) {
    a.count = count;
    hipLaunchKernelGGL(mipx::pack_nodes, dim3((unsigned)count), dim3(256), 0, st, a);
}
void enqueue_unpack_nodes(mipx::PackArgs a, int count, hipStream_t st) {
    a.count = count;
    hipLaunchKernelGGL(mipx::unpack_nodes, dim3((unsigned)count), dim3(256), 0, st, a);
}
void enqueue_gather_plain_nodes(mipx::PlainGatherArgs a, int count, hipStream_t st) {
    a.count = count;
    hipLaunchKernelGGL(mipx::gather_plain_nodes, dim3((unsigned)count), dim3(256), 0, st, a);
}
// (the lineage kernels keep one byte per column in LDS: n bytes)
void enqueue_treerec_bounds(mipx::TrBoundsArgs a, int count, hipStream_t st) {
    a.count = count;
    hipLaunchKernelGGL(mipx::treerec_bounds, dim3((unsigned)count), dim3(mipx::kTrNT), (size_t)a.n, st, a);
}
void enqueue_restart_seed(mipx::RestartSeedArgs a, int count, hipStream_t st) {
    a.count = count;
    hipLaunchKernelGGL(mipx::restart_seed, dim3((unsigned)count), dim3(mipx::kTrNT), (size_t)a.n, st, a);
}
void enqueue_cutmig_lists(mipx::CutMigArgs a, int count, hipStream_t st) {
    a.count = count;
    hipLaunchKernelGGL(mipx::cutmig_lists, dim3(rows_grid4(count)), dim3(256), 0, st, a);
}
void enqueue_cutmig_gather(mipx::CutMigArgs a, int count, hipStream_t st) {
    a.count = count;
    hipLaunchKernelGGL(mipx::cutmig_gather, dim3(rows_grid4(count)), dim3(256), 0, st, a);
}
void enqueue_cutmig_scatter(mipx::CutMigArgs a, int count, hipStream_t st) {
    a.count = count;
    hipLaunchKernelGGL(mipx::cutmig_scatter, dim3(rows_grid4(count)), dim3(256), 0, st, a);
}
void enqueue_cutmig_unpack_lists(mipx::CutMigArgs a, int count, hipStream_t st) {
    a.count = count;
    hipLaunchKernelGGL(mipx::cutmig_unpack_lists, dim3(rows_grid4(count)), dim3(256), 0, st, a);
}
// sizes (spill_count), then their exclusive offsets in place (spill_scan): a.off holds count + 1 entries
void enqueue_spill_count(mipx::SpillArgs a, int count, hipStream_t st) {
    a.count = count;
    hipLaunchKernelGGL(mipx::spill_count, dim3(rows_grid4(count)), dim3(256), 0, st, a);
}
void enqueue_spill_scan(mipx::SpillArgs a, int count, hipStream_t st) {
    a.count = count;
    hipLaunchKernelGGL(mipx::spill_scan, dim3(1), dim3(1024), 0, st, a);
}
void enqueue_spill_pack(mipx::SpillArgs a, int count, hipStream_t st) {
    a.count = count;
    hipLaunchKernelGGL(mipx::spill_pack, dim3(rows_grid4(count)), dim3(256), 0, st, a);
}
void enqueue_spill_unpack(mipx::SpillArgs a, int count, hipStream_t st) {
    a.count = count;
    hipLaunchKernelGGL(mipx::spill_unpack, dim3(rows_grid4(count)), dim3(256), 0, st, a);
}
void enqueue_spill_gather_rows(mipx::SpillArgs a, int count, hipStream_t st, const double *src_l, const double *src_u,
                               const int8_t *src_v) {
    a.count = count;
    hipLaunchKernelGGL(mipx::spill_gather_rows, dim3((unsigned)count), dim3(256), 0, st, a, src_l, src_u, src_v);
}

// The one launch site of each kernel behind a support evaluation (cglp_kernels.hip.h, cglp_screen_kernels.hip.h):
// the leaves T (or the packed leaves `count`) and the segments G are set into the args here and nowhere else, and
// the grid follows from them.  The session (cglp_api.hip.h), mipx_support_screen_batch and the entries of
// include/mipx_supportkernels.h (supportkernels_api.hip.h) all launch through these.
inline int sup_segments(int64_t T) { return (int)((T + mipx::kSupSeg - 1) / mipx::kSupSeg); }
static_assert(mipx::kSupSeg == mipx::kScrSeg, "the selection and the pack kernels share their segments");

void enqueue_support_screen(mipx::SupScreenArgs a, int T, hipStream_t st) {   // one wave64 per leaf
    a.T = T;
    hipLaunchKernelGGL(mipx::support_screen, dim3((unsigned)((T + mipx::kScrWaves - 1) / mipx::kScrWaves)), dim3(mipx::kScrNT), 0, st, a);
}
void enqueue_support_pack_count(mipx::SupPackArgs a, int T, hipStream_t st) {
    a.T = T; a.G = sup_segments(T);
    hipLaunchKernelGGL(mipx::support_pack_count, dim3((unsigned)a.G), dim3(mipx::kScrNT), 0, st, a);
}
void enqueue_support_pack(mipx::SupPackArgs a, int T, hipStream_t st) {
    a.T = T; a.G = sup_segments(T);
    hipLaunchKernelGGL(mipx::support_pack, dim3((unsigned)a.G), dim3(mipx::kScrNT), 0, st, a);
}
void enqueue_support_gather(mipx::SupMoveArgs a, int count, hipStream_t st) {   // one workgroup per packed leaf
    a.count = count;
    hipLaunchKernelGGL(mipx::support_gather, dim3((unsigned)count), dim3(mipx::kScrNT), 0, st, a);
}
void enqueue_support_scatter(mipx::SupMoveArgs a, int count, hipStream_t st) {
    a.count = count;
    hipLaunchKernelGGL(mipx::support_scatter, dim3((unsigned)count), dim3(mipx::kScrNT), 0, st, a);
}
void enqueue_support_mark(int T, const int32_t *status, uint8_t *has_y, hipStream_t st) {
    hipLaunchKernelGGL(mipx::support_mark, dim3((unsigned)((T + mipx::kScrNT - 1) / mipx::kScrNT)), dim3(mipx::kScrNT), 0, st, T, status, has_y);
}
void enqueue_support_select(mipx::SupSelectArgs a, int T, hipStream_t st) {
    a.T = T; a.G = sup_segments(T);
    hipLaunchKernelGGL(mipx::support_select, dim3((unsigned)a.G), dim3(mipx::kSupNT), 0, st, a);
}
void enqueue_support_select_merge(mipx::SupSelectArgs a, int T, hipStream_t st) {   // one workgroup over the segments' candidates
    a.T = T; a.G = sup_segments(T);
    hipLaunchKernelGGL(mipx::support_select_merge, dim3(1), dim3(mipx::kSupNT), 0, st, a);
}
}  // namespace

struct NodeRec {
    double key;          // queue key: dual bound (best first) or -depth (depth first)
    double dual_bound;   // bound inherited from the parent (parent's LP objective)
    double b_val;
    int32_t slot;        // row in the device pool, -1 once released, <= -2 on the host (host spill: entry -2 - slot)
    int32_t depth;
    int32_t b_idx;       // variable branched on to create this node (-1 root)
    int32_t b_dir;       // 0 left (x <= floor), 1 right (x >= ceil)
    int32_t anchor;      // entry of the anchor table its warm start refactors from (-1: the root's)
    int32_t born;        // step that created the node (MIPX_TREE_PROFILE: age histogram)
    int32_t ncut;        // cut rows the node carries (cut rounds: inherited from its parent)
    // (no default initialisers: a fresh block of the node table must not be touched page by page)
};

// The node table: every node ever created, indexed by id.  Blocks of 2^18 records instead of one
// vector: growing never copies (a 5 M-node table is 240 MB -- one reallocation stalled the step
// loop for 59 ms).
struct NodeTable {
    static constexpr int kShift = 18;
    static constexpr size_t kMask = ((size_t)1 << kShift) - 1;
    std::vector<std::unique_ptr<NodeRec[]>> blocks;
    size_t n = 0;
    NodeRec &operator[](size_t i) { return blocks[i >> kShift][i & kMask]; }
    const NodeRec &operator[](size_t i) const { return blocks[i >> kShift][i & kMask]; }
    void push_back(const NodeRec &r) {
        if ((n >> kShift) == blocks.size()) blocks.emplace_back(new NodeRec[(size_t)1 << kShift]);
        (*this)[n++] = r;
    }
    size_t size() const { return n; }
};

// CPython's heapq on node ids (Lib/heapq.py heappush/heappop/_siftdown/_siftup), so that ties are
// broken exactly as queue.PriorityQueue breaks them in the reference.
struct PyHeap {
    struct Item { double key; int64_t id; };
    std::vector<Item> h;   // keys inline: sifting never touches the node table
    static bool lt(const Item &a, const Item &b) { return a.key < b.key; }
    void siftdown(size_t startpos, size_t pos) {
        const Item item = h[pos];
        while (pos > startpos) {
            const size_t parent = (pos - 1) >> 1;
            if (lt(item, h[parent])) { h[pos] = h[parent]; pos = parent; continue; }
            break;
        }
        h[pos] = item;
    }
    void siftup(size_t pos) {
        const size_t end = h.size(), start = pos;
        const Item item = h[pos];
        size_t child = 2 * pos + 1;
        while (child < end) {
            const size_t right = child + 1;
            if (right < end && !lt(h[child], h[right])) child = right;
            h[pos] = h[child];
            pos = child;
            child = 2 * pos + 1;
        }
        h[pos] = item;
        siftdown(start, pos);
    }
    void push(double key, int64_t id) { h.push_back({key, id}); siftdown(0, h.size() - 1); }
    int64_t pop() {
        const Item last = h.back();
        h.pop_back();
        if (h.empty()) return last.id;
        const Item top = h[0];
        h[0] = last;
        siftup(0);
        return top.id;
    }
    bool empty() const { return h.empty(); }
    size_t size() const { return h.size(); }
};

// Open list of the batched best-first search (frontier batches > 1): a step takes the B smallest
// keys at once, so per-node heap order is not needed.  Keys are bucketed linearly above the first
// (smallest: a child's bound is never below its parent's) key; a step empties whole buckets in
// key order and splits the last one exactly with nth_element.  O(1) pushes, O(B) per step, where
// the binary heap paid ~0.1 us per push and pop in cache misses.
struct BucketQueue {
    struct Item { double key; int64_t id; };
    static constexpr size_t kMaxBuckets = (size_t)1 << 22;
    std::vector<std::vector<Item>> tab;
    double k0 = 0.0, inv_width = 0.0;
    size_t cur = 0, count = 0;
    bool started = false;
    size_t index(double key) const {
        const double r = (key - k0) * inv_width;
        if (!(r > 0.0)) return 0;
        return r >= (double)(kMaxBuckets - 1) ? kMaxBuckets - 1 : (size_t)r;
    }
    void push(double key, int64_t id) {
        if (!started && !hold && std::isfinite(key)) {  // (the root's inherited bound is -inf: bucket 0)
            started = true;
            k0 = key;
            inv_width = 4096.0 / std::fmax(std::fabs(key), 1.0);  // bucket width: 2^-12 of |first key|
        }
        const size_t i = started ? index(key) : 0;
        if (i >= tab.size()) tab.resize(i + 1 + (i >> 3));
        tab[i].push_back({key, id});
        if (count == 0 || i < cur) cur = i;
        count++;
    }
    // A step's pushes in one go, in the given order (the queue ends up exactly as after the pushes one by
    // one): a push lands in one of 10^5 buckets -- the header of its vector and the cache line of its tail
    // are two misses -- so the headers are prefetched 16 items ahead and the tails 8 ahead.
    void push_many(const Item *it, size_t cnt) {
        if (cnt == 0) return;
        if (!started) {   // (the scale comes from the first finite key: let the one-by-one path set it)
            for (size_t k = 0; k < cnt; k++) push(it[k].key, it[k].id);
            return;
        }
        size_t hi = 0;
        for (size_t k = 0; k < cnt; k++) hi = std::max(hi, index(it[k].key));
        if (hi >= tab.size()) tab.resize(hi + 1 + (hi >> 3));
        constexpr size_t A = 16, Bd = 8;
        for (size_t k = 0; k < cnt + A; k++) {
            if (k < cnt) __builtin_prefetch(&tab[index(it[k].key)], 1);
            if (k >= A - Bd && k - (A - Bd) < cnt) {
                const std::vector<Item> &v = tab[index(it[k - (A - Bd)].key)];
                if (!v.empty()) __builtin_prefetch(v.data() + v.size(), 1);
            }
            if (k >= A) {
                const Item &e = it[k - A];
                const size_t i = index(e.key);
                tab[i].push_back(e);
                if (count == 0 || i < cur) cur = i;
                count++;
            }
        }
    }
    bool empty() const { return count == 0; }
    size_t size() const { return count; }
    void settle() { while (cur < tab.size() && tab[cur].empty()) cur++; }
    double min_key() {
        settle();
        double k = std::numeric_limits<double>::infinity();
        for (const Item &it : tab[cur]) k = std::fmin(k, it.key);
        return k;
    }
    // Restart (mipx_restart.h): the seeds are keyed -inf and their children's keys come in no order, so the
    // first finite key is not the smallest.  While a seed is in the queue there is no scale -- everything
    // lies in bucket 0, split exactly by pop_batch -- and the scale is set from the smallest key once the
    // last seed has left.
    bool hold = false;
    void release_hold() {
        const double inf = std::numeric_limits<double>::infinity();
        if (tab.empty()) return;
        double mn = inf;
        for (const Item &it : tab[0]) {
            if (it.key == -inf) return;   // (a seed is still there)
            mn = std::fmin(mn, it.key);
        }
        if (!std::isfinite(mn)) return;
        hold = false;
        std::vector<Item> all;
        all.swap(tab[0]);
        count = 0;
        cur = 0;
        started = true;   // the scale push() would take from a first key, from the smallest one
        k0 = mn;
        inv_width = 4096.0 / std::fmax(std::fabs(mn), 1.0);
        for (const Item &it : all) push(it.key, it.id);
    }
    // the `want` smallest items (ties: smaller id first) are appended to out
    void pop_batch(size_t want, std::vector<Item> &out) {
        if (hold) release_hold();
        while (want > 0 && count > 0) {
            settle();
            std::vector<Item> &v = tab[cur];
            if (v.size() <= want) {
                out.insert(out.end(), v.begin(), v.end());
                want -= v.size();
                count -= v.size();
                v.clear();
            } else if (started && v.size() > 8 * want && tab.size() * 16 < kMaxBuckets && refinements < max_refinements) {
                // (before the first finite key there is no scale to refine: the seeds of a restart, all keyed -inf)
                // a deep search piles its open nodes just above the dual bound: buckets sized for
                // the first key end up holding 10^5..10^6 of them and every step pays nth_element
                // and an erase over all of those (2.7 ms per step at 5 M open nodes) -> finer buckets
                refine();
            } else {
                auto less = [](const Item &a, const Item &b) { return a.key < b.key || (a.key == b.key && a.id < b.id); };
                std::nth_element(v.begin(), v.begin() + (std::ptrdiff_t)want, v.end(), less);
                out.insert(out.end(), v.begin(), v.begin() + (std::ptrdiff_t)want);
                v.erase(v.begin(), v.begin() + (std::ptrdiff_t)want);
                count -= want;
                want = 0;
            }
        }
    }
    int refinements = 0;
    // (two refinements = 256 x finer than the first scale: beyond that the pushes of a step scatter
    // over 10^5 bucket tails and the bookkeeping pays in cache misses what the pop saves)
    int max_refinements = std::getenv("MIPX_BQ_REFINE") ? std::atoi(std::getenv("MIPX_BQ_REFINE")) : 2;
    void refine() {  // 16 x finer buckets, same order of the items inside the new buckets' sources
        std::vector<std::vector<Item>> old;
        old.swap(tab);
        inv_width *= 16.0;
        count = 0;
        cur = 0;
        refinements++;
        for (const auto &v : old)
            for (const Item &it : v) push(it.key, it.id);
    }
    // every item, in bucket order (for peek / sharding)
    void items(std::vector<Item> &out) const {
        for (size_t i = cur; i < tab.size(); i++) out.insert(out.end(), tab[i].begin(), tab[i].end());
    }
    void clear() {
        for (auto &v : tab) v.clear();
        count = 0;
        cur = 0;
    }
    // (the bucket scale -- k0, width, refinements -- survives a clear: keep_shard refills the queue)
};

// Per-step device outputs and host staging, double-buffered so that the host bookkeeping of step
// k overlaps the node-LP kernel of step k+1 (frontier batches > 1).
struct StepBuf {
    int32_t *d_slot = nullptr, *d_iters = nullptr, *d_plist = nullptr;
    double *d_x = nullptr;
    int8_t *d_vout = nullptr;
    // what the host reads back every step, packed so that ONE copy into pinned memory fetches it: the layout in
    // use (for the tree's dive depth) and its device view, both set by layout_pack
    char *d_pack = nullptr, *h_pack = nullptr;
    step_layout::StepPack pack{1, 0, 0, 0};
    step_layout::StepPack::View<char> d{};
    int32_t *h_slot = nullptr;  // pinned staging of the batch's pool rows
    hipEvent_t e0 = nullptr, e1 = nullptr, done = nullptr;
    hipEvent_t k2a = nullptr, k2b = nullptr, k3b = nullptr;   // cut rounds: around K2 and K3 of a round
    std::vector<int64_t> ids;
    std::vector<NodeRec> recs;  // the batch's node records, copied at pop time (one random access per node and step)
    std::vector<int32_t> slots;  // staging kept alive
    // branching parents by dive level (0: the batch, p: the p-th dive children): output position,
    // record row, variable, and the two child rows each
    struct Branchings { std::vector<int32_t> pos, slot, var, child; };
    std::vector<Branchings> br;
    std::vector<int32_t> dive_slots;  // record rows of the dive children (freed with the step)
    // cut rounds (mipx_tree_create_ex with cut parameters): per node of the batch the working cut
    // list, the row duals, the loop's state and the pool of candidate cuts (a slab of slab_rows rows)
    int32_t *w_ncut = nullptr, *w_ids = nullptr, *cs_state = nullptr, *cs_active = nullptr,
            *cs_resolve = nullptr, *cs_counters = nullptr, *k2_ncuts = nullptr, *k3_nadded = nullptr,
            *k3_added = nullptr, *k3_term = nullptr, *pool_list = nullptr, *dump_idx = nullptr,
            *cs_need_tab = nullptr;
    double *d_y = nullptr, *cs_before = nullptr, *slab_pi = nullptr, *slab_pi0 = nullptr,
           *dump_T = nullptr, *dump_vec = nullptr;
    int32_t *h_cs = nullptr;   // pinned: step_layout::CutState
    int dive = 0;  // this step was launched with the in-place dive: children in a row per node
    bool scored_once = false;  // K4 ran on this step (the first run's request counter was zeroed by K1)
    // the step finished on the device (finish_kernels.hip.h): the parents' records and the pool rows the
    // children may take go up with the batch, a summary + compact lists come back
    bool fast = false;
    int tabv = 0;                                // the table version this step's finish writes
    char *d_par = nullptr, *h_par = nullptr;     // step_layout::ParentBlock
    int32_t *c_info = nullptr, *c_cnt = nullptr, *c_eval = nullptr, *c_flag = nullptr;
    double *c_val = nullptr;
    mipx::FinishSummary *d_sum = nullptr;
    mipx::OpenEntry *d_open = nullptr;
    int32_t *d_dead = nullptr;
    mipx::PcSample *d_samples = nullptr, *h_samples = nullptr;   // h_samples: pinned staging of a host-finished step's samples
    int32_t *d_skeys = nullptr;                  // the samples' table entries, densely (pc_apply scans them)
    char *h_fin = nullptr;                       // pinned: step_layout::FinishBlock
    std::vector<int32_t> budget;
    // host spill: the batch's spilled nodes, staged pinned as [offsets (rl_n + 1) | rows | records] and unpacked
    // into their new rows on the launch stream before the node LPs read them
    char *h_rl = nullptr, *d_rl = nullptr;
    int rl_n = 0;
    // dual function (recording on): the node LPs' row duals, the record kernel's entries and its timing
    double *df_y = nullptr;
    char *df_h = nullptr, *df_d = nullptr;
    hipEvent_t df_e0 = nullptr, df_e1 = nullptr;
    bool df_timed = false;
    int heur_n = 0;   // primal heuristic: the points of this step it was launched on (0: none)
    int ls_n = 0;     // local search: the points of this step it was launched on behind the heuristic (0: none)
    int fp_n = 0;     // fix-and-propagate dive: the points of this step it was launched on behind the heuristic (0: none)
    int wr_n = 0;     // weighted row repair: the points of this step it was launched on behind the heuristic (0: none)
    int cube_n = 0;   // cube search: the points of this step it was launched on beside the heuristic (0: none)
    int comp_n = 0;   // completion: the points per block of this step it was launched on behind the heuristics (0: none)
    bool comp_cube = false;   // ... and whether the cube's block went with the heuristic's
    int lpdive_n = 0; // LP dive: the points of this step it was launched on (0: none)
    int prop_n = 0;   // bound propagation: the nodes of this step it was launched on (0: none)
    std::vector<int> rc_cnt;          // reduced-cost tightening: the parents it was launched on, per level, not yet
    hipStream_t rc_stream = nullptr;  // collected (empty: none), and the stream the launches went to
    int B = 0;
    bool in_flight = false;
    double inflight_min = std::numeric_limits<double>::infinity();   // lowest inherited bound of the batch (exchange record)
};

// Host spill (include/mipx_spill.h): open nodes moved out of the pool into compact records in pinned host
// memory.  One segment per spill event, freed once its last record is reloaded or dropped.
struct SpillSeg { char *host = nullptr; int64_t bytes = 0, live = 0; };
struct SpillLoc { int32_t seg; int32_t bytes; int64_t off; };
struct HostSpill {
    int64_t cap = 0;                 // max host bytes; 0: off
    hipStream_t st = nullptr;        // count / scan / pack and the copy down, beside the steps in flight
    double *d_root = nullptr;        // [root l | root u]
    int32_t *d_slot = nullptr;       // one event's scratch: the victims' rows, ids, record offsets, records
    int64_t *d_id = nullptr, *d_off = nullptr;
    char *d_rec = nullptr;
    size_t vict_cap = 0, rec_cap = 0, rl_cap = 0;
    std::vector<SpillSeg> segs;
    std::vector<int32_t> seg_free;
    std::vector<char *> dead;        // emptied segments, freed at the next event (hipHostFree waits for the device)
    std::vector<SpillLoc> loc;       // indexed by -2 - NodeRec::slot
    std::vector<int32_t> loc_free;
    int64_t bytes = 0, peak = 0, spilled = 0, reloaded = 0, on_host = 0, events = 0;
    double spill_us = 0.0, reload_us = 0.0;
};

// Dual function (include/mipx_dualfn.h): one record (y, t) per node solved to optimality, appended to a
// store in device memory; the infeasible nodes' bounds and basis codes beside it.  The per-node arrays
// exist only while recording is on (NodeRec keeps its size).
struct DualFn {
    bool on = false;
    int64_t cap = 0, bytes = 0;          // byte cap, bytes in use (records and infeasible rows)
    int rows = 0;                        // the LP's own rows (slacks of the penalised LP)
    std::vector<int32_t> pos;            // per engine row: its LP row, and the sign
    std::vector<double> sign;
    std::vector<int64_t> parent;         // per node id: parent id (-1 root)
    std::vector<int32_t> rec;            // per node id: its record (-1 none)
    std::vector<uint8_t> haschild;       // per node id
    std::vector<int64_t> rec_node;       // per record: node id
    std::vector<int32_t> rec_status;     // per record: 0 node LP, 1 penalised re-solve
    double *d_y = nullptr, *d_t = nullptr;   // the store: rows of m, and t
    int64_t rcap = 0;                    // rows allocated
    std::vector<int64_t> inf_node;       // infeasible nodes with saved rows, in order
    int64_t inf_done = 0;                // ... the first inf_done of them have been re-solved (or given up)
    double *d_il = nullptr, *d_iu = nullptr;  // their rows: n bounds each, nv codes
    int8_t *d_iv = nullptr;
    int64_t icap = 0;
    int64_t dropped = 0, resolves = 0, noterm = 0;
    double record_us = 0.0, eval_us = 0.0;
    // per step buffer: the node LPs' row duals (levels x max_batch x m), the entry lists (staged pinned)
    size_t ystep_rows = 0;
    // evaluation: the lineage arrays on the device, rebuilt when the records or the tree changed
    bool dirty = true;
    int32_t *d_prec = nullptr, *d_order = nullptr, *d_lvl = nullptr, *d_leaf = nullptr;
    int nlvl = 0, nleaf = 0, bare = 0;
    double *d_V = nullptr, *d_W = nullptr, *d_out = nullptr;
    size_t vcap = 0, wcap = 0, ocap = 0;
    std::vector<double> hostA;           // A (m x n), read back once for the penalised LP
};

#include "treerec.hip.h"

// Restart (include/mipx_restart.h): what a tree made by mipx_tree_create_restart knows of its making.
struct RestartRec {
    bool on = false;
    int64_t skeleton = 0;             // records copied from the source
    std::vector<int64_t> seeds;       // the source's childless records, ascending: the open nodes it started with
    int64_t bytes = 0;                // device bytes the seeding wrote
    double seed_us = 0.0;             // device time of restart_seed
};

// What stands behind a step option's packed block, per step buffer: the block on the device, its pinned mirror,
// optionally a block of points, and the event pair around the option's launches.  A plain struct that mipx_tree_destroy
// releases like everything else of the tree; the members are defined beside dmalloc and tree_d2h.  It knows nothing of
// an option's cap or on: the mipx_tree_set_* entries switch the option off, grow, and switch it on last.
namespace {
struct StepRing {
    char *d_out[3] = {nullptr, nullptr, nullptr}, *h_out[3] = {nullptr, nullptr, nullptr};
    double *d_x[3] = {nullptr, nullptr, nullptr};   // (stays null where the option has no points of its own)
    hipEvent_t e0[3] = {nullptr, nullptr, nullptr}, e1[3] = {nullptr, nullptr, nullptr};
    int grow(mipx_ctx *ctx, size_t out_bytes, size_t x_doubles);   // new blocks for all three buffers, or none at all
    void drop();      // the blocks (grow and release use it)
    void release();   // the blocks and the events
    int begin(mipx_ctx *ctx, int bi, hipStream_t st);   // e0 of buffer bi, in front of the option's launches on st
    int end(mipx_ctx *ctx, int bi, hipStream_t st);     // e1, behind them
    int fetch(mipx_tree *t, int bi, size_t bytes, double &us);   // the block to its mirror; the pair's time onto us
};
}  // namespace

// Primal heuristic (include/mipx_heur.h): the option's parameters, the root's bounds on the device, and per step
// buffer the rounded points and what comes down with each step (step_layout::HeurOut).
struct HeurState {
    bool on = false;
    int points = 0, every = 1, max_moves = 0;
    int cap = 0;                     // points the step buffers are laid out for
    double tol = 1e-9;
    double *d_lu = nullptr;          // [root l | root u]
    StepRing ring;                   // (with the rounded points)
    int64_t tried = 0, feasible = 0, stuck = 0, capped = 0, repair = 0, lift = 0, installed = 0;
    double us = 0.0;                 // device time of heur_round_repair
};

// Pair-move local search behind the heuristic (include/mipx_lsearch.h): the move cap and, per step buffer, what
// comes down with each step (step_layout::LsOut); the points and their objectives are the heuristic's, in place.
struct LsState {
    bool on = false;
    int max_moves = 0;
    int cap = 0;                     // points the step buffers are laid out for (the heuristic's cap)
    StepRing ring;
    int64_t run = 0, improved = 0, singles = 0, pairs = 0, capped = 0, installed = 0;
    double us = 0.0;                 // device time of ls_pair_search
};

// Fix-and-propagate dive behind the heuristic (include/mipx_fixprop.h): the caps and, per step buffer, what comes
// down with each step (step_layout::FpOut); the points are the heuristic's, in place.
struct FpState {
    bool on = false;
    int max_rounds = 0, max_tries = 0;
    int cap = 0;                     // points the step buffers are laid out for (the heuristic's cap)
    StepRing ring;
    int64_t tried = 0, feasible = 0, stuck = 0, capped = 0, fixings = 0, tries = 0, installed = 0;
    double us = 0.0;                 // device time of fixprop_dive and of the lift behind it
};

// Weighted row repair behind the heuristic (include/mipx_wrepair.h): the cap and, per step buffer, what comes down
// with each step (step_layout::WrOut); the points are the heuristic's, in place.  Never on together with the dive.
struct WrState {
    bool on = false;
    int max_steps = 0;
    int cap = 0;                     // points the step buffers are laid out for (the heuristic's cap)
    StepRing ring;
    int64_t tried = 0, feasible = 0, capped = 0, moves = 0, bumps = 0, installed = 0;
    double us = 0.0;                 // device time of wrepair_steps and of the lift behind it
};

// Cube search beside the heuristic (include/mipx_cube.h): the column cap, the launch's workspace (mipx::CubeWs; one,
// the launches are queued on one stream) and, per step buffer, the cube points -- a block of their own: the
// heuristic's slots may hold feasible points already -- and what comes down with each step (step_layout::CubeOut).
struct CubeState {
    bool on = false;
    int max_columns = 0;
    int cap = 0, ws_columns = 0;     // points the step buffers are laid out for (the heuristic's cap); K the workspace is for
    char *d_ws = nullptr;
    StepRing ring;                   // (with the option's points)
    int64_t tried = 0, found = 0, none = 0, columns = 0, at_cap = 0, installed = 0;
    double us = 0.0;                 // device time of the three kernels and of the lift behind them
};

// Completion over the continuous columns (include/mipx_complete.h): the tolerance, the launch's workspace
// (mipx::CompWs for 2 cap points; one, the launches are queued on one stream) and, per step buffer, the completed
// points -- a block of their own, the heuristic's cap points and then the cube's -- and what comes down with each step
// (step_layout::CompOut).
struct CompState {
    bool on = false;
    double ctol = 1e-6;
    int cap = 0;                     // points per block the step buffers are laid out for (the heuristic's cap)
    char *d_ws = nullptr;
    StepRing ring;                   // (with the option's points)
    int64_t tried = 0, completed = 0, infeasible = 0, failed = 0, rescued = 0, installed = 0, pivots = 0;
    double us = 0.0;                 // device time of the two kernels and the LP launch between them
};

// LP dive (include/mipx_lpdive.h): the caps, the lock counts of rule 1 (once per problem), the dive's workspace
// (mipx::LpdiveWs for cap points; one, the launches are queued on one stream) and, per step buffer, the dive's points
// and what comes down with each step (mipx::LpdiveOut).  Nothing of it lies in the packed step buffer.
struct LpdiveState {
    bool on = false;
    int max_rounds = 0, every = 0, rule = 0;
    int cap = 0;                     // points the buffers are laid out for (the heuristic's cap)
    int32_t *d_locks = nullptr;
    char *d_ws = nullptr;
    StepRing ring;                   // (with the option's points)
    int64_t tried = 0, feasible = 0, infeasible = 0, failed = 0, moves = 0, installed = 0, pivots = 0;
    double us = 0.0;                 // device time of the dive's kernels and the LP launches between them
};

// Objective step (include/mipx_objstep.h): the step and the counters.
struct ObjStepState {
    bool on = false;
    double step = 0.0;
    int64_t popped = 0, unbranched = 0, launches = 0;
};

// Bound propagation (include/mipx_prop.h): the option's parameters and, per step buffer, what comes down with
// each step (step_layout::PropOut).
struct PropState {
    bool on = false;
    int max_rounds = 0, use_cutoff = 1;
    int cap = 0;                     // nodes the step buffers are laid out for (the tree's max_batch)
    double tol = 1e-6;
    StepRing ring;
    int64_t nodes = 0, tightened = 0, infeasible = 0, changed = 0, rounds = 0, capped = 0;
    double us = 0.0;                 // device time of prop_bounds
};

// Reduced-cost tightening (include/mipx_rcfix.h): per step buffer the node LPs' row duals, the parents' lists going
// up and the results coming down (step_layout::RcOut), and an event pair per level.
constexpr int kRcLevels = 9;   // the batch and its plunge levels (1 + kMaxDive)
struct RcState {
    bool on = false;
    int cap = 0;                     // nodes per level the step buffers are laid out for (the tree's max_batch)
    double tol = 1e-6, dtol = 1e-9;
    double *d_y[3] = {nullptr, nullptr, nullptr};   // kRcLevels x cap x m
    int32_t *d_io[3] = {nullptr, nullptr, nullptr}, *h_io[3] = {nullptr, nullptr, nullptr};
    hipEvent_t e0[3][kRcLevels] = {}, e1[3][kRcLevels] = {};
    int64_t nodes = 0, tightened = 0, cut_off = 0, no_bound = 0, changed = 0, launches = 0;
    double us = 0.0;                 // device time of rc_tighten
};

struct mipx_tree {
    mipx_problem *prob = nullptr;
    mipx_ctx *ctx = nullptr;
    int n = 0, m = 0, n_int = 0;
    int rule = 0, search = 0, sb_iters = 5, max_batch = 1;
    int64_t capacity = 0;
    std::vector<int32_t> int_idx;
    // device pool + per-step buffers
    double *pool_l = nullptr, *pool_u = nullptr;
    int8_t *pool_v = nullptr;
    double *atab_T = nullptr, *atab_vec = nullptr;   // mipx_tree_reanchor: one anchor per re-anchored node
    int32_t *atab_idx = nullptr;
    int64_t atab_count = 0;
    int32_t *d_int_idx = nullptr, *d_pairs = nullptr, *d_pairs2 = nullptr;
    double *d_cost_l = nullptr, *d_cost_r = nullptr, *d_cost_l2 = nullptr, *d_cost_r2 = nullptr;
    uint8_t *d_has = nullptr, *d_has2 = nullptr;
    char *h_tab = nullptr;  // pinned mirror of [cost_l | cost_r | has_entry]: d_cost_l .. d_has are one allocation
    // the table block on the device: [cost_l | cost_r | has | pad | times_l | times_r | own sums (4 n)]; with the
    // device finish the device holds the table (every sample reaches it through pc_apply, in stream order) and
    // the host vectors are the snapshot read back with each step
    size_t tab_off2 = 0, tab_bytes = 0, tab_stride = 0;
    // Device finish: the table is a ring of kTabV versions.  Step k's finish (on stf, beside the node LPs of
    // step k + 1) copies the version at the tail and applies its samples to the copy; a launch reads the
    // version of the last step the HOST has finished -- complete by then, never written again while a
    // kernel in flight reads it, and the same version in every run.
    int tab_tail = 0, tab_host = 0;
    // Samples of a host-finished node / an exchange's merge are applied LATE, to the version at the tail of stf's
    // queue at that time: ev_tab[v] / tab_late[v] say that version v got such an update and when it is complete.
    // Only a launch that reads that very version waits for it (in the pipeline a launch reads an older one).
    hipEvent_t ev_tab[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    bool tab_late[8] = {false, false, false, false, false, false, false, false};
    double *h_delta = nullptr, *d_delta = nullptr;   // exchange: the other ranks' new samples (4 staging slots)
    int delta_turn = 0;
    std::vector<double> pc_others_prev;
    std::vector<double> pc_posted;  // own samples as last posted: per entry the (sum, times) with the highest times (x_fill_record)
    double *d_primal = nullptr;
    double primal_sent = std::numeric_limits<double>::infinity();   // what the device knows of the host's incumbent value
    bool fast_ok = false;           // steps are finished on the device where they file no probe request
    bool times_dirty = false;       // the host replaced the table: times go up with it
    size_t samples_cap = 0;
    std::vector<mipx::PcSample> pend_samples;   // a host-finished step's samples, on their way to the device table
    hipStream_t st2 = nullptr;  // strong-branching probes + re-scoring run beside the step in flight
    hipStream_t st3 = nullptr;  // children records of step k are written beside the node LPs of step k+1
    hipStream_t stf = nullptr;  // device finish: the finish kernels of step k and the table's version chain, beside the node LPs of step k+1
    hipEvent_t ev_child = nullptr;
    bool child_pending = false;
    bool cold_launch = false;       // the next launch_lp is the root's first solve (LpArgs::cold)
    int32_t *h_pairs = nullptr; // pinned staging of the branching lists
    char *h_pres = nullptr;     // pinned mirror of the probe results [pp_obj | pp_status]
    StepBuf buf[3];   // a ring: up to three steps in flight (mipx_tree_solve)
    bool table_dirty = false, pipeline = true;
    int dive = 0;           // mipx_tree_set_dive: dive children in a row per node (0: off)
    bool pool_exhausted = false;
    int64_t age_hist[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // popped nodes by age in steps (1 = created by the previous step)
    int64_t depth_sum = 0;
    int64_t dives = 0;      // dive children evaluated in place
    mipx_tree_hook hook = nullptr;
    void *hook_user = nullptr;
    int hook_every = 0;
    // probe pool (strong branching)
    int64_t probe_cap = 0;
    double *pp_l = nullptr, *pp_u = nullptr, *pp_obj = nullptr;
    int8_t *pp_v = nullptr;
    int32_t *pp_status = nullptr;
    // host state
    NodeTable nodes;
    std::vector<int32_t> free_slots;
    PyHeap heap;        // exact mode (max_batch == 1) and depth-first search
    BucketQueue bq;     // batched best-first search
    bool use_bq = false;
    std::vector<BucketQueue::Item> popped;
    std::vector<BucketQueue::Item> pend;   // a step's pushes, handed to the bucket queue in one go (tree_finish)
    std::priority_queue<std::pair<double, int64_t>, std::vector<std::pair<double, int64_t>>,
                        std::greater<std::pair<double, int64_t>>> open_bounds;  // lazy, for DFS
    std::vector<uint8_t> is_open;
    double closed_min = std::numeric_limits<double>::infinity();
    double primal = std::numeric_limits<double>::infinity();
    std::vector<double> best_x;
    bool have_x = false, unbounded = false, started = false;
    int status = 0;  // 0 unsolved, 1 optimal, 2 infeasible, 3 unbounded, 4 stopped
    int64_t evaluated = 0, lps = 0, probes = 0, pivots = 0, steps = 0, cut_resolves = 0;
    double solve_seconds = 0.0, kernel_ms = 0.0, k2_ms = 0.0, k3_ms = 0.0;
    std::vector<double> cost_l, cost_r;
    std::vector<int32_t> times_l, times_r;
    std::vector<uint8_t> has_entry;
    // trace of evaluated nodes: id, lp status, branch variable, objective
    std::vector<int64_t> tr_id;
    std::vector<int32_t> tr_status, tr_bidx;
    std::vector<double> tr_obj;
    std::vector<int32_t> tr_cuts;   // cut rounds: 8 per evaluated node (rounds, the six GMIC counters, cut rows it ends with)
    bool trace = false;
    bool anchor_mode = false, anchor_set = false;
    // multi-GPU exchange (mipx_tree_set_comm)
    mipx_comm *comm = nullptr;
    int x_every = 0;
    bool x_done = false;             // the ranks agreed to stop (set by an applied exchange)
    bool x_fatal = false;            // ... because a rank failed (reason 5)
    bool child_recorded = false;     // ev_child has been recorded at least once
    int fault_step = 0;              // MIPX_FAULT_STEP (tests): the step whose host half fails
    int x_stop_flag = 0;             // this rank hit one of its own limits (3: it failed)
    int64_t x_rounds = 0;            // exchanges applied
    int x_batch = 1;                 // frontier batch of the running solve (what "cannot fill a batch" means)
    double x_mip_gap = 0.0;
    std::vector<double> x_rec;       // this rank's record
    std::vector<double> pc_base, pc_own, pc_others;   // [sum_l | sum_r | times_l | times_r], n each
    int64_t ramp[4] = {0, 0, 0, 0};  // evaluated, lps, probes, pivots at sharding time (replicated ramp-up)
    int64_t g_counts[5] = {0, 0, 0, 0, 0};   // global evaluated, lps, probes, pivots, open
    double g_dual = -std::numeric_limits<double>::infinity();
    int g_inc_rank = -1;
    int64_t nodes_sent = 0, nodes_received = 0;
    // cut rounds
    bool cuts = false;
    mipx_cut_params cp{};
    int kc = 0;             // cut rows a node can carry
    int mrows = 0;          // rows allotted per node: m + kc (m without cut rounds)
    int slab_rows = 0;      // candidate cuts a node can hold while it is being bounded
    double *store_pi = nullptr, *store_pi0 = nullptr;   // the cut store (append-only)
    int32_t *store_count = nullptr;
    int64_t store_cap = 0;
    int32_t *pool_ncut = nullptr, *pool_ids = nullptr;  // node pool: the nodes' cut lists
    int32_t *pp_ncut = nullptr, *pp_ids = nullptr;      // probe pool
    uint8_t *d_is_int = nullptr;
    int64_t cut_totals[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // rounds, it/n created, it/n added, it/n removed, dropped
    double phase_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // MIPX_TREE_PROFILE=1: host-side breakdown
    std::vector<double> root_l, root_u;   // the root's bounds (compact records store the differences)
    HostSpill hs;
    DualFn df;
    TreeRec tr;
    RestartRec rs;
    HeurState hr;
    LsState ls;
    FpState fp;
    WrState wr;
    CubeState cu;
    CompState cc;
    LpdiveState ld;
    ObjStepState os;
    PropState pg;
    RcState rc;
    // cut migration (mipx_tree_set_cut_migration): the top cm_rows rows of the cut store take the cut rows
    // of nodes received from other ranks, filled in order by the migration code (host-side fill level)
    int64_t cm_rows = 0, cm_used = 0;
    int64_t cm_nodes_sent = 0, cm_rows_sent = 0, cm_rows_received = 0;
    double probe_ms[4] = {0, 0, 0, 0};  // probes phase: requests | enqueue | wait | results
};

namespace {

template <typename T>
int dmalloc(mipx_ctx *ctx, T **p, size_t count) {
    HIP_TRY(ctx, hipMalloc((void **)p, (count ? count : 1) * sizeof(T)));
    return MIPX_OK;
}

// The blocks of every buffer, null-safe; the events stay.
void StepRing::drop() {
    for (int k = 0; k < 3; k++) {
        if (d_x[k]) (void)hipFree(d_x[k]);
        if (d_out[k]) (void)hipFree(d_out[k]);
        if (h_out[k]) (void)hipHostFree(h_out[k]);
        d_x[k] = nullptr; d_out[k] = nullptr; h_out[k] = nullptr;
    }
}

// The old blocks go first, then all three buffers are made anew (out_bytes each on the device and pinned, x_doubles
// doubles of points where that is not 0) with the events that are not there yet.  A failure frees what was made: the
// ring then holds no block at all, and the caller's option is off with nothing to launch on.
int StepRing::grow(mipx_ctx *ctx, size_t out_bytes, size_t x_doubles) {
    const auto make = [&](int k) -> int {
        int rc = x_doubles ? dmalloc(ctx, &d_x[k], x_doubles) : MIPX_OK;
        if (rc == MIPX_OK) rc = dmalloc(ctx, &d_out[k], out_bytes);
        if (rc) return rc;
        HIP_TRY(ctx, hipHostMalloc((void **)&h_out[k], out_bytes));
        if (!e0[k]) HIP_TRY(ctx, hipEventCreate(&e0[k]));
        if (!e1[k]) HIP_TRY(ctx, hipEventCreate(&e1[k]));
        return MIPX_OK;
    };
    drop();
    int rc = MIPX_OK;
    for (int k = 0; k < 3 && rc == MIPX_OK; k++) rc = make(k);
    if (rc) drop();
    return rc;
}

void StepRing::release() {
    drop();
    for (int k = 0; k < 3; k++) {
        if (e0[k]) (void)hipEventDestroy(e0[k]);
        if (e1[k]) (void)hipEventDestroy(e1[k]);
        e0[k] = nullptr; e1[k] = nullptr;
    }
}

int StepRing::begin(mipx_ctx *ctx, int bi, hipStream_t st) {
    HIP_TRY(ctx, hipEventRecord(e0[bi], st));
    return MIPX_OK;
}

int StepRing::end(mipx_ctx *ctx, int bi, hipStream_t st) {
    HIP_TRY(ctx, hipEventRecord(e1[bi], st));
    return MIPX_OK;
}

double tree_open_min(mipx_tree *t) {
    const double inf = std::numeric_limits<double>::infinity();
    if (t->use_bq) return t->bq.empty() ? inf : t->bq.min_key();
    if (t->search == 0) return t->heap.empty() ? inf : t->heap.h[0].key;
    while (!t->open_bounds.empty() && !t->is_open[t->open_bounds.top().second]) t->open_bounds.pop();
    return t->open_bounds.empty() ? inf : t->open_bounds.top().first;
}

// What a node's bound is compared with to decide whether the node goes on, and what the kernels get as their
// cutoff: the incumbent's value, or with an objective step (include/mipx_objstep.h) the value one step below it plus
// a slack where that is lower.  +inf without an incumbent.
double tree_cutoff(const mipx_tree *t) {
    const double U = t->primal;
    if (!t->os.on || !std::isfinite(U)) return U;
    const double C = U - t->os.step + 1e-6 * std::fmax(1.0, std::fabs(U));
    return C < U ? C : U;
}

double tree_dual_bound(mipx_tree *t) { return std::fmin(tree_open_min(t), t->closed_min); }   // (of this rank's shard)

// reference current_gap (branch_and_bound.py:203-213); -1 encodes None
double tree_gap(mipx_tree *t) {
    const double inf = std::numeric_limits<double>::infinity();
    const double p = t->primal;
    if (p == inf) return -1.0;  // (before the dual bound: that one scans a bucket of the open list)
    const double d = t->comm ? t->g_dual : tree_dual_bound(t);   // (sharded: the ranks' MIN, as of the last exchange)
    if (p == 0 && d == 0) return 0.0;
    if (p == 0) return inf;
    return std::fabs(p - d) / std::fabs(p);
}

bool tree_queue_empty(const mipx_tree *t) { return t->use_bq ? t->bq.empty() : t->heap.empty(); }

// open nodes in queue order (heap array order / bucket order)
void tree_queue_ids(const mipx_tree *t, std::vector<int64_t> &out) {
    if (t->use_bq) {
        std::vector<BucketQueue::Item> items;
        t->bq.items(items);
        for (const auto &it : items) out.push_back(it.id);
    } else {
        for (const auto &it : t->heap.h) out.push_back(it.id);
    }
}

#ifdef MIPX_HOSTPROF
#include <x86intrin.h>
static unsigned long long g_hp_push = 0, g_hp_rec = 0, g_hp_n = 0;
#endif
void tree_push(mipx_tree *t, int64_t id) {
#ifdef MIPX_HOSTPROF
    const unsigned long long t0_ = __rdtsc();
    struct Acc { unsigned long long t0; ~Acc() { g_hp_push += __rdtsc() - t0; g_hp_n++; } } acc_{t0_};
#endif
    if (t->use_bq) t->bq.push(t->nodes[id].key, id);
    else t->heap.push(t->nodes[id].key, id);
    if (t->search != 0) {  // depth first: the dual bound comes from a lazy heap over the open nodes
        if ((size_t)id >= t->is_open.size()) t->is_open.resize(id + 1, 0);
        t->is_open[id] = 1;
        t->open_bounds.push({t->nodes[id].dual_bound, id});
    }
}

constexpr int kTabV = 8;   // table versions (device finish): one per step in flight and a few to spare
struct TabPtr { double *cl, *cr; uint8_t *has; int32_t *times; double *own; };
TabPtr tab_at(const mipx_tree *t, int v) {
    char *base = (char *)t->d_cost_l + (size_t)v * t->tab_stride;
    const size_t n = (size_t)t->n;
    TabPtr p;
    p.cl = (double *)base; p.cr = (double *)(base + 8 * n); p.has = (uint8_t *)(base + 16 * n);
    p.times = (int32_t *)(base + t->tab_off2); p.own = (double *)(base + t->tab_off2 + 8 * n);
    return p;
}

// what a launch over nodes with cut rows adds to launch_lp (cut rounds only)
struct CutLaunch {
    const int32_t *ncut = nullptr, *ids = nullptr;   // the nodes' cut lists, by batch position
    int vstat_by_node = 0;                           // the warm-start bases are dense too (l, u through slot)
    const int32_t *active = nullptr;                 // skip mask
    double *y = nullptr;                             // row duals out (batch x mrows)
    int m_rows = -1;                                 // largest row count in the launch (tile choice)
    double *dT = nullptr, *dvec = nullptr;           // dump every node's final tableau (K2's input)
    int32_t *didx = nullptr;
    bool no_anchor = false;
};

int launch_lp(mipx_tree *t, int batch, const double *l, const double *u, const int8_t *v,
              const int32_t *slot, int max_iter, int32_t *status, double *obj, double *x,
              int8_t *vout, int32_t *iters, int32_t *npiv, hipStream_t stream = nullptr,
              const StepBuf *dive = nullptr, const int32_t *asel = nullptr, const CutLaunch *cl = nullptr,
              double *y_out = nullptr) {
    mipx::LpArgs a = problem_args(t->prob, !(cl != nullptr && cl->no_anchor));
    if (dive) {  // in-place dive: K4's rule inside K1, level p's children at positions p * batch ..
        a.dive = dive->dive; a.dive_off = batch; a.rule = t->rule; a.n_int = t->n_int;
        const TabPtr tb = tab_at(t, t->fast_ok ? t->tab_host : 0);
        a.int_idx = t->d_int_idx; a.cost_l = tb.cl; a.cost_r = tb.cr; a.has_entry = tb.has;
        a.dive_cutoff = tree_cutoff(t);
        a.dive_var = dive->d.dvar; a.dive_dir = dive->d.ddir; a.dive_val = dive->d.dval;
        a.dive_preset = 1;           // the kernel itself marks "no child / no dive" first
        a.zero16 = dive->d.ask_count; // and zeroes K4's request counter
    }
    a.l = l; a.u = u; a.vstat_in = v; a.slot = slot; a.max_iter = max_iter;
    a.cold = t->cold_launch ? 1 : 0;   // (the root's step: its pool row holds no basis)
    t->cold_launch = false;
    if (asel != nullptr && t->atab_T != nullptr) {  // node LPs: the anchor their record names
        a.anchor_sel = asel; a.atab_T = t->atab_T; a.atab_vec = t->atab_vec; a.atab_idx = t->atab_idx;
    }
    a.status = status; a.obj = obj; a.x = x; a.vstat_out = vout;
    a.iters = iters; a.npivots = npiv; a.batch = batch;
    int m_rows = -1;
    if (cl != nullptr) {
        a.ncut = cl->ncut; a.cut_ids = cl->ids; a.cut_stride = t->kc;
        a.cut_pi = t->store_pi; a.cut_pi0 = t->store_pi0;
        a.mstride = t->mrows; a.vstat_by_node = cl->vstat_by_node; a.active = cl->active;
        a.y = cl->y;
        if (cl->dT) { a.dbg_T = cl->dT; a.dbg_vec = cl->dvec; a.dbg_idx = cl->didx; a.dbg_all = 1; }
        m_rows = cl->m_rows;
    }
    if (y_out) a.y = y_out;   // row duals of every output position (dual function recording)
    return launch_lp_any(t->prob, a, batch, stream, m_rows);
}

#include "dualfn.hip.h"

// Device -> host copies of the step loop go through the side stream, never the null stream: a
// null-stream copy shares a hardware queue with whatever the runtime mapped there, and in a
// process that also ran an ML framework's streams and RCCL that was the main stream with a 2 ms node-LP launch queued
// (measured: ~1 ms per synchronous hipMemcpy, 18 ms per 20 steps).
int tree_d2h(mipx_tree *t, void *dst, const void *src, size_t bytes) {
    HIP_TRY(t->ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, t->st2));
    HIP_TRY(t->ctx, hipStreamSynchronize(t->st2));
    return MIPX_OK;
}

int StepRing::fetch(mipx_tree *t, int bi, size_t bytes, double &us) {
    const int rc = tree_d2h(t, h_out[bi], d_out[bi], bytes);
    if (rc) return rc;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e0[bi], e1[bi]) == hipSuccess) us += 1000.0 * ms;
    return MIPX_OK;
}

// ---- primal heuristic (include/mipx_heur.h) ---------------------------------------------------------------
// One launch of heur_round_repair over `batch` points in device memory, queued on `st`.
int heur_launch(const mipx_problem *p, hipStream_t st, int batch, const double *d_x, const double *d_l, const double *d_u,
                const int32_t *d_int_idx, int n_int, double tol, int max_moves, const uint8_t *d_skip,
                const int32_t *d_lp_status, double *d_x_out, double *d_obj, int32_t *d_status, int32_t *d_moves) {
    mipx_ctx *ctx = p->ctx;
    if (p->m > mipx::kHeurMax || p->n > mipx::kHeurMax) return fail(ctx, MIPX_ETOOBIG, "primal heuristic: more than 1024 rows or columns");
    if (batch <= 0) return MIPX_OK;
    mipx::HeurArgs a;
    a.m = p->m; a.n = p->n; a.n_int = n_int; a.max_moves = max_moves; a.tol = tol;
    a.A = p->dA; a.b = p->db; a.c = p->dc; a.l = d_l; a.u = d_u; a.int_idx = d_int_idx;
    a.x = d_x; a.lp_status = d_lp_status; a.skip = d_skip;
    a.x_out = d_x_out; a.obj_out = d_obj; a.status_out = d_status; a.moves_out = d_moves;
    hipLaunchKernelGGL(mipx::heur_round_repair, dim3((unsigned)batch), dim3(mipx::kHeurNT), 0, st, a);
    HIP_TRY(ctx, hipGetLastError());
    return MIPX_OK;
}

// One launch of ls_pair_search over `batch` points in device memory, queued on `st` (d_gate: null, or per point the
// status of the heuristic that made it -- a point whose entry is not 0 is skipped and left as it is; d_x_out may be d_x).
int ls_launch(const mipx_problem *p, hipStream_t st, int batch, const double *d_x, const double *d_l, const double *d_u,
              const int32_t *d_int_idx, int n_int, double tol, int max_moves, const uint8_t *d_skip, const int32_t *d_gate,
              double *d_x_out, double *d_obj, int32_t *d_status, int32_t *d_moves) {
    mipx_ctx *ctx = p->ctx;
    if (p->m > mipx::kLsMax || p->n > mipx::kLsMax) return fail(ctx, MIPX_ETOOBIG, "local search: more than 1024 rows or columns");
    if (batch <= 0) return MIPX_OK;
    mipx::LsArgs a;
    a.m = p->m; a.n = p->n; a.n_int = n_int; a.max_moves = max_moves; a.tol = tol;
    a.A = p->dA; a.b = p->db; a.c = p->dc; a.l = d_l; a.u = d_u; a.int_idx = d_int_idx;
    a.x = d_x; a.skip = d_skip; a.gate = d_gate;
    a.x_out = d_x_out; a.obj_out = d_obj; a.status_out = d_status; a.moves_out = d_moves;
    hipLaunchKernelGGL(mipx::ls_pair_search, dim3((unsigned)batch), dim3(mipx::kLsNT), 0, st, a);
    HIP_TRY(ctx, hipGetLastError());
    return MIPX_OK;
}

// One launch of fixprop_dive over `batch` points in device memory, queued on `st` (d_gate: null, or per point the
// status of the heuristic that tried it first -- only its stuck and capped points are run, the others are left as
// they are; d_x_out may be d_x).
int fp_launch(const mipx_problem *p, hipStream_t st, int batch, const double *d_x, const double *d_l, const double *d_u,
              const int32_t *d_int_idx, int n_int, double cutoff, double tol, int max_rounds, int max_tries, const uint8_t *d_skip,
              const int32_t *d_gate, double *d_x_out, double *d_obj, int32_t *d_status, int32_t *d_counts) {
    mipx_ctx *ctx = p->ctx;
    if (p->m > mipx::kFpMax || p->n > mipx::kFpMax) return fail(ctx, MIPX_ETOOBIG, "fix-and-propagate dive: more than 1024 rows or columns");
    if (batch <= 0) return MIPX_OK;
    mipx::FixpropArgs a;
    a.m = p->m; a.n = p->n; a.n_int = n_int; a.max_rounds = max_rounds; a.max_tries = max_tries;
    a.cut = std::isfinite(cutoff) ? 1 : 0; a.tol = tol; a.cutoff = cutoff;
    a.A = p->dA; a.b = p->db; a.c = p->dc; a.l = d_l; a.u = d_u; a.int_idx = d_int_idx;
    a.x = d_x; a.skip = d_skip; a.gate = d_gate;
    a.x_out = d_x_out; a.obj_out = d_obj; a.status_out = d_status; a.counts_out = d_counts;
    hipLaunchKernelGGL(mipx::fixprop_dive, dim3((unsigned)batch), dim3(mipx::kFpNT), 0, st, a);
    HIP_TRY(ctx, hipGetLastError());
    return MIPX_OK;
}

// One launch of wrepair_steps over `batch` points in device memory, queued on `st` (d_gate: null, or per point the
// status of the heuristic that tried it first -- only its stuck and capped points are run; keep_gated: d_x_out holds
// that heuristic's points, and the others are left as they are).
int wr_launch(const mipx_problem *p, hipStream_t st, int batch, const double *d_x, const double *d_l, const double *d_u,
              const int32_t *d_int_idx, int n_int, double tol, int max_steps, const uint8_t *d_skip, const int32_t *d_gate,
              bool keep_gated, double *d_x_out, double *d_obj, int32_t *d_status, int32_t *d_counts) {
    mipx_ctx *ctx = p->ctx;
    if (p->m > mipx::kWrMax || p->n > mipx::kWrMax) return fail(ctx, MIPX_ETOOBIG, "weighted row repair: more than 1024 rows or columns");
    if (batch <= 0) return MIPX_OK;
    mipx::WrepairArgs a;
    a.m = p->m; a.n = p->n; a.n_int = n_int; a.max_steps = max_steps; a.keep_gated = keep_gated ? 1 : 0; a.tol = tol;
    a.A = p->dA; a.b = p->db; a.c = p->dc; a.l = d_l; a.u = d_u; a.int_idx = d_int_idx;
    a.x = d_x; a.skip = d_skip; a.gate = d_gate;
    a.x_out = d_x_out; a.obj_out = d_obj; a.status_out = d_status; a.counts_out = d_counts;
    hipLaunchKernelGGL(mipx::wrepair_steps, dim3((unsigned)batch), dim3(mipx::kWrNT), 0, st, a);
    HIP_TRY(ctx, hipGetLastError());
    return MIPX_OK;
}

// One run of the cube search over `batch` points in device memory, queued on `st`: cube_prepare, cube_enumerate and
// cube_pick, one behind the other (d_ws: a block of mipx::CubeWs(batch, m, max_columns).bytes() at least; d_lp_status:
// null, or per point the status of its node LP -- a point whose entry is not 0 is skipped; d_x_out is not d_x).
int cube_launch(const mipx_problem *p, hipStream_t st, int batch, const double *d_x, const double *d_l, const double *d_u,
                const int32_t *d_int_idx, int n_int, double cutoff, double tol, double ftol, int max_columns,
                const uint8_t *d_skip, const int32_t *d_lp_status, char *d_ws, double *d_x_out, double *d_obj,
                int32_t *d_status, int32_t *d_counts) {
    mipx_ctx *ctx = p->ctx;
    if (p->m > mipx::kCubeMax || p->n > mipx::kCubeMax) return fail(ctx, MIPX_ETOOBIG, "cube search: more than 1024 rows or columns");
    if (max_columns < 1 || max_columns > mipx::kCubeMaxK) return fail(ctx, MIPX_EINVAL, "cube search: max_columns outside 1..20");
    if (batch <= 0) return MIPX_OK;
    const mipx::CubeWs w((size_t)batch, (size_t)p->m, max_columns);
    mipx::CubeArgs a;
    a.m = p->m; a.n = p->n; a.n_int = n_int; a.K = max_columns; a.nchunks = mipx::cube_chunks(max_columns); a.p0 = 0;
    a.tol = tol; a.ftol = ftol; a.cutoff = cutoff;
    a.A = p->dA; a.b = p->db; a.c = p->dc; a.l = d_l; a.u = d_u; a.int_idx = d_int_idx;
    a.x = d_x; a.skip = d_skip; a.lp_status = d_lp_status;
    a.ws_s = (double *)(d_ws + w.s); a.ws_obj0 = (double *)(d_ws + w.obj0); a.ws_pobj = (double *)(d_ws + w.pobj);
    a.ws_kf = (int32_t *)(d_ws + w.kf); a.ws_pcode = (int32_t *)(d_ws + w.pcode);
    a.x_out = d_x_out; a.obj_out = d_obj; a.status_out = d_status; a.counts_out = d_counts;
    hipLaunchKernelGGL(mipx::cube_prepare, dim3((unsigned)batch), dim3(mipx::kCubeNT), 0, st, a);
    for (a.p0 = 0; a.p0 < batch; a.p0 += mipx::kCubeGridY)   // (the points lie in the grid's y, which ends at 65535)
        hipLaunchKernelGGL(mipx::cube_enumerate, dim3((unsigned)a.nchunks, (unsigned)std::min(batch - a.p0, mipx::kCubeGridY)),
                           dim3(mipx::kCubeNT), 0, st, a);
    a.p0 = 0;
    hipLaunchKernelGGL(mipx::cube_pick, dim3((unsigned)batch), dim3(mipx::kCubeNT), 0, st, a);
    HIP_TRY(ctx, hipGetLastError());
    return MIPX_OK;
}

// One block of points of a completion launch: `count` points in device memory, with their optional skip bytes, gate
// (a heuristic's status per point: 3 is skipped, and with gate_strict everything but 0) and basis codes (n + m per
// point), all indexed from the block's start.
struct CompSrc {
    const double *x;
    const uint8_t *skip;
    const int32_t *gate;
    bool gate_strict;
    const int8_t *vstat;
    int count;
};

// One completion (include/mipx_complete.h) of the points of `nsrc` blocks, queued on `st`: complete_prepare per block,
// ONE node-LP launch over all of them, complete_finish.  The outputs are indexed by position: the blocks behind one
// another (d_ws: mipx::CompWs(total, m, n).bytes() at least; d_x_out is none of the blocks).  The LP launch always
// carries basis codes (all 0 where a block has none: a cold start), so it never takes launch_root_coop's path, which
// would have the host wait; the problem's anchor is not used.
int comp_launch(mipx_problem *p, hipStream_t st, const CompSrc *src, int nsrc, const double *d_l, const double *d_u,
                const int32_t *d_int_idx, int n_int, double ctol, char *d_ws, double *d_x_out, double *d_obj,
                int32_t *d_status, int32_t *d_pivots) {
    mipx_ctx *ctx = p->ctx;
    if (p->m > mipx::kCompMax || p->n > mipx::kCompMax) return fail(ctx, MIPX_ETOOBIG, "completion: more than 1024 rows or columns");
    int total = 0;
    for (int k = 0; k < nsrc; k++) total += src[k].count > 0 ? src[k].count : 0;
    if (total <= 0) return MIPX_OK;
    const mipx::CompWs w((size_t)total, (size_t)p->m, (size_t)p->n);
    mipx::CompArgs a;
    a.m = p->m; a.n = p->n; a.n_int = n_int; a.p0 = 0; a.ctol = ctol;
    a.A = p->dA; a.b = p->db; a.c = p->dc; a.l = d_l; a.u = d_u; a.int_idx = d_int_idx;
    a.x = nullptr; a.skip = nullptr; a.gate = nullptr; a.gate_strict = 0; a.vstat = nullptr;
    a.ws_L = (double *)(d_ws + w.L); a.ws_U = (double *)(d_ws + w.U); a.ws_x = (const double *)(d_ws + w.x);
    a.ws_skipped = (int32_t *)(d_ws + w.skipped); a.ws_lp_status = (const int32_t *)(d_ws + w.lp_status);
    a.ws_pivots = (const int32_t *)(d_ws + w.pivots); a.ws_vstat = (int8_t *)(d_ws + w.vstat);
    a.x_out = d_x_out; a.obj_out = d_obj; a.status_out = d_status; a.pivots_out = d_pivots;
    for (int k = 0; k < nsrc; k++) {
        if (src[k].count <= 0) continue;
        a.x = src[k].x; a.skip = src[k].skip; a.gate = src[k].gate; a.gate_strict = src[k].gate_strict ? 1 : 0; a.vstat = src[k].vstat;
        hipLaunchKernelGGL(mipx::complete_prepare, dim3((unsigned)src[k].count), dim3(mipx::kCompNT), 0, st, a);
        a.p0 += src[k].count;
    }
    HIP_TRY(ctx, hipGetLastError());
    mipx::LpArgs g = problem_args(p, false);
    g.l = a.ws_L; g.u = a.ws_U; g.vstat_in = a.ws_vstat; g.max_iter = 0;
    g.status = (int32_t *)(d_ws + w.lp_status); g.x = (double *)(d_ws + w.x); g.npivots = (int32_t *)(d_ws + w.pivots);
    g.batch = total;
    const int rc = launch_lp_any(p, g, total, st);
    if (rc) return rc;
    a.p0 = 0;
    hipLaunchKernelGGL(mipx::complete_finish, dim3((unsigned)total), dim3(mipx::kCompNT), 0, st, a);
    HIP_TRY(ctx, hipGetLastError());
    return MIPX_OK;
}

// One LP dive (include/mipx_lpdive.h) of `batch` points in device memory, queued on `st`: lpdive_prepare, then per
// round lpdive_step and ONE node-LP launch over all the points, the last lpdive_step and lpdive_finish (d_ws:
// mipx::LpdiveWs(batch, m, n).bytes() at least; d_locks: lpdive_locks' counts; d_slot: null, or per point the row of
// d_l0 / d_u0 its box lies in; d_gate: null, or per point the status of its node LP -- a point whose entry is not 0 is
// skipped; d_x_out is not d_x0).  Every LP launch carries basis codes, as the completion's does.  With `poll` the host
// reads the round's counter of live points behind every step and stops launching at 0 (the batch entry; the outputs
// do not depend on it); without, nothing is read.
int lpdive_launch(mipx_problem *p, hipStream_t st, int batch, const double *d_x0, const double *d_l0, const double *d_u0,
                  const int32_t *d_slot, const uint8_t *d_skip, const int32_t *d_gate, const int8_t *d_vstat,
                  const int32_t *d_int_idx, int n_int, const int32_t *d_locks, double cutoff, int max_rounds, int rule,
                  bool poll, char *d_ws, double *d_x_out, double *d_obj, int32_t *d_status, int32_t *d_rounds,
                  int32_t *d_fixings, int32_t *d_flips, int32_t *d_pivots) {
    mipx_ctx *ctx = p->ctx;
    if (p->m > mipx::kLpdiveMax || p->n > mipx::kLpdiveMax) return fail(ctx, MIPX_ETOOBIG, "LP dive: more than 1024 rows or columns");
    if (max_rounds < 1 || max_rounds > mipx::kLpdiveMaxRounds) return fail(ctx, MIPX_EINVAL, "LP dive: max_rounds outside 1..1024");
    if (batch <= 0) return MIPX_OK;
    const mipx::LpdiveWs w((size_t)batch, (size_t)p->m, (size_t)p->n);
    mipx::LpdiveArgs a;
    a.m = p->m; a.n = p->n; a.n_int = n_int; a.rule = rule; a.round = 0; a.max_rounds = max_rounds;
    a.cutoff = cutoff; a.ftol = 1e-6; a.ctol = 1e-6;
    a.A = p->dA; a.b = p->db; a.c = p->dc; a.int_idx = d_int_idx; a.locks = d_locks;
    a.x0 = d_x0; a.l0 = d_l0; a.u0 = d_u0; a.slot = d_slot; a.skip = d_skip; a.gate = d_gate; a.vstat = d_vstat;
    a.ws_L = (double *)(d_ws + w.L); a.ws_U = (double *)(d_ws + w.U); a.ws_x = (double *)(d_ws + w.x);
    a.ws_vin = (int8_t *)(d_ws + w.vin); a.ws_vout = (const int8_t *)(d_ws + w.vout);
    a.ws_lp_obj = (const double *)(d_ws + w.lp_obj); a.ws_lp_status = (const int32_t *)(d_ws + w.lp_status);
    a.ws_lp_pivots = (const int32_t *)(d_ws + w.lp_pivots); a.ws_rec = (double *)(d_ws + w.rec);
    a.ws_rec_j = (int32_t *)(d_ws + w.rec_j); a.ws_phase = (int32_t *)(d_ws + w.phase); a.ws_live = (int32_t *)(d_ws + w.live);
    a.x_out = d_x_out; a.obj_out = d_obj; a.status_out = d_status; a.rounds_out = d_rounds; a.fixings_out = d_fixings;
    a.flips_out = d_flips; a.pivots_out = d_pivots;
    HIP_TRY(ctx, hipMemsetAsync(a.ws_live, 0, 4 * (size_t)(mipx::kLpdiveMaxRounds + 2), st));
    hipLaunchKernelGGL(mipx::lpdive_prepare, dim3((unsigned)batch), dim3(mipx::kLpdiveNT), 0, st, a);
    HIP_TRY(ctx, hipGetLastError());
    mipx::LpArgs g = problem_args(p, false);
    g.l = a.ws_L; g.u = a.ws_U; g.vstat_in = a.ws_vin; g.max_iter = 0;
    g.status = (int32_t *)(d_ws + w.lp_status); g.obj = (double *)(d_ws + w.lp_obj); g.x = a.ws_x;
    g.vstat_out = (int8_t *)(d_ws + w.vout); g.npivots = (int32_t *)(d_ws + w.lp_pivots);
    g.batch = batch;
    for (a.round = 1; a.round <= max_rounds + 1; a.round++) {
        hipLaunchKernelGGL(mipx::lpdive_step, dim3((unsigned)batch), dim3(mipx::kLpdiveWave), 0, st, a);
        HIP_TRY(ctx, hipGetLastError());
        if (a.round > max_rounds) break;
        if (poll) {
            int32_t live = 0;
            HIP_TRY(ctx, hipMemcpyAsync(&live, a.ws_live + a.round, 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(ctx, hipStreamSynchronize(st));
            if (live == 0) break;   // (no point goes into this round's LP: every later step would return at once)
        }
        mipx::LpArgs h = g;
        const int rc = launch_lp_any(p, h, batch, st);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(mipx::lpdive_finish, dim3((unsigned)batch), dim3(mipx::kLpdiveNT), 0, st, a);
    HIP_TRY(ctx, hipGetLastError());
    return MIPX_OK;
}

// The step's node LP solutions (level 0, the first positions) through the heuristic, behind its node LPs; the points
// it did not end feasible on through the fix-and-propagate dive, whose feasible points take their place and go through
// the heuristic once more (the lift), or through the weighted row repair in the same way (one of the two at most); and
// the feasible points of both through the local search, in place.  With the cube search the same LP points go through
// it as well, whatever the rounding made of them: its points lie in a block of their own, are lifted by the heuristic
// there and go through the local search there.
int heur_step_launch(mipx_tree *t, StepBuf &S) {
    HeurState &hr = t->hr;
    S.heur_n = 0;
    if (!hr.on || t->steps % hr.every != 0) return MIPX_OK;
    mipx_ctx *ctx = t->ctx;
    hipStream_t st = ctx->stream;
    const int bi = (int)(&S - t->buf), P = std::min(S.B, hr.points);
    const auto o = step_layout::HeurOut((size_t)hr.cap).view(hr.ring.d_out[bi]);
    if (int e = hr.ring.begin(ctx, bi, st)) return e;
    const int rc = heur_launch(t->prob, st, P, S.d_x, hr.d_lu, hr.d_lu + t->n, t->d_int_idx, t->n_int, hr.tol, hr.max_moves,
                               nullptr, S.d.status, hr.ring.d_x[bi], o.obj, o.status, o.moves);
    if (rc) return rc;
    if (int e = hr.ring.end(ctx, bi, st)) return e;
    S.heur_n = P;
    S.ls_n = 0;
    S.fp_n = 0;
    FpState &fp = t->fp;
    const auto fo = step_layout::FpOut((size_t)(fp.on ? fp.cap : 0)).view(fp.on ? fp.ring.d_out[bi] : nullptr);
    if (fp.on) {
        // the same LP points, gated by the heuristic's status; a dive point lands in the heuristic's slot of hr.d_x, its
        // objective and the lifted one in the dive's own block (a point the lift skips has its objective there zeroed)
        if (int e = fp.ring.begin(ctx, bi, st)) return e;
        int frc = fp_launch(t->prob, st, P, S.d_x, hr.d_lu, hr.d_lu + t->n, t->d_int_idx, t->n_int, tree_cutoff(t), hr.tol,
                            fp.max_rounds, fp.max_tries, nullptr, o.status, hr.ring.d_x[bi], fo.obj, fo.status, fo.counts);
        if (frc) return frc;
        frc = heur_launch(t->prob, st, P, hr.ring.d_x[bi], hr.d_lu, hr.d_lu + t->n, t->d_int_idx, t->n_int, hr.tol, hr.max_moves,
                          nullptr, fo.status, hr.ring.d_x[bi], fo.obj, fo.lift_status, fo.lift_moves);
        if (frc) return frc;
        if (int e = fp.ring.end(ctx, bi, st)) return e;
        S.fp_n = P;
    }
    S.wr_n = 0;
    WrState &wr = t->wr;
    const auto wo = step_layout::WrOut((size_t)(wr.on ? wr.cap : 0)).view(wr.on ? wr.ring.d_out[bi] : nullptr);
    if (wr.on) {
        // the dive's place, to the letter: the same LP points, gated by the heuristic's status; a repaired point lands in
        // the heuristic's slot of hr.d_x, its objective and the lifted one in this option's own block
        if (int e = wr.ring.begin(ctx, bi, st)) return e;
        int wrc = wr_launch(t->prob, st, P, S.d_x, hr.d_lu, hr.d_lu + t->n, t->d_int_idx, t->n_int, hr.tol, wr.max_steps,
                            nullptr, o.status, true, hr.ring.d_x[bi], wo.obj, wo.status, wo.counts);
        if (wrc) return wrc;
        wrc = heur_launch(t->prob, st, P, hr.ring.d_x[bi], hr.d_lu, hr.d_lu + t->n, t->d_int_idx, t->n_int, hr.tol, hr.max_moves,
                          nullptr, wo.status, hr.ring.d_x[bi], wo.obj, wo.lift_status, wo.lift_moves);
        if (wrc) return wrc;
        if (int e = wr.ring.end(ctx, bi, st)) return e;
        S.wr_n = P;
    }
    S.cube_n = 0;
    CubeState &cu = t->cu;
    const auto co = step_layout::CubeOut((size_t)(cu.on ? cu.cap : 0)).view(cu.on ? cu.ring.d_out[bi] : nullptr);
    if (cu.on) {
        // the LP points again, gated by the node LP's status as the heuristic is; a FOUND point goes through the heuristic
        // in place (rounding an integral point changes nothing and its repair is empty: the lift), gated by the cube's status
        if (int e = cu.ring.begin(ctx, bi, st)) return e;
        int crc = cube_launch(t->prob, st, P, S.d_x, hr.d_lu, hr.d_lu + t->n, t->d_int_idx, t->n_int, tree_cutoff(t), hr.tol,
                              mipx::kVarEps, cu.max_columns, nullptr, S.d.status, cu.d_ws, cu.ring.d_x[bi], co.obj, co.status, co.counts);
        if (crc) return crc;
        crc = heur_launch(t->prob, st, P, cu.ring.d_x[bi], hr.d_lu, hr.d_lu + t->n, t->d_int_idx, t->n_int, hr.tol, hr.max_moves,
                          nullptr, co.status, cu.ring.d_x[bi], co.obj, co.lift_status, co.lift_moves);
        if (crc) return crc;
        if (int e = cu.ring.end(ctx, bi, st)) return e;
        S.cube_n = P;
    }
    LsState &ls = t->ls;
    if (ls.on) {
        const auto lo = step_layout::LsOut((size_t)ls.cap).view(ls.ring.d_out[bi]);
        if (int e = ls.ring.begin(ctx, bi, st)) return e;
        const int lrc = ls_launch(t->prob, st, P, hr.ring.d_x[bi], hr.d_lu, hr.d_lu + t->n, t->d_int_idx, t->n_int, hr.tol, ls.max_moves,
                                  nullptr, o.status, hr.ring.d_x[bi], o.obj, lo.status, lo.moves);
        if (lrc) return lrc;
        if (fp.on) {   // ... and the lifted dive points, whose objectives and counts are in the dive's block
            const int drc = ls_launch(t->prob, st, P, hr.ring.d_x[bi], hr.d_lu, hr.d_lu + t->n, t->d_int_idx, t->n_int, hr.tol,
                                      ls.max_moves, nullptr, fo.lift_status, hr.ring.d_x[bi], fo.obj, fo.ls_status, fo.ls_moves);
            if (drc) return drc;
        }
        if (wr.on) {   // ... or the lifted points of the weighted repair, in its block
            const int wrc = ls_launch(t->prob, st, P, hr.ring.d_x[bi], hr.d_lu, hr.d_lu + t->n, t->d_int_idx, t->n_int, hr.tol,
                                      ls.max_moves, nullptr, wo.lift_status, hr.ring.d_x[bi], wo.obj, wo.ls_status, wo.ls_moves);
            if (wrc) return wrc;
        }
        if (cu.on) {   // ... and the lifted cube points, in their own block
            const int crc = ls_launch(t->prob, st, P, cu.ring.d_x[bi], hr.d_lu, hr.d_lu + t->n, t->d_int_idx, t->n_int, hr.tol,
                                      ls.max_moves, nullptr, co.lift_status, cu.ring.d_x[bi], co.obj, co.ls_status, co.ls_moves);
            if (crc) return crc;
        }
        if (int e = ls.ring.end(ctx, bi, st)) return e;
        S.ls_n = P;
    }
    // completion: behind the last stage of every block, the heuristic's slots (its own points and those of the dive or
    // the weighted repair) and the cube's FOUND points (a cube without a point leaves the LP point in its slot, which
    // is nobody's point), in one LP launch; point k of either block starts from the final basis of node LP k, the LP
    // whose solution it was made from (S.d_vout, level 0)
    S.comp_n = 0;
    S.comp_cube = false;
    CompState &cc = t->cc;
    if (cc.on && t->n_int < t->n) {
        const auto qo = step_layout::CompOut((size_t)cc.cap).view(cc.ring.d_out[bi]);
        const CompSrc src[2] = {{hr.ring.d_x[bi], nullptr, o.status, false, S.d_vout, P},
                                {cu.on ? cu.ring.d_x[bi] : nullptr, nullptr, co.status, true, S.d_vout, cu.on ? P : 0}};
        if (int e = cc.ring.begin(ctx, bi, st)) return e;
        const int qrc = comp_launch(t->prob, st, src, 2, hr.d_lu, hr.d_lu + t->n, t->d_int_idx, t->n_int, cc.ctol, cc.d_ws,
                                    cc.ring.d_x[bi], qo.obj, qo.status, qo.pivots);
        if (qrc) return qrc;
        if (int e = cc.ring.end(ctx, bi, st)) return e;
        S.comp_n = P;
        S.comp_cube = cu.on;
    }
    // LP dive: the LP points again, each inside its node's box (its pool row, as it is when the kernels run: behind the
    // node LPs of this step and before its finish) and warm from its node LP's final basis; while the host holds no
    // incumbent, or every ld.every steps
    S.lpdive_n = 0;
    LpdiveState &ld = t->ld;
    if (ld.on && (!(t->primal < std::numeric_limits<double>::infinity()) || (ld.every > 0 && t->steps % ld.every == 0))) {
        const auto dl = mipx::LpdiveOut((size_t)ld.cap).view(ld.ring.d_out[bi]);
        if (int e = ld.ring.begin(ctx, bi, st)) return e;
        const int drc = lpdive_launch(t->prob, st, P, S.d_x, t->pool_l, t->pool_u, S.d_slot, nullptr, S.d.status, S.d_vout,
                                      t->d_int_idx, t->n_int, ld.d_locks, tree_cutoff(t), ld.max_rounds, ld.rule, false, ld.d_ws,
                                      ld.ring.d_x[bi], dl.obj, dl.status, dl.rounds, dl.fixings, dl.flips, dl.pivots);
        if (drc) return drc;
        if (int e = ld.ring.end(ctx, bi, st)) return e;
        S.lpdive_n = P;
    }
    return MIPX_OK;
}

// The local search's counters over one block of `count` points: its own, or the one it fills inside the block of the
// dive, the weighted repair or the cube search.
void ls_count(LsState &ls, const int32_t *status, const int32_t *moves, int count) {
    for (int k = 0; k < count; k++) {
        if (status[k] == MIPX_LS_SKIPPED) continue;
        ls.run++;
        ls.singles += moves[2 * k];
        ls.pairs += moves[2 * k + 1];
        if (moves[2 * k] + moves[2 * k + 1] > 0) ls.improved++;
        if (status[k] == MIPX_LS_CAPPED) ls.capped++;
    }
}

// ... and what it found, before the step's nodes are evaluated: the best feasible point (ties: the lowest
// position) is the incumbent if it beats the one the tree holds -- as an incumbent received from an exchange.
int heur_step_collect(mipx_tree *t, StepBuf &S) {
    HeurState &hr = t->hr;
    const int bi = (int)(&S - t->buf), P = S.heur_n, n = t->n;
    S.heur_n = 0;
    const step_layout::HeurOut lay((size_t)hr.cap);
    int rc = hr.ring.fetch(t, bi, lay.bytes(), hr.us);
    if (rc) return rc;
    const auto o = lay.view((const char *)hr.ring.h_out[bi]);
    const double *obj = o.obj; const int32_t *status = o.status, *moves = o.moves;
    // local search: its counters; the objectives above are already the improved ones
    LsState &ls = t->ls;
    const int LP = S.ls_n;
    S.ls_n = 0;
    const int32_t *ls_moves = nullptr;
    if (LP > 0) {
        const step_layout::LsOut llay((size_t)ls.cap);
        if ((rc = ls.ring.fetch(t, bi, llay.bytes(), ls.us))) return rc;
        const auto lo = llay.view((const char *)ls.ring.h_out[bi]);
        ls_moves = lo.moves;
        ls_count(ls, lo.status, lo.moves, LP);
    }
    // fix-and-propagate dive: its counters, and which points are its own (their objectives are in its block)
    FpState &fp = t->fp;
    const int FP = S.fp_n;
    S.fp_n = 0;
    const double *fp_obj = nullptr;
    const int32_t *fp_ok = nullptr, *fp_ls_moves = nullptr;
    if (FP > 0) {
        const step_layout::FpOut flay((size_t)fp.cap);
        if ((rc = fp.ring.fetch(t, bi, flay.bytes(), fp.us))) return rc;
        const auto fo = flay.view((const char *)fp.ring.h_out[bi]);
        fp_obj = fo.obj;
        fp_ok = fo.lift_status;   // (0: the dive ended feasible and the heuristic's second pass lifted the point)
        for (int k = 0; k < FP; k++) {
            if (fo.status[k] == MIPX_FP_SKIPPED) continue;
            fp.tried++;
            fp.fixings += fo.counts[2 * k];
            fp.tries += fo.counts[2 * k + 1];
            if (fo.status[k] == MIPX_FP_FEASIBLE) fp.feasible++;
            if (fo.status[k] == MIPX_FP_STUCK) fp.stuck++;
            if (fo.status[k] == MIPX_FP_CAPPED) fp.capped++;
        }
        if (LP > 0) {
            fp_ls_moves = fo.ls_moves;
            ls_count(ls, fo.ls_status, fo.ls_moves, FP);
        }
    }
    // weighted row repair: the same in its block (it is never on together with the dive, so fp_* are free for it)
    WrState &wr = t->wr;
    const int WP = S.wr_n;
    S.wr_n = 0;
    if (WP > 0) {
        const step_layout::WrOut wlay((size_t)wr.cap);
        if ((rc = wr.ring.fetch(t, bi, wlay.bytes(), wr.us))) return rc;
        const auto wo = wlay.view((const char *)wr.ring.h_out[bi]);
        fp_obj = wo.obj;
        fp_ok = wo.lift_status;   // (0: the repair ended feasible and the heuristic's second pass lifted the point)
        for (int k = 0; k < WP; k++) {
            if (wo.status[k] == MIPX_WR_SKIPPED) continue;
            wr.tried++;
            wr.moves += wo.counts[2 * k];
            wr.bumps += wo.counts[2 * k + 1];
            if (wo.status[k] == MIPX_WR_FEASIBLE) wr.feasible++;
            if (wo.status[k] == MIPX_WR_CAPPED) wr.capped++;
        }
        if (LP > 0) {
            fp_ls_moves = wo.ls_moves;
            ls_count(ls, wo.ls_status, wo.ls_moves, WP);
        }
    }
    // cube search: its counters, and its points (a family of their own, in their own block)
    CubeState &cu = t->cu;
    const int CP = S.cube_n;
    S.cube_n = 0;
    const double *cu_obj = nullptr;
    const int32_t *cu_ok = nullptr, *cu_ls_moves = nullptr;
    if (CP > 0) {
        const step_layout::CubeOut clay((size_t)cu.cap);
        if ((rc = cu.ring.fetch(t, bi, clay.bytes(), cu.us))) return rc;
        const auto co = clay.view((const char *)cu.ring.h_out[bi]);
        cu_obj = co.obj;
        cu_ok = co.lift_status;   // (0: the cube held a point and the heuristic's pass lifted it)
        for (int k = 0; k < CP; k++) {
            if (co.status[k] == MIPX_CUBE_SKIPPED) continue;
            cu.tried++;
            cu.columns += co.counts[2 * k];
            if (co.counts[2 * k] == cu.max_columns) cu.at_cap++;
            if (co.status[k] == MIPX_CUBE_FOUND) cu.found++;
            if (co.status[k] == MIPX_CUBE_NONE) cu.none++;
        }
        if (LP > 0) {
            cu_ls_moves = co.ls_moves;
            ls_count(ls, co.ls_status, co.ls_moves, CP);
        }
    }
    // completion: its counters; a COMPLETED point stands in for its source point below, with the objective of its LP
    CompState &cc = t->cc;
    const int QP = S.comp_n;
    const bool q_cube = S.comp_cube;
    S.comp_n = 0;
    S.comp_cube = false;
    const double *q_obj = nullptr;
    const int32_t *q_status = nullptr;
    if (QP > 0) {
        const step_layout::CompOut qlay((size_t)cc.cap);
        if ((rc = cc.ring.fetch(t, bi, qlay.bytes(), cc.us))) return rc;
        const auto qo = qlay.view((const char *)cc.ring.h_out[bi]);
        q_obj = qo.obj;
        q_status = qo.status;
        for (int k = 0; k < (q_cube ? 2 : 1) * QP; k++) {
            if (qo.status[k] == MIPX_COMPLETE_SKIPPED) continue;
            cc.tried++;
            cc.pivots += qo.pivots[k];
            if (qo.status[k] == MIPX_COMPLETE_COMPLETED) cc.completed++;
            else if (qo.status[k] == MIPX_COMPLETE_INFEASIBLE) cc.infeasible++;
            else cc.failed++;
        }
    }
    int best = -1;
    bool best_fp = false, best_cube = false, best_comp = false;
    double best_obj = 0.0;
    for (int k = 0; k < P; k++) {
        const bool done = q_status && k < QP && q_status[k] == MIPX_COMPLETE_COMPLETED;   // (position k of the heuristic's block)
        const bool own = status[k] == MIPX_HEUR_FEASIBLE;
        const bool other = fp_ok && status[k] != MIPX_HEUR_SKIPPED && !own && fp_ok[k] == MIPX_HEUR_FEASIBLE;
        if (done && !own && !other) cc.rescued++;
        if (other || (done && !own)) {   // (the dive's or the repair's slot; a rescued point competes where they would)
            const double v = done ? q_obj[k] : fp_obj[k];
            if (best < 0 || v < best_obj) { best = k; best_fp = other; best_comp = done; best_obj = v; }
        }
        if (status[k] == MIPX_HEUR_SKIPPED) continue;
        hr.tried++;
        hr.repair += moves[2 * k];
        hr.lift += moves[2 * k + 1];
        if (status[k] == MIPX_HEUR_STUCK) hr.stuck++;
        if (status[k] == MIPX_HEUR_CAPPED) hr.capped++;
        if (!own) continue;
        hr.feasible++;
        const double v = done ? q_obj[k] : obj[k];
        if (best < 0 || v < best_obj) { best = k; best_fp = false; best_comp = done; best_obj = v; }
    }
    // (the cube's points behind the others: a tie goes to the earlier family, then to the lowest position)
    for (int k = 0; k < CP; k++) {
        const bool done = q_status && q_cube && k < QP && q_status[QP + k] == MIPX_COMPLETE_COMPLETED;
        const bool own = cu_ok[k] == MIPX_HEUR_FEASIBLE;
        if (done && !own) cc.rescued++;
        if (!done && !own) continue;
        const double v = done ? q_obj[QP + k] : cu_obj[k];
        if (best < 0 || v < best_obj) { best = k; best_fp = false; best_cube = true; best_comp = done; best_obj = v; }
    }
    // LP dive: its counters, and its FEASIBLE points, a family of their own behind every other
    LpdiveState &ld = t->ld;
    const int DP = S.lpdive_n;
    S.lpdive_n = 0;
    bool best_ld = false;
    if (DP > 0) {
        const mipx::LpdiveOut dlay((size_t)ld.cap);
        if ((rc = ld.ring.fetch(t, bi, dlay.bytes(), ld.us))) return rc;
        const auto dl = dlay.view((const char *)ld.ring.h_out[bi]);
        for (int k = 0; k < DP; k++) {
            if (dl.status[k] == MIPX_LPDIVE_SKIPPED) continue;
            ld.tried++;
            ld.moves += dl.fixings[k] + dl.flips[k];
            ld.pivots += dl.pivots[k];
            if (dl.status[k] == MIPX_LPDIVE_INFEASIBLE || dl.status[k] == MIPX_LPDIVE_CUTOFF) ld.infeasible++;
            else if (dl.status[k] != MIPX_LPDIVE_FEASIBLE) ld.failed++;
            if (dl.status[k] != MIPX_LPDIVE_FEASIBLE) continue;
            ld.feasible++;
            if (best < 0 || dl.obj[k] < best_obj) {
                best = k; best_fp = false; best_cube = false; best_comp = false; best_ld = true; best_obj = dl.obj[k];
            }
        }
    }
    if (best >= 0 && best_obj < t->primal) {
        t->primal = best_obj;
        // (the block that won: a completed point lies in the completion's, at its source's position)
        const double *from = best_ld ? ld.ring.d_x[bi] : best_comp ? cc.ring.d_x[bi] + (best_cube ? (size_t)QP * n : 0) : best_cube ? cu.ring.d_x[bi] : hr.ring.d_x[bi];
        if (best_comp) cc.installed++;
        if (best_ld) ld.installed++;
        if ((rc = tree_d2h(t, t->best_x.data(), from + (size_t)best * n, (size_t)n * 8))) return rc;
        t->have_x = true;
        // (the point is a closed leaf of value obj: without it no closed leaf holds the incumbent's value, and the
        // dual bound of an emptied queue would end above the incumbent instead of on it)
        t->closed_min = std::fmin(t->closed_min, best_obj);
        hr.installed++;
        if (best_fp) (WP > 0 ? wr.installed : fp.installed)++;
        if (best_cube) cu.installed++;
        const int32_t *lm = best_ld ? nullptr : best_cube ? cu_ls_moves : best_fp ? fp_ls_moves : ls_moves;
        if (lm && lm[2 * best] + lm[2 * best + 1] > 0) ls.installed++;
    }
    return MIPX_OK;
}

// ---- bound propagation (include/mipx_prop.h) ---------------------------------------------------------------
// One launch of prop_bounds over `batch` boxes in device memory, queued on `st` (d_slot: the rows of d_l, d_u the
// nodes are, or null for rows 0 .. batch - 1; d_l_out, d_u_out may be d_l, d_u).
int prop_launch(const mipx_problem *p, hipStream_t st, int batch, const int32_t *d_slot, const double *d_l, const double *d_u,
                const int32_t *d_int_idx, int n_int, double cutoff, double tol, int max_rounds, double *d_l_out,
                double *d_u_out, int32_t *d_status, int32_t *d_changed, int32_t *d_rounds, int32_t *d_capped) {
    mipx_ctx *ctx = p->ctx;
    if (p->m > mipx::kPropMax || p->n > mipx::kPropMax) return fail(ctx, MIPX_ETOOBIG, "bound propagation: more than 1024 rows or columns");
    if (batch <= 0) return MIPX_OK;
    mipx::PropArgs a;
    a.m = p->m; a.n = p->n; a.n_int = n_int; a.max_rounds = max_rounds;
    a.cut = std::isfinite(cutoff) ? 1 : 0; a.tol = tol; a.cutoff = cutoff;
    a.A = p->dA; a.b = p->db; a.c = p->dc; a.int_idx = d_int_idx; a.slot = d_slot;
    a.l = d_l; a.u = d_u; a.l_out = d_l_out; a.u_out = d_u_out;
    a.status_out = d_status; a.changed_out = d_changed; a.rounds_out = d_rounds; a.capped_out = d_capped;
    hipLaunchKernelGGL(mipx::prop_bounds, dim3((unsigned)batch), dim3(mipx::kPropNT), 0, st, a);
    HIP_TRY(ctx, hipGetLastError());
    return MIPX_OK;
}

// The step's nodes through the propagation, in place on their pool rows, in front of their node LPs.
int prop_step_launch(mipx_tree *t, StepBuf &S) {
    PropState &pg = t->pg;
    mipx_ctx *ctx = t->ctx;
    hipStream_t st = ctx->stream;
    const int bi = (int)(&S - t->buf), B = S.B;
    const auto o = step_layout::PropOut((size_t)pg.cap).view(pg.ring.d_out[bi]);
    const double cutoff = pg.use_cutoff ? tree_cutoff(t) : std::numeric_limits<double>::infinity();
    if (int e = pg.ring.begin(ctx, bi, st)) return e;
    const int rc = prop_launch(t->prob, st, B, S.d_slot, t->pool_l, t->pool_u, t->d_int_idx, t->n_int, cutoff, pg.tol,
                               pg.max_rounds, t->pool_l, t->pool_u, o.status, o.changed, o.rounds, o.capped);
    if (rc) return rc;
    if (int e = pg.ring.end(ctx, bi, st)) return e;
    S.prop_n = B;
    return MIPX_OK;
}

// ... and what it found, once the step is done: the counters, and the nodes found infeasible (inf[k] != 0).
int prop_step_collect(mipx_tree *t, StepBuf &S, std::vector<uint8_t> &inf) {
    PropState &pg = t->pg;
    const int bi = (int)(&S - t->buf), B = S.prop_n;
    S.prop_n = 0;
    const step_layout::PropOut lay((size_t)pg.cap);
    const int rc = pg.ring.fetch(t, bi, lay.bytes(), pg.us);
    if (rc) return rc;
    const auto o = lay.view((const char *)pg.ring.h_out[bi]);
    inf.assign((size_t)B, 0);
    for (int k = 0; k < B; k++) {
        pg.nodes++;
        pg.changed += o.changed[k];
        pg.rounds += o.rounds[k];
        pg.capped += o.capped[k];
        if (o.status[k] == MIPX_PROP_TIGHTENED) pg.tightened++;
        if (o.status[k] == MIPX_PROP_INFEASIBLE) { pg.infeasible++; inf[(size_t)k] = 1; }
    }
    return MIPX_OK;
}

constexpr int kAskCap = 2048;  // probe requests per step carried in the packed read-back
constexpr int kMaxDive = 8;    // dive children in a row per node (buffers are sized for it)

// ---- reduced-cost tightening (include/mipx_rcfix.h) --------------------------------------------------------
static_assert(kRcLevels == 1 + kMaxDive, "RcState keeps an event pair per level of a step");
// One launch of rc_tighten over `batch` nodes in device memory, queued on `st` (d_slot: the rows of d_l, d_u the
// nodes are, d_pos: their rows of d_y, or null for rows 0 .. batch - 1; d_l_out, d_u_out may be d_l, d_u; d_z may
// be null).
int rc_launch(const mipx_problem *p, hipStream_t st, int batch, const int32_t *d_slot, const int32_t *d_pos, const double *d_l,
              const double *d_u, const double *d_y, const int32_t *d_int_idx, int n_int, double cutoff, double tol, double dtol,
              double *d_l_out, double *d_u_out, double *d_z, int32_t *d_status, int32_t *d_changed) {
    mipx_ctx *ctx = p->ctx;
    if (p->m > mipx::kRcMax || p->n > mipx::kRcMax) return fail(ctx, MIPX_ETOOBIG, "reduced-cost tightening: more than 1024 rows or columns");
    if (batch <= 0) return MIPX_OK;
    mipx::RcArgs a;
    a.m = p->m; a.n = p->n; a.n_int = n_int; a.cutoff = cutoff; a.tol = tol; a.dtol = dtol;
    a.A = p->dA; a.b = p->db; a.c = p->dc; a.int_idx = d_int_idx; a.slot = d_slot; a.pos = d_pos;
    a.l = d_l; a.u = d_u; a.y = d_y; a.l_out = d_l_out; a.u_out = d_u_out; a.z_out = d_z;
    a.status_out = d_status; a.changed_out = d_changed;
    hipLaunchKernelGGL(mipx::rc_tighten, dim3((unsigned)batch), dim3(mipx::kRcNT), 0, st, a);
    HIP_TRY(ctx, hipGetLastError());
    return MIPX_OK;
}

step_layout::RcOut rc_layout(const mipx_tree *t) { return {(size_t)kRcLevels, (size_t)t->rc.cap}; }

// What the launches of S's last finish found, once they are done: the counters and the kernel's device time.
int rc_step_collect(mipx_tree *t, StepBuf &S) {
    if (S.rc_cnt.empty()) return MIPX_OK;
    RcState &rs = t->rc;
    mipx_ctx *ctx = t->ctx;
    const int bi = (int)(&S - t->buf);
    const step_layout::RcOut lay = rc_layout(t);
    HIP_TRY(ctx, hipStreamSynchronize(S.rc_stream));
    const int rc = tree_d2h(t, (char *)rs.h_io[bi] + lay.status, (const char *)rs.d_io[bi] + lay.status, lay.bytes() - lay.status);
    if (rc) return rc;
    const auto o = lay.view((const int32_t *)rs.h_io[bi]);
    for (size_t level = 0; level < S.rc_cnt.size(); level++) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, rs.e0[bi][level], rs.e1[bi][level]) == hipSuccess) rs.us += 1000.0 * ms;
        rs.launches++;
        for (size_t k = lay.level(level), end = k + (size_t)S.rc_cnt[level]; k < end; k++) {
            rs.nodes++;
            rs.changed += o.changed[k];
            if (o.status[k] == MIPX_RCFIX_TIGHTENED) rs.tightened++;
            if (o.status[k] == MIPX_RCFIX_CUT_OFF) rs.cut_off++;
            if (o.status[k] == MIPX_RCFIX_NO_BOUND) rs.no_bound++;
        }
    }
    S.rc_cnt.clear();
    return MIPX_OK;
}

// The branching parents of S's levels staged for the tightening: their (pool row, output position) lists in one
// copy on `cs`, in front of the level-by-level launches (rc_level_launch).
int rc_step_stage(mipx_tree *t, StepBuf &S, hipStream_t cs, int levels) {
    RcState &rs = t->rc;
    const int bi = (int)(&S - t->buf);
    const step_layout::RcOut lay = rc_layout(t);
    const auto h = lay.view(rs.h_io[bi]);
    for (int level = 0; level < levels; level++) {
        const auto &bl = S.br[(size_t)level];
        if (bl.pos.empty()) break;
        if (bl.pos.size() > (size_t)rs.cap) return fail(t->ctx, MIPX_ENOMEM, "tree: more branching parents in a level than the batch holds");
        std::memcpy(h.slot + lay.level((size_t)level), bl.slot.data(), bl.slot.size() * 4);
        std::memcpy(h.pos + lay.level((size_t)level), bl.pos.data(), bl.pos.size() * 4);
    }
    HIP_TRY(t->ctx, hipMemcpyAsync(rs.d_io[bi], rs.h_io[bi], lay.in_bytes(), hipMemcpyHostToDevice, cs));
    S.rc_stream = cs;
    return MIPX_OK;
}

// Level `level`'s `count` parents through rc_tighten on `cs`, in place on their pool rows.
int rc_level_launch(mipx_tree *t, StepBuf &S, hipStream_t cs, int level, int count) {
    RcState &rs = t->rc;
    mipx_ctx *ctx = t->ctx;
    const int bi = (int)(&S - t->buf);
    const step_layout::RcOut lay = rc_layout(t);
    const auto d = lay.view(rs.d_io[bi]);
    const size_t off = lay.level((size_t)level);
    HIP_TRY(ctx, hipEventRecord(rs.e0[bi][level], cs));
    const int rc = rc_launch(t->prob, cs, count, d.slot + off, d.pos + off, t->pool_l, t->pool_u, rs.d_y[bi], t->d_int_idx, t->n_int,
                             tree_cutoff(t), rs.tol, rs.dtol, t->pool_l, t->pool_u, nullptr, d.status + off, d.changed + off);
    if (rc) return rc;
    HIP_TRY(ctx, hipEventRecord(rs.e1[bi][level], cs));
    S.rc_cnt.push_back(count);
    return MIPX_OK;
}

// The step buffers (step_layout.h) at this tree's dimensions.  The element sizes the layouts take are the
// kernels' types: a probe request, an open entry, and the summary in front of the table block at 128.
using step_layout::CutState;
using Ask = mipx::ScoreArgs::Ask;
static_assert(sizeof(mipx::FinishSummary) == 128, "step_layout::FinishBlock keeps 128 bytes for the summary");
static_assert(alignof(Ask) <= 16 && alignof(mipx::OpenEntry) <= 32, "step_layout aligns requests to 16, open entries to 32");
step_layout::StepPack step_pack(const mipx_tree *t, int levels) { return {(size_t)levels, (size_t)t->max_batch, (size_t)kAskCap, sizeof(Ask)}; }
step_layout::FinishBlock finish_block(const mipx_tree *t, size_t per) { return {t->tab_bytes, per, (size_t)t->max_batch, sizeof(mipx::OpenEntry)}; }

// The packed read-back laid out for `levels` = 1 + dive output levels: the layout and its device view.
void layout_pack(mipx_tree *t, StepBuf &S, int levels) {
    S.pack = step_pack(t, levels);
    S.d = S.pack.view(S.d_pack);
}

int launch_score(mipx_tree *t, StepBuf &S, int batch, bool side = false, bool no_ask = false, int side_stream = -1) {
    const bool on_st2 = side_stream < 0 ? side : side_stream == 1;   // (default: the side tables go with the side stream)
    hipStream_t where = side_stream == 2 ? t->stf : on_st2 ? t->st2 : t->ctx->stream;   // (2: the finish stream)
    mipx::ScoreArgs s;
    s.n = t->n; s.n_int = t->n_int; s.batch = batch; s.rule = t->rule;
    s.int_idx = t->d_int_idx; s.x = S.d_x; s.status = S.d.status;
    const TabPtr tb = tab_at(t, t->fast_ok ? t->tab_host : 0);
    s.cost_l = side ? t->d_cost_l2 : tb.cl; s.cost_r = side ? t->d_cost_r2 : tb.cr;
    s.has_entry = side ? t->d_has2 : tb.has;
    s.branch_idx = S.d.bidx; s.branch_val = S.d.bval; s.mip_feasible = S.d.mipf;
    s.n_probe = S.d.nprobe;
    s.probe_list = S.d_plist;
    s.ask_count = S.d.ask_count; s.ask_cap = kAskCap; s.ask = (side || no_ask) ? nullptr : (Ask *)S.d.ask;
    s.ask_nodes = S.B;  // dive children (positions >= B) are never probed in their own step
    if (!side && !no_ask && !(S.dive && batch == (S.dive + 1) * S.B && !S.scored_once))
        HIP_TRY(t->ctx, hipMemsetAsync(S.d.ask_count, 0, 16, side_stream == 2 ? t->stf : t->ctx->stream));
    if (!no_ask) S.scored_once = true;
    hipLaunchKernelGGL(mipx::branch_score, dim3(batch), dim3(64), 0, where, s);
    HIP_TRY(t->ctx, hipGetLastError());
    return MIPX_OK;
}

// pseudo_cost.py:68-100
void pc_update(mipx_tree *t, int var, int dir, int lp_status, double objective, double dual_bound,
               double variable_change) {
    double &cost = dir ? t->cost_r[var] : t->cost_l[var];
    int32_t &times = dir ? t->times_r[var] : t->times_l[var];
    const size_t n = (size_t)t->n;
    if (lp_status == 0 || lp_status == 3) {
        double bc = objective - dual_bound;
        if (bc < 0) bc = 0;
        cost = (cost * (double)times + bc / variable_change) / (double)(times + 1);
        if (t->comm) t->pc_own[(dir ? n : 0) + (size_t)var] += bc / variable_change;   // this rank's samples, in sum form
    } else if (t->comm) {
        // a sample that counts without a cost leaves the mean where it is (pseudo_cost.py:97-100): in
        // sum form it weighs in with the current mean, so that sum / times reproduces the recurrence
        t->pc_own[(dir ? n : 0) + (size_t)var] += cost;
    }
    times += 1;
    if (t->comm) t->pc_own[(dir ? 3 * n : 2 * n) + (size_t)var] += 1.0;
    t->has_entry[var] = 1;
    if (t->fast_ok) {   // the device holds the table: the sample follows (pc_apply, tree_finish)
        mipx::PcSample sm;
        sm.var_dir = 2 * var + dir; sm.status = lp_status; sm.obj = objective; sm.bound = dual_bound; sm.vc = variable_change;
        t->pend_samples.push_back(sm);
    }
}

// A filled FinishArgs -- and with pseudo costs (g.rule == 1) the table version the step's samples go to -- as
// launches on st: the one place the finish kernels are launched from (launch_finish below, and
// mipx_finish_step_batch of finish_api.hip.h on caller data).
void enqueue_finish(const mipx::FinishArgs &g, const mipx::PcApplyArgs *a, hipStream_t st) {
    const int B = g.B;
    hipLaunchKernelGGL(mipx::finish_candidates, dim3((B + 255) / 256), dim3(256), 0, st, g);
    hipLaunchKernelGGL(mipx::finish_prefix_min, dim3(1), dim3(1024), 0, st, g);
    hipLaunchKernelGGL(mipx::finish_decide, dim3((B + 255) / 256), dim3(256), 0, st, g);
    hipLaunchKernelGGL(mipx::finish_scan, dim3(1), dim3(1024), 0, st, g);
    if (g.n <= 256) hipLaunchKernelGGL((mipx::finish_write<1>), dim3(B), dim3(256), 0, st, g);
    else if (g.n <= 512) hipLaunchKernelGGL((mipx::finish_write<2>), dim3(B), dim3(256), 0, st, g);
    else hipLaunchKernelGGL((mipx::finish_write<4>), dim3(B), dim3(256), 0, st, g);
    if (g.rule == 1) {
        hipLaunchKernelGGL(mipx::finish_samples, dim3((B + 255) / 256), dim3(256), 0, st, g);
        hipLaunchKernelGGL(mipx::pc_apply, dim3(2 * g.n), dim3(64), 0, st, *a);
    }
}

// Everything the six kernels of a cut round read and write, as device pointers: the engine fills one from its tree
// and step buffers (cut_round_data below), mipx_cut_round_*_batch of cutround_api.hip.h from a caller's arrays.
struct CutRoundData {
    int n = 0, m0 = 0, mstride = 0, kc = 0, B = 0, slab_rows = 0;
    // cut_round_begin
    int round = 0, max_rounds = 0, have_dump = 0;
    double progress_tol = 0.0, max_dual_bound = 0.0;
    const int32_t *status = nullptr, *mipf = nullptr;
    const double *obj = nullptr, *y = nullptr;
    int8_t *vstat = nullptr;
    int32_t *ncut = nullptr, *ids = nullptr, *state = nullptr;
    double *obj_before = nullptr;
    int32_t *active = nullptr, *resolve = nullptr, *need_tab = nullptr, *counters = nullptr;
    // K2, pool_append, K3, cut_round_apply
    const double *A = nullptr, *b = nullptr, *T = nullptr, *x = nullptr;
    const int32_t *idx = nullptr;
    const uint8_t *is_int = nullptr;
    double max_term = 0.0, min_cut_depth = 0.0, cos_parallel = 0.0, max_abs_coef = 0.0;
    int max_nonzero_coefs = 0, mfma = 0;
    double *slab_pi = nullptr, *slab_pi0 = nullptr;
    int32_t *pool_list = nullptr;
    double *store_pi = nullptr, *store_pi0 = nullptr;
    int32_t *store_count = nullptr;
    int store_cap = 0;
    int32_t *k2_ncuts = nullptr, *k3_nadded = nullptr, *k3_added = nullptr, *k3_term = nullptr;
};

// The first half of a cut round as launches on st: with `gather` the working copies of the nodes' cut lists first
// (cut_gather_state, the start of a step), then cut_round_begin.  The one place the two are launched from (the
// engine's step start and tree_cut_rounds, and mipx_cut_round_begin_batch on caller data).
int enqueue_cut_begin(mipx_ctx *ctx, const CutRoundData &d, const mipx::CutGatherArgs *gather, bool begin, hipStream_t st) {
    if (gather != nullptr) {
        hipLaunchKernelGGL(mipx::cut_gather_state, dim3(d.B), dim3(64), 0, st, *gather);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (!begin) return MIPX_OK;
    mipx::CutRoundArgs ra;
    ra.n = d.n; ra.m0 = d.m0; ra.mstride = d.mstride; ra.kc = d.kc; ra.batch = d.B; ra.round = d.round;
    ra.max_rounds = d.max_rounds;
    ra.progress_tol = d.progress_tol; ra.max_dual_bound = d.max_dual_bound;
    ra.status = d.status; ra.obj = d.obj; ra.mipf = d.mipf; ra.y = d.y; ra.vstat = d.vstat;
    ra.ncut = d.ncut; ra.ids = d.ids; ra.state = d.state; ra.obj_before = d.obj_before;
    ra.active = d.active; ra.resolve = d.resolve; ra.counters = d.counters;
    ra.have_dump = d.have_dump; ra.need_tab = d.need_tab;
    hipLaunchKernelGGL(mipx::cut_round_begin, dim3(d.B), dim3(64), 0, st, ra);
    HIP_TRY(ctx, hipGetLastError());
    return MIPX_OK;
}

// The workgroups per node and the cuts per group K2 runs with: 0 asks for the engine's rule (few nodes: their cuts
// spread over more workgroups; the largest group whose staging fits the LDS that many workgroups leave each other).
void cut_launch_shape(const CutRoundData &d, int &chunks, int &group) {
    if (chunks == 0) chunks = d.B >= 256 ? 1 : (d.B >= 32 ? 4 : 16);
    if (group == 0) group = mipx::gomory_group(d.n, d.mstride, (long)d.B * chunks);
}

// The second half as launches on st: K2 into the nodes' slabs, pool_append, K3 over the pool lists, cut_round_apply.
// The one place the four are launched from in their engine form.  marks (optional): three events, recorded before
// K2, behind it and behind K3 (the engine's k2_ms / k3_ms).
int enqueue_cut_generate(mipx_ctx *ctx, const CutRoundData &d, int chunks, int group, hipStream_t st,
                         const hipEvent_t *marks = nullptr) {
    const int B = d.B, n = d.n;
    cut_launch_shape(d, chunks, group);
    mipx::GomoryArgs ga;
    ga.m = d.m0; ga.n = n; ga.batch = B;
    ga.A = d.A; ga.b = d.b;
    ga.T = d.T; ga.idx = d.idx; ga.x = d.x; ga.is_int = d.is_int;
    ga.max_term = d.max_term;
    ga.ncuts = d.k2_ncuts; ga.row_idx = nullptr; ga.pi = nullptr; ga.pi0 = nullptr;
    ga.safe_pi = nullptr; ga.safe_pi0 = nullptr;
    ga.chunks = chunks;
    ga.ncut = d.ncut; ga.cut_ids = d.ids; ga.cut_pi = d.store_pi; ga.cut_pi0 = d.store_pi0;
    ga.cut_stride = d.kc; ga.mstride = d.mstride; ga.vstat = d.vstat; ga.clip_x = 1;
    ga.active = d.active;
    ga.slab_pi = d.slab_pi; ga.slab_pi0 = d.slab_pi0;
    ga.slab_n = d.state + (size_t)mipx::CF_SLAB_N * B; ga.slab_rows = d.slab_rows;
    ga.group = group;
    ga.mfma = d.mfma;
    const size_t lds2 = mipx::gomory_lds_bytes(n, d.mstride, ga.group);
    if (marks) HIP_TRY(ctx, hipEventRecord(marks[0], st));
    if (lds2 > 64 * 1024)
        HIP_TRY(ctx, hipFuncSetAttribute((const void *)mipx::gomory_cuts<256>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2));
    hipLaunchKernelGGL((mipx::gomory_cuts<256>), dim3(B * ga.chunks), dim3(256), lds2, st, ga);
    HIP_TRY(ctx, hipGetLastError());
    if (marks) HIP_TRY(ctx, hipEventRecord(marks[1], st));
    mipx::PoolAppendArgs pa;
    pa.batch = B; pa.slab_rows = d.slab_rows; pa.active = d.active; pa.k2_ncuts = d.k2_ncuts;
    pa.state = d.state; pa.pool_list = d.pool_list;
    hipLaunchKernelGGL(mipx::pool_append, dim3((B + 63) / 64), dim3(64), 0, st, pa);
    HIP_TRY(ctx, hipGetLastError());
    mipx::SelectArgs sa;
    sa.n = n; sa.batch = B; sa.kmax = d.slab_rows;
    sa.npool = d.state + (size_t)mipx::CF_POOL_N * B; sa.pi = d.slab_pi; sa.pi0 = d.slab_pi0; sa.x = d.x;
    sa.max_nonzero_coefs = d.max_nonzero_coefs; sa.min_cut_depth = d.min_cut_depth;
    sa.cos_parallel = d.cos_parallel; sa.max_abs_coef = d.max_abs_coef;
    sa.nadded = d.k3_nadded; sa.added = d.k3_added; sa.terminator = d.k3_term; sa.depth = nullptr;
    sa.pool_list = d.pool_list; sa.clip_x = 1; sa.active = d.active;
    const size_t lds3 = (size_t)d.slab_rows * (3 * 8 + 2 * 4) + 16 + 64;
    hipLaunchKernelGGL(mipx::select_cuts, dim3(B), dim3(256), lds3, st, sa);
    HIP_TRY(ctx, hipGetLastError());
    if (marks) HIP_TRY(ctx, hipEventRecord(marks[2], st));
    mipx::CutApplyArgs aa;
    aa.n = n; aa.m0 = d.m0; aa.mstride = d.mstride; aa.kc = d.kc; aa.batch = B; aa.slab_rows = d.slab_rows;
    aa.active = d.active; aa.k3_nadded = d.k3_nadded; aa.k3_added = d.k3_added;
    aa.slab_pi = d.slab_pi; aa.slab_pi0 = d.slab_pi0; aa.pool_list = d.pool_list;
    aa.vstat = d.vstat; aa.ncut = d.ncut; aa.ids = d.ids; aa.state = d.state;
    aa.store_pi = d.store_pi; aa.store_pi0 = d.store_pi0; aa.store_count = d.store_count;
    aa.store_cap = d.store_cap;
    aa.resolve = d.resolve; aa.counters = d.counters;
    hipLaunchKernelGGL(mipx::cut_round_apply, dim3(B), dim3(256), 0, st, aa);
    HIP_TRY(ctx, hipGetLastError());
    return MIPX_OK;
}

// the kernels that finish a step on the device, queued behind its scoring
int launch_finish(mipx_tree *t, StepBuf &S) {
    mipx_ctx *ctx = t->ctx;
    hipStream_t st = t->stf;   // (behind the step's scoring, queued there by tree_launch)
    const int prev = t->tab_tail;
    S.tabv = (prev + 1) % kTabV;
    t->tab_tail = S.tabv;
    t->tab_late[S.tabv] = false;   // (written afresh: a copy of the tail, which holds every late update queued so far)
    if (t->rule == 1)
        HIP_TRY(ctx, hipMemcpyAsync(tab_at(t, S.tabv).cl, tab_at(t, prev).cl, t->tab_bytes, hipMemcpyDeviceToDevice, st));
    const int B = S.B;
    const size_t MB = (size_t)t->max_batch;
    const auto par = step_layout::ParentBlock((size_t)B, 2 * (1 + (size_t)t->dive)).view((const char *)S.d_par);
    mipx::FinishArgs g;
    g.n = t->n; g.m = t->m; g.B = B; g.dive = S.dive; g.rule = t->rule;
    g.status = S.d.status; g.bidx = S.d.bidx; g.mipf = S.d.mipf; g.nprobe = S.d.nprobe; g.npiv = S.d.npiv;
    g.dvar = S.d.dvar; g.ddir = S.d.ddir; g.obj = S.d.obj; g.bval = S.d.bval; g.dval = S.d.dval;
    g.ask_count = S.d.ask_count; g.ask_cap = kAskCap; g.vout = S.d_vout;
    g.slot = S.d_slot;
    g.par_d = par.par_d; g.par_i = par.par_i; g.budget = par.budget;
    g.pool_l = t->pool_l; g.pool_u = t->pool_u; g.pool_v = t->pool_v; g.primal = t->d_primal;
    g.c_info = S.c_info; g.c_cnt = S.c_cnt; g.c_eval = S.c_eval; g.c_val = S.c_val; g.c_flag = S.c_flag;
    g.sum = S.d_sum; g.open = S.d_open; g.dead = S.d_dead; g.samples = S.d_samples; g.sample_keys = S.d_skeys;
    g.c_run = S.c_val + 2 * MB;
    mipx::PcApplyArgs a;
    if (t->rule == 1) {
        const TabPtr tb = tab_at(t, S.tabv);
        a.n = t->n; a.sum = S.d_sum; a.count = -1; a.samples = S.d_samples; a.keys = S.d_skeys;
        a.cost_l = tb.cl; a.cost_r = tb.cr; a.has = tb.has; a.times = tb.times; a.own = tb.own;
    }
    enqueue_finish(g, t->rule == 1 ? &a : nullptr, st);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(S.done, st));
    return MIPX_OK;
}

// The host replaced the table (mipx_tree_set_pseudo_costs): a new version at the tail, read from now on.
// Rare and blocking: nothing else orders a host-side replacement against the steps in flight.
int table_replace(mipx_tree *t) {
    mipx_ctx *ctx = t->ctx;
    const size_t n = (size_t)t->n;
    HIP_TRY(ctx, hipStreamSynchronize(t->stf));
    const int prev = t->tab_tail, w = (prev + 1) % kTabV;
    const TabPtr src = tab_at(t, prev), dst = tab_at(t, w);
    HIP_TRY(ctx, hipMemcpy(dst.cl, src.cl, t->tab_bytes, hipMemcpyDeviceToDevice));
    HIP_TRY(ctx, hipMemcpy(dst.cl, t->cost_l.data(), n * 8, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(dst.cr, t->cost_r.data(), n * 8, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(dst.has, t->has_entry.data(), n, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(dst.times, t->times_l.data(), n * 4, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(dst.times + n, t->times_r.data(), n * 4, hipMemcpyHostToDevice));
    t->tab_tail = w;
    t->tab_host = w;
    t->table_dirty = false;
    t->times_dirty = false;
    return MIPX_OK;
}

// ---- host spill (include/mipx_spill.h) ----
inline bool spilled(int32_t slot) { return slot <= -2; }
int spill_steps(const mipx_tree *t) { return t->max_batch > 1 ? 3 : 1; }
// the rows a step launch must find free so that batch_size() grants the whole batch (see the header)
int64_t spill_headroom(const mipx_tree *t) {
    return (int64_t)spill_steps(t) * t->max_batch * (2 * (1 + (int64_t)t->dive) + 1);
}
int64_t spill_max_record(const mipx_tree *t) {
    return mipx::spill_record_bytes(t->n, t->cuts ? t->kc : 0, t->n + t->mrows, t->cuts ? t->kc : 0);
}
mipx::SpillArgs spill_args(mipx_tree *t) {
    mipx::SpillArgs a;
    a.n = t->n; a.nv = t->n + t->mrows; a.kc = t->cuts ? t->kc : 0;
    a.root_l = t->hs.d_root; a.root_u = t->hs.d_root + t->n;
    a.l = t->pool_l; a.u = t->pool_u; a.v = t->pool_v; a.ncut = t->pool_ncut; a.ids = t->pool_ids;
    return a;
}

// a spilled record leaves the store (reloaded, or its node closed unevaluated); an emptied segment is freed later
void spill_release(mipx_tree *t, int32_t slot) {
    HostSpill &h = t->hs;
    const int32_t li = -2 - slot;
    SpillSeg &g = h.segs[(size_t)h.loc[(size_t)li].seg];
    if (--g.live == 0) {
        h.dead.push_back(g.host);
        h.bytes -= g.bytes;
        g.host = nullptr;
        g.bytes = 0;
        h.seg_free.push_back(h.loc[(size_t)li].seg);
    }
    h.loc_free.push_back(li);
    h.on_host--;
}

// Decode a spilled node's record on the host (peek_open / peek_cuts): bounds, the whole basis row, cut list.
void spill_decode(const mipx_tree *t, int32_t slot, double *l, double *u, int8_t *v, int32_t *ids) {
    const SpillLoc &lc = t->hs.loc[(size_t)(-2 - slot)];
    const char *p = t->hs.segs[(size_t)lc.seg].host + lc.off;
    const int n = t->n, nv = t->n + t->mrows;
    int32_t nd, ncut;
    std::memcpy(&nd, p + 8, 4);
    std::memcpy(&ncut, p + 12, 4);
    const int64_t o_l = 16 + mipx::spill_pad8(4 * (int64_t)nd), o_u = o_l + 8 * (int64_t)nd, o_v = o_u + 8 * (int64_t)nd;
    if (l) std::memcpy(l, t->root_l.data(), (size_t)n * 8);
    if (u) std::memcpy(u, t->root_u.data(), (size_t)n * 8);
    for (int32_t q = 0; q < nd; q++) {
        int32_t c;
        std::memcpy(&c, p + 16 + 4 * (size_t)q, 4);
        if (l) std::memcpy(l + c, p + o_l + 8 * (size_t)q, 8);
        if (u) std::memcpy(u + c, p + o_u + 8 * (size_t)q, 8);
    }
    for (int j = 0; v && j < nv; j++) {
        const uint8_t c = (uint8_t)p[o_v + j / 2];
        v[j] = (int8_t)((int8_t)(j & 1 ? c : (uint8_t)(c << 4)) >> 4);
    }
    if (ids && ncut > 0) std::memcpy(ids, p + o_v + mipx::spill_pad8((nv + 1) / 2), (size_t)ncut * 4);
}

// One spill event: the worst-keyed resident open nodes (the queue pops them last) go to the host until
// `target` rows are free.  Only open nodes move: the rows of the steps in flight -- their batches, and with the
// device finish the budgets they took at launch -- are not in the queue.  Returns MIPX_ENOMEM when the records
// would exceed the host cap (nothing moved).
int spill_event(mipx_tree *t, int64_t target) {
    mipx_ctx *ctx = t->ctx;
    HostSpill &h = t->hs;
    const auto t0 = std::chrono::steady_clock::now();
    for (char *q : h.dead) (void)hipHostFree(q);
    h.dead.clear();
    std::vector<BucketQueue::Item> items;
    if (t->use_bq) t->bq.items(items);
    else for (const auto &it : t->heap.h) items.push_back({it.key, it.id});
    items.erase(std::remove_if(items.begin(), items.end(), [&](const BucketQueue::Item &it) { return t->nodes[it.id].slot < 0; }),
                items.end());
    const int64_t K = std::min<int64_t>(target - (int64_t)t->free_slots.size(), (int64_t)items.size());
    if (K <= 0) return MIPX_OK;
    auto worse = [](const BucketQueue::Item &a, const BucketQueue::Item &b) { return a.key > b.key || (a.key == b.key && a.id > b.id); };
    std::nth_element(items.begin(), items.begin() + (K - 1), items.end(), worse);
    items.resize((size_t)K);
    std::sort(items.begin(), items.end(), [](const BucketQueue::Item &a, const BucketQueue::Item &b) { return a.id < b.id; });
    if ((size_t)K > h.vict_cap) {
        const size_t c = std::max<size_t>((size_t)K, 2 * h.vict_cap);
        (void)hipFree(h.d_slot); (void)hipFree(h.d_id); (void)hipFree(h.d_off);
        h.d_slot = nullptr; h.d_id = nullptr; h.d_off = nullptr; h.vict_cap = 0;
        if (dmalloc(ctx, &h.d_slot, c) || dmalloc(ctx, &h.d_id, c) || dmalloc(ctx, &h.d_off, c + 1)) return MIPX_EHIP;
        h.vict_cap = c;
    }
    std::vector<int32_t> rows((size_t)K);
    std::vector<int64_t> ids((size_t)K), off((size_t)K + 1);
    for (int64_t k = 0; k < K; k++) { ids[(size_t)k] = items[(size_t)k].id; rows[(size_t)k] = t->nodes[items[(size_t)k].id].slot; }
    hipStream_t st = h.st;
    if (t->child_recorded) HIP_TRY(ctx, hipStreamWaitEvent(st, t->ev_child, 0));   // (host finish: children rows being written)
    HIP_TRY(ctx, hipMemcpyAsync(h.d_slot, rows.data(), (size_t)K * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(h.d_id, ids.data(), (size_t)K * 8, hipMemcpyHostToDevice, st));
    mipx::SpillArgs a = spill_args(t);
    a.slot = h.d_slot; a.node_id = h.d_id; a.off = h.d_off;
    enqueue_spill_count(a, (int)K, st);
    enqueue_spill_scan(a, (int)K, st);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(off.data(), h.d_off, ((size_t)K + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    const int64_t total = off[(size_t)K];
    if (h.bytes + total > h.cap) return MIPX_ENOMEM;
    if ((size_t)total > h.rec_cap) {
        (void)hipFree(h.d_rec);
        h.d_rec = nullptr;
        h.rec_cap = 0;
        if (dmalloc(ctx, &h.d_rec, (size_t)total + (size_t)total / 2)) return MIPX_EHIP;
        h.rec_cap = (size_t)total + (size_t)total / 2;
    }
    char *seg = nullptr;
    HIP_TRY(ctx, hipHostMalloc((void **)&seg, (size_t)total, hipHostMallocDefault));
    a.rec = h.d_rec;
    enqueue_spill_pack(a, (int)K, st);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(seg, h.d_rec, (size_t)total, hipMemcpyDeviceToHost, st));
    if (hipError_t e = hipStreamSynchronize(st)) {
        (void)hipHostFree(seg);
        return fail(ctx, MIPX_EHIP, "tree: host spill", e);
    }
    // the copy is complete: the rows are free from here on
    int32_t si;
    if (!h.seg_free.empty()) { si = h.seg_free.back(); h.seg_free.pop_back(); }
    else { si = (int32_t)h.segs.size(); h.segs.emplace_back(); }
    h.segs[(size_t)si] = {seg, total, K};
    for (int64_t k = 0; k < K; k++) {
        int32_t li;
        if (!h.loc_free.empty()) { li = h.loc_free.back(); h.loc_free.pop_back(); }
        else { li = (int32_t)h.loc.size(); h.loc.emplace_back(); }
        h.loc[(size_t)li] = {si, (int32_t)(off[(size_t)k + 1] - off[(size_t)k]), off[(size_t)k]};
        t->nodes[ids[(size_t)k]].slot = -2 - li;
        t->free_slots.push_back(rows[(size_t)k]);
    }
    h.bytes += total;
    h.peak = std::max(h.peak, h.bytes);
    h.spilled += K;
    h.on_host += K;
    h.events++;
    h.spill_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    return MIPX_OK;
}

// Before a launch: make sure batch_size() can grant `want` nodes (their children rows, those of the steps in
// flight where the host finishes them, and a row per spilled node of the batch).  Below that, one event spills
// down to a low watermark a further headroom (or an eighth of the pool) lower, so that events stay rare.
int spill_room(mipx_tree *t, int want, int64_t inflight) {
    const int64_t per = 2 * (1 + (int64_t)t->dive);
    // (a traced step is finished on the host, whatever fast_ok says: its children take their rows then)
    const int64_t need = per * want + (t->fast_ok && !t->trace ? 0 : per * inflight) + want;
    if ((int64_t)t->free_slots.size() >= need) return MIPX_OK;
    const int64_t target = need + std::max(spill_headroom(t), t->capacity / 8);
    const int rc = spill_event(t, target);
    if (rc == MIPX_ENOMEM) {   // the host store is full: stop as a full pool stops
        t->pool_exhausted = true;
        (void)fail(t->ctx, MIPX_ENOMEM, "tree: node pool and host spill store exhausted (search stopped; raise max_host_bytes)");
        return MIPX_OK;
    }
    return rc;
}

// tree_launch: rows for the batch's spilled nodes and their records staged (the unpack is queued by
// spill_reload_enqueue, behind the children rows of the last finished step)
int spill_assign(mipx_tree *t, StepBuf &S) {
    HostSpill &h = t->hs;
    const auto t0 = std::chrono::steady_clock::now();
    const int B = (int)S.ids.size();
    const size_t MB = (size_t)t->max_batch;
    int64_t *off = (int64_t *)S.h_rl;
    int32_t *rows = (int32_t *)(S.h_rl + (MB + 1) * 8);
    char *rec = S.h_rl + (MB + 1) * 8 + (MB * 4 + 7) / 8 * 8;
    int r = 0;
    off[0] = 0;
    for (int k = 0; k < B; k++) {
        const int32_t sl = S.slots[(size_t)k];
        if (!spilled(sl)) continue;
        if (t->free_slots.empty())   // (batch_size() reserves a row per node of the batch while nodes are on the host)
            return fail(t->ctx, MIPX_ENOMEM, "tree: no pool row for a node coming back from the host");
        const SpillLoc &lc = h.loc[(size_t)(-2 - sl)];
        std::memcpy(rec + off[r], h.segs[(size_t)lc.seg].host + lc.off, (size_t)lc.bytes);
        off[r + 1] = off[r] + lc.bytes;
        spill_release(t, sl);
        rows[r] = t->free_slots.back();
        t->free_slots.pop_back();
        S.slots[(size_t)k] = rows[r];
        r++;
    }
    S.rl_n = r;
    h.reloaded += r;
    h.reload_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    return MIPX_OK;
}

int spill_reload_enqueue(mipx_tree *t, StepBuf &S) {
    mipx_ctx *ctx = t->ctx;
    const int r = S.rl_n;
    S.rl_n = 0;
    if (r == 0) return MIPX_OK;
    const size_t MB = (size_t)t->max_batch, o_rows = (MB + 1) * 8, o_rec = o_rows + (MB * 4 + 7) / 8 * 8;
    const int64_t bytes = ((const int64_t *)S.h_rl)[r];
    hipStream_t st = t->ctx->stream;
    HIP_TRY(ctx, hipMemcpyAsync(S.d_rl, S.h_rl, ((size_t)r + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(S.d_rl + o_rows, S.h_rl + o_rows, (size_t)r * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(S.d_rl + o_rec, S.h_rl + o_rec, (size_t)bytes, hipMemcpyHostToDevice, st));
    mipx::SpillArgs a = spill_args(t);
    a.off = (int64_t *)S.d_rl; a.slot = (const int32_t *)(S.d_rl + o_rows); a.rec = S.d_rl + o_rec;
    enqueue_spill_unpack(a, r, st);
    HIP_TRY(ctx, hipGetLastError());
    return MIPX_OK;
}

// First half of a step: pop the batch and enqueue its node LPs + scoring (no host wait).
int tree_launch(mipx_tree *t, StepBuf &S, int want) {
    mipx_ctx *ctx = t->ctx;
    hipStream_t st = ctx->stream;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto tp = now();
    // 1. pop the batch (a node whose inherited bound cannot beat the incumbent is closed unevaluated)
    std::vector<int64_t> &ids = S.ids;
    std::vector<int32_t> &slots = S.slots;
    ids.clear();
    slots.clear();
    S.recs.clear();
    S.B = 0;
    S.in_flight = false;
    S.inflight_min = std::numeric_limits<double>::infinity();
    const double cut = tree_cutoff(t);   // (the incumbent does not change while the batch is popped)
    auto take = [&](int64_t id) {
        if (t->search != 0) t->is_open[id] = 0;
        NodeRec &nd = t->nodes[id];
        const int32_t slot = nd.slot;
        nd.slot = -1;  // (the row itself is released when the step is finished)
        if (!(nd.dual_bound < cut)) {
            // (closed only because of the objective step: nothing in it is below the incumbent, a leaf of that value)
            const bool by_step = nd.dual_bound < t->primal;
            if (by_step) t->os.popped++;
            t->closed_min = std::fmin(t->closed_min, by_step ? t->primal : nd.dual_bound);
            if (t->tr.on) t->tr.closed(id);
            if (spilled(slot)) spill_release(t, slot);   // (its record is dropped, never reloaded)
            else t->free_slots.push_back(slot);
            return;
        }
        ids.push_back(id);
        slots.push_back(slot);
        S.recs.push_back(nd);
        S.inflight_min = std::fmin(S.inflight_min, nd.dual_bound);
        { const int64_t age = t->steps + 1 - nd.born; t->age_hist[age < 1 ? 0 : age > 7 ? 7 : age]++; t->depth_sum += nd.depth; }
    };
    if (t->use_bq) {
        while ((int)ids.size() < want && !t->bq.empty()) {
            t->popped.clear();
            t->bq.pop_batch((size_t)want - ids.size(), t->popped);
            const size_t np = t->popped.size();
            for (size_t i = 0; i < np; i++) {  // the node table is far bigger than the caches
                if (i + 16 < np) __builtin_prefetch(&t->nodes[t->popped[i + 16].id], 1);
                take(t->popped[i].id);
            }
        }
    } else {
        while ((int)ids.size() < want && !tree_queue_empty(t)) take(t->heap.pop());
    }
    const int B = (int)ids.size();
    if (B == 0) return MIPX_OK;
    if (cut < t->primal) t->os.launches++;
    if (t->hs.on_host > 0) {   // (rows for the batch's spilled nodes: before the budget below)
        const int arc = spill_assign(t, S);
        if (arc) return arc;
    }
    S.B = B;
    S.in_flight = true;
    t->steps++;
    t->phase_ms[0] += std::chrono::duration<double, std::milli>(now() - tp).count();
    if (t->fast_ok && t->table_dirty) {
        const int trc = table_replace(t);
        if (trc) return trc;
    }
    if (t->fast_ok && t->tab_late[t->tab_host]) {   // late samples / a merge on their way into the version read below
        HIP_TRY(ctx, hipStreamWaitEvent(st, t->ev_tab[t->tab_host], 0));
        t->tab_late[t->tab_host] = false;
    }
    if (t->table_dirty) {  // pseudo-cost table as of the last finished step
        const size_t n = t->n;
        // (one copy from the pinned mirror; the previous upload has long been consumed: two steps ago)
        char *ht = t->h_tab + (size_t)(t->steps & 3) * 17 * n;  // (four mirrors in turn: three steps can be in flight)
        std::memcpy(ht, t->cost_l.data(), n * 8);
        std::memcpy(ht + n * 8, t->cost_r.data(), n * 8);
        std::memcpy(ht + 2 * n * 8, t->has_entry.data(), n);
        HIP_TRY(ctx, hipMemcpyAsync(t->d_cost_l, ht, 17 * n, hipMemcpyHostToDevice, st));
        t->table_dirty = false;
    }
    S.fast = t->fast_ok && !t->trace;
    if (t->fast_ok && t->rule == 1 && std::getenv("MIPX_DEBUG_TABLE")) {
        // debugging aid: the version the launch reads against the host's snapshot (equal when nothing is in flight)
        (void)hipStreamSynchronize(t->stf);
        std::vector<char> blk(t->tab_bytes);
        (void)hipMemcpy(blk.data(), tab_at(t, t->tab_host).cl, t->tab_bytes, hipMemcpyDeviceToHost);
        const size_t n = (size_t)t->n;
        const double *cl = (const double *)blk.data(), *cr = cl + n;
        const uint8_t *has = (const uint8_t *)(blk.data() + 16 * n);
        const int32_t *tl = (const int32_t *)(blk.data() + t->tab_off2), *tr = tl + n;
        int bad = 0;
        for (size_t j = 0; j < n; j++)
            if (cl[j] != t->cost_l[j] || cr[j] != t->cost_r[j] || has[j] != t->has_entry[j] || tl[j] != t->times_l[j] || tr[j] != t->times_r[j]) {
                if (bad++ < 4)
                    std::fprintf(stderr, "[mipx table] step %lld var %zu: device (%.17g %.17g has %d times %d %d) host (%.17g %.17g has %d times %d %d)\n",
                                 (long long)t->steps, j, cl[j], cr[j], has[j], tl[j], tr[j], t->cost_l[j], t->cost_r[j], t->has_entry[j], t->times_l[j], t->times_r[j]);
            }
        if (bad) std::fprintf(stderr, "[mipx table] step %lld: %d entries differ (version %d, tail %d)\n", (long long)t->steps, bad, t->tab_host, t->tab_tail);
    }
    if (S.fast) {
        if (t->primal < t->primal_sent) {   // the host knows a better incumbent than the device (exchange, host-finished step)
            hipLaunchKernelGGL(mipx::primal_lower, dim3(1), dim3(1), 0, t->stf, t->d_primal, t->primal);
            t->primal_sent = t->primal;
        }
        // the parents' records and the pool rows the children may take: chain k, level p, direction d owns
        // budget[k][2 p + d] (the claim batch_size() left room for, handed out up front)
        const size_t per = 2 * (1 + (size_t)t->dive), need = per * (size_t)B;
        if (t->free_slots.size() < need)   // (batch_size() left room for them: this would be an accounting bug)
            return fail(ctx, MIPX_ENOMEM, "tree: fewer free pool rows than the batch's children budget");
        S.budget.assign(t->free_slots.end() - (std::ptrdiff_t)need, t->free_slots.end());
        t->free_slots.resize(t->free_slots.size() - need);
        const step_layout::ParentBlock lay((size_t)B, per);
        const auto par = lay.view(S.h_par);
        for (int k = 0; k < B; k++) {
            const NodeRec &nd = S.recs[(size_t)k];
            par.par_d[k] = nd.dual_bound; par.par_d[B + k] = nd.b_val;
            par.par_i[k] = nd.b_idx; par.par_i[B + k] = nd.b_dir; par.par_i[2 * B + k] = nd.depth; par.par_i[3 * B + k] = nd.anchor;
        }
        std::memcpy(par.budget, S.budget.data(), need * 4);
        HIP_TRY(ctx, hipMemcpyAsync(S.d_par, S.h_par, lay.bytes(), hipMemcpyHostToDevice, st));
    }
    std::memcpy(S.h_slot, slots.data(), (size_t)B * 4);
    for (int k = 0; k < B; k++) S.h_slot[B + k] = S.recs[(size_t)k].anchor;  // [pool rows | anchor-table entries]
    HIP_TRY(ctx, hipMemcpyAsync(S.d_slot, S.h_slot, (size_t)B * 8, hipMemcpyHostToDevice, st));
    // 2. LP relaxations + scoring (after the children records of the last finished step)
    if (t->child_pending) {
        HIP_TRY(ctx, hipStreamWaitEvent(st, t->ev_child, 0));
        t->child_pending = false;
    }
    if (S.rl_n > 0) {   // the batch's spilled nodes back into their rows (the rows may have fed those children)
        const int rrc = spill_reload_enqueue(t, S);
        if (rrc) return rrc;
    }
    S.dive = t->dive;  // (register tiles and the HBM-streaming kernel alike)
    S.scored_once = false;
    int rc = MIPX_OK;
    if (t->cuts) {
        // working copies of the nodes' cut lists, the loop state zeroed; then the node LPs over their
        // m + ncut rows (row duals kept: the slack-cut removal reads them) and the integrality test
        HIP_TRY(ctx, hipMemsetAsync(S.cs_counters, 0, 16, st));
        mipx::CutGatherArgs ga;
        ga.batch = B; ga.kc = t->kc; ga.slot = S.d_slot;
        ga.pool_ncut = t->pool_ncut; ga.pool_ids = t->pool_ids;
        ga.ncut = S.w_ncut; ga.ids = S.w_ids; ga.state = S.cs_state; ga.counters = S.cs_counters;
        CutRoundData cd;
        cd.B = B;
        if ((rc = enqueue_cut_begin(ctx, cd, &ga, false, st))) return rc;   // (the gather alone: the node LPs come first)
        int maxc = 0;
        for (int k = 0; k < B; k++) maxc = std::max(maxc, (int)S.recs[(size_t)k].ncut);
        CutLaunch cl;
        cl.ncut = S.w_ncut; cl.ids = S.w_ids; cl.y = S.d_y; cl.m_rows = t->m + maxc;
        if (t->cp.exact_tableau == 0) {   // the tableau the solve ends with is the first round's (K2's input)
            cl.dT = S.dump_T; cl.dvec = S.dump_vec; cl.didx = S.dump_idx;
        }
        HIP_TRY(ctx, hipEventRecord(S.e0, st));
        t->cold_launch = B == 1 && t->nodes.size() == 1 && S.recs[0].depth == 0 && S.recs[0].b_idx == -1 && S.recs[0].ncut == 0 &&
                         !t->prob->anchor_on && !t->rs.on;   // (the root alone, never solved, no cut yet: one cold LP)
        rc = launch_lp(t, B, t->pool_l, t->pool_u, t->pool_v, S.d_slot, 0, S.d.status, S.d.obj, S.d_x,
                       S.d_vout, S.d_iters, S.d.npiv, nullptr, nullptr, S.d_slot + B, &cl);
        if (rc) return rc;
        HIP_TRY(ctx, hipEventRecord(S.e1, st));
        if ((rc = launch_score(t, S, B, false, true))) return rc;
        HIP_TRY(ctx, hipEventRecord(S.done, st));
        return MIPX_OK;
    }
    S.prop_n = 0;
    if (t->pg.on && (rc = prop_step_launch(t, S))) return rc;   // (bound propagation: in place, in front of the node LPs)
    HIP_TRY(ctx, hipEventRecord(S.e0, st));
    // the root alone, never solved: one cold LP (above the register tiles it is spread over the chip, K1c)
    t->cold_launch = B == 1 && t->nodes.size() == 1 && S.recs[0].depth == 0 && S.recs[0].b_idx == -1 && !t->prob->anchor_on &&
                     !t->rs.on;   // (a restart's root is a seed: its row holds the source's root basis)
    rc = launch_lp(t, B, t->pool_l, t->pool_u, t->pool_v, S.d_slot, 0, S.d.status, S.d.obj,
                   S.d_x, S.d_vout, S.d_iters, S.d.npiv, nullptr, S.dive ? &S : nullptr, S.d_slot + B, nullptr,
                   t->df.on ? S.df_y : t->rc.on ? t->rc.d_y[&S - t->buf] : nullptr);   // (the two exclude each other)
    if (rc) return rc;
    HIP_TRY(ctx, hipEventRecord(S.e1, st));
    if (S.fast) {
        // scoring and finish beside the node LPs of the next step: stf waits for this step's node LPs, the main
        // stream goes straight on to the next launch
        HIP_TRY(ctx, hipStreamWaitEvent(t->stf, S.e1, 0));
        if ((rc = launch_score(t, S, (S.dive + 1) * B, false, false, 2))) return rc;
        return launch_finish(t, S);   // (records S.done behind the finish, on stf)
    }
    if ((rc = launch_score(t, S, (S.dive + 1) * B))) return rc;
    if (t->hr.on && (rc = heur_step_launch(t, S))) return rc;
    HIP_TRY(ctx, hipEventRecord(S.done, st));
    return MIPX_OK;
}

// The cut loop of BaseNode._base_bound (base_node.py:196-203) for the whole batch at once: round r
// of every node that is still generating runs together.  Per round two small read-backs (how many
// nodes go on; how many LPs changed and the largest row count), everything else stays on the device:
//   cut_round_begin   stall test of the last round, loop condition, slack-cut removal   (:292-341)
//   K1                the tableau of the basis on the remaining rows                     (:513-526)
//   K2 + pool_append  GMI cuts, safely rounded, into the node's pool                     (:365-385, :468-511)
//   K3                selection                                                          (:387-454)
//   cut_round_apply   selected cuts -> cut store, node list, basis; pool minus selected  (:456-463)
//   K1 + K4           re-solve of the nodes whose rows changed, integrality test         (:319)
// A node whose rows did not change is not re-solved (the reference re-solves the unchanged LP and
// gets the same objective: it stalls either way).
int tree_cut_rounds(mipx_tree *t, StepBuf &S) {
    mipx_ctx *ctx = t->ctx;
    hipStream_t st = ctx->stream;
    const int B = S.B, n = t->n;
    const CutState cs((size_t)t->max_batch);
    const int32_t *cnt = cs.counters(S.h_cs);
    int maxc = 0;
    for (int k = 0; k < B; k++) maxc = std::max(maxc, (int)S.recs[(size_t)k].ncut);
    // Without exact_tableau every LP launch of the loop dumps the tableau it ends with, and K2 reads that:
    // a launch of its own for the tableau only where a round starts by removing rows.  (exact_tableau:
    // the tableau is refactored from the slack basis like the per-node path's, always by its own launch.)
    const bool fused = t->cp.exact_tableau == 0;
    CutRoundData cd;
    cd.n = n; cd.m0 = t->m; cd.mstride = t->mrows; cd.kc = t->kc; cd.B = B; cd.slab_rows = t->slab_rows;
    cd.max_rounds = t->cp.max_cut_generation_iterations; cd.have_dump = fused ? 1 : 0;
    cd.progress_tol = t->cp.cutting_plane_progress_tolerance; cd.max_dual_bound = t->cp.max_dual_bound;
    cd.status = S.d.status; cd.obj = S.d.obj; cd.mipf = S.d.mipf; cd.y = S.d_y; cd.vstat = S.d_vout;
    cd.ncut = S.w_ncut; cd.ids = S.w_ids; cd.state = S.cs_state; cd.obj_before = S.cs_before;
    cd.active = S.cs_active; cd.resolve = S.cs_resolve; cd.need_tab = S.cs_need_tab; cd.counters = S.cs_counters;
    cd.A = t->prob->dA; cd.b = t->prob->db; cd.T = S.dump_T; cd.idx = S.dump_idx; cd.x = S.d_x; cd.is_int = t->d_is_int;
    cd.max_term = t->cp.max_term; cd.max_nonzero_coefs = t->cp.max_nonzero_coefs; cd.min_cut_depth = t->cp.min_cut_depth;
    cd.cos_parallel = t->cp.cos_parallel; cd.max_abs_coef = t->cp.max_abs_coef;
    cd.mfma = (std::getenv("MIPX_K2_MFMA") && std::atoi(std::getenv("MIPX_K2_MFMA"))) ? 1 : 0;   // (experiment: cut_kernels.hip.h)
    cd.slab_pi = S.slab_pi; cd.slab_pi0 = S.slab_pi0; cd.pool_list = S.pool_list;
    cd.store_pi = t->store_pi; cd.store_pi0 = t->store_pi0; cd.store_count = t->store_count;
    cd.store_cap = (int)(t->store_cap - t->cm_rows);   // (the migration region is not K3's)
    cd.k2_ncuts = S.k2_ncuts; cd.k3_nadded = S.k3_nadded; cd.k3_added = S.k3_added; cd.k3_term = S.k3_term;
    for (int round = 0;; round++) {
        HIP_TRY(ctx, hipMemsetAsync(S.cs_counters, 0, 8, st));   // n_active, n_changed (max_ncut stays)
        HIP_TRY(ctx, hipMemsetAsync(S.cs_counters + 3, 0, 4, st));   // n_need_tab
        cd.round = round;
        int rc = enqueue_cut_begin(ctx, cd, nullptr, true, st);
        if (rc) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(S.h_cs, S.cs_counters, 16, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        if (cnt[CutState::kActive] == 0) break;   // nobody generates any more
        // the tableau of every generating node's basis (refactorisation from the slack basis -- or,
        // without exact_tableau, from the root's anchor where the node has no cut rows -- then zero
        // iterations: the basis is optimal), dumped for K2
        if (cnt[CutState::kNeedTab] > 0) {
            CutLaunch cl;
            cl.ncut = S.w_ncut; cl.ids = S.w_ids; cl.vstat_by_node = 1; cl.active = S.cs_need_tab;
            cl.m_rows = t->m + maxc; cl.dT = S.dump_T; cl.dvec = S.dump_vec; cl.didx = S.dump_idx;
            cl.no_anchor = t->cp.exact_tableau != 0;
            rc = launch_lp(t, B, t->pool_l, t->pool_u, S.d_vout, S.d_slot, 0, nullptr, nullptr, nullptr,
                           nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &cl);
            if (rc) return rc;
        }
        const hipEvent_t marks[3] = {S.k2a, S.k2b, S.k3b};
        if ((rc = enqueue_cut_generate(ctx, cd, 0, 0, st, marks))) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(S.h_cs, S.cs_counters, 16, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        {   // (the stream is idle: the round's kernel times for the roofline entries of the cut configs)
            float a = 0.f, b = 0.f;
            if (hipEventElapsedTime(&a, S.k2a, S.k2b) == hipSuccess) t->k2_ms += a;
            if (hipEventElapsedTime(&b, S.k2b, S.k3b) == hipSuccess) t->k3_ms += b;   // (pool_append + K3)
        }
        const int changed = cnt[CutState::kChanged];
        maxc = std::max(maxc, (int)cnt[CutState::kMaxNcut]);
        if (changed > 0) {   // re-solve where rows came or went, warm from the node's own basis (:319)
            CutLaunch rl;
            rl.ncut = S.w_ncut; rl.ids = S.w_ids; rl.vstat_by_node = 1; rl.active = S.cs_resolve;
            rl.y = S.d_y; rl.m_rows = t->m + maxc;
            if (fused) { rl.dT = S.dump_T; rl.dvec = S.dump_vec; rl.didx = S.dump_idx; }
            rl.no_anchor = true;   // (a node that changed rows has, or just had, cut rows)
            rc = launch_lp(t, B, t->pool_l, t->pool_u, S.d_vout, S.d_slot, 0, S.d.status, S.d.obj, S.d_x,
                           S.d_vout, S.d_iters, S.d.npiv, nullptr, nullptr, nullptr, &rl);
            if (rc) return rc;
            if ((rc = launch_score(t, S, B, false, true))) return rc;
            t->lps += changed;
            t->cut_resolves += changed;
        }
    }
    // per node: rounds and the six GMIC counters, its final number of cut rows
    // (fields 0..6 lie behind one another on the device; with a full batch also on the host: one copy)
    static_assert((int)CutState::kStateFields == (int)mipx::CF_N_REMOVED + 1, "the state fields the host reads: rounds .. n_removed");
    if ((size_t)B == cs.max_batch) {
        HIP_TRY(ctx, hipMemcpyAsync(cs.field(S.h_cs, 0), S.cs_state, CutState::kStateFields * (size_t)B * 4, hipMemcpyDeviceToHost, st));
    } else {
        for (int f = 0; f < CutState::kStateFields; f++)
            HIP_TRY(ctx, hipMemcpyAsync(cs.field(S.h_cs, f), S.cs_state + (size_t)f * B, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(ctx, hipMemcpyAsync(cs.field(S.h_cs, CutState::kRowsAfter), S.w_ncut, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(cs.field(S.h_cs, CutState::kDropped), S.cs_state + (size_t)mipx::CF_DROPPED * B, (size_t)B * 4,
                                hipMemcpyDeviceToHost, st));
    // the final scoring of the batch (branching variable, strong-branching requests)
    int rc = launch_score(t, S, B);
    if (rc) return rc;
    HIP_TRY(ctx, hipEventRecord(S.done, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    for (int k = 0; k < B; k++) {
        for (int f = 0; f < CutState::kStateFields; f++) t->cut_totals[f] += *cs.field(S.h_cs, f, (size_t)k);
        t->cut_totals[7] += *cs.field(S.h_cs, CutState::kDropped, (size_t)k);
    }
    return MIPX_OK;
}

// The table block as the device holds it -> the host's vectors (a snapshot: x_fill_record, the API, the
// re-scoring of a host-finished step read them).
void table_snapshot(mipx_tree *t, const char *blk) {
    const size_t n = (size_t)t->n;
    std::memcpy(t->cost_l.data(), blk, n * 8);
    std::memcpy(t->cost_r.data(), blk + n * 8, n * 8);
    std::memcpy(t->has_entry.data(), blk + 16 * n, n);
    std::memcpy(t->times_l.data(), blk + t->tab_off2, n * 4);
    std::memcpy(t->times_r.data(), blk + t->tab_off2 + n * 4, n * 4);
    if (t->comm) std::memcpy(t->pc_own.data(), blk + t->tab_off2 + 8 * n, 4 * n * 8);
}

// Second half of a step the device finished (finish_kernels.hip.h): counters, the new open nodes into the
// node table and the queue, the free rows back, the incumbent, the table snapshot.
int tree_finish_fast(mipx_tree *t, StepBuf &S, const mipx::FinishSummary &sum, std::vector<int> &deferred) {
    mipx_ctx *ctx = t->ctx;
    const int B = S.B, n = t->n;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto tp = now();
    deferred.clear();
    t->lps += (B - sum.n_deferred) + sum.dives;
    t->dives += sum.dives;
    t->evaluated += sum.evaluated;
    t->pivots += sum.pivots;
    t->closed_min = std::fmin(t->closed_min, sum.closed_min);
    if (sum.unbounded) t->unbounded = true;
    const size_t per = 2 * (1 + (size_t)t->dive);
    if (sum.n_open < 0 || (size_t)sum.n_open > per * (size_t)B || sum.n_dead < 0 || (size_t)sum.n_dead > per * (size_t)B ||
        (size_t)sum.n_open + (size_t)sum.n_dead != per * (size_t)B)
        return fail(ctx, MIPX_EHIP, "tree: the device finish returned an inconsistent summary");
    const auto fin = finish_block(t, per).view(S.h_fin);
    const bool tab = t->rule == 1;
    mipx::OpenEntry *open = (mipx::OpenEntry *)fin.open;
    if (tab) HIP_TRY(ctx, hipMemcpyAsync(fin.table, tab_at(t, S.tabv).cl, t->tab_bytes, hipMemcpyDeviceToHost, t->st2));
    t->tab_host = S.tabv;   // launches from now on read the table as of this step
    if (sum.n_open > 0)
        HIP_TRY(ctx, hipMemcpyAsync(open, S.d_open, (size_t)sum.n_open * sizeof(mipx::OpenEntry), hipMemcpyDeviceToHost, t->st2));
    if (sum.n_dead > 0)
        HIP_TRY(ctx, hipMemcpyAsync(fin.dead, S.d_dead, (size_t)sum.n_dead * 4, hipMemcpyDeviceToHost, t->st2));
    if (sum.n_deferred > 0)   // the nodes that filed probe requests: everything the host loop reads per node
        HIP_TRY(ctx, hipMemcpyAsync(S.h_pack, S.d_pack, S.pack.bytes(), hipMemcpyDeviceToHost, t->st2));
    HIP_TRY(ctx, hipStreamSynchronize(t->st2));
    if (sum.n_deferred > 0) {
        const auto hv = S.pack.view((const char *)S.h_pack);
        const int32_t asked = *hv.ask_count;
        if (asked < 1 || asked > kAskCap) return fail(ctx, MIPX_EHIP, "tree: the device finish deferred nodes without a request list");
        const Ask *ask = (const Ask *)hv.ask;
        for (int32_t q = 0; q < asked; q++) deferred.push_back(ask[q].node);
        std::sort(deferred.begin(), deferred.end());
        deferred.erase(std::unique(deferred.begin(), deferred.end()), deferred.end());
        if ((int)deferred.size() != sum.n_deferred) return fail(ctx, MIPX_EHIP, "tree: deferred nodes and request list disagree");
    }
    t->phase_ms[1] += std::chrono::duration<double, std::milli>(now() - tp).count(); tp = now();
    if (tab) table_snapshot(t, fin.table);
    // the new open nodes, in the order the host loop created them (chain by chain, level by level, left
    // then right)
    const bool defer_push = t->use_bq && t->search == 0;
    t->pend.clear();
    for (int q = 0; q < sum.n_open; q++) {
        const mipx::OpenEntry &e = open[q];
        NodeRec c;
        c.dual_bound = e.key;
        c.depth = e.depth;
        c.key = t->search == 0 ? e.key : -(double)e.depth;
        c.b_idx = e.bidx_dir >> 1; c.b_dir = e.bidx_dir & 1; c.b_val = e.bval;
        c.born = (int32_t)t->steps; c.anchor = e.anchor; c.ncut = 0; c.slot = e.slot;
        t->nodes.push_back(c);
        const int64_t cid = (int64_t)t->nodes.size() - 1;
        if (defer_push) t->pend.push_back({c.key, cid});
        else tree_push(t, cid);
    }
    if (defer_push) t->bq.push_many(t->pend.data(), t->pend.size());
    // rows free again: the budget rows that hold no open node, the batch's own rows
    t->free_slots.insert(t->free_slots.end(), fin.dead, fin.dead + sum.n_dead);
    if (deferred.empty()) {
        t->free_slots.insert(t->free_slots.end(), S.slots.begin(), S.slots.begin() + B);
    } else {    // (a deferred node's row feeds its children: the host part releases it)
        size_t d = 0;
        for (int k = 0; k < B; k++) {
            if (d < deferred.size() && deferred[d] == k) { d++; continue; }
            t->free_slots.push_back(S.slots[(size_t)k]);
        }
    }
    S.budget.clear();
    t->phase_ms[3] += std::chrono::duration<double, std::milli>(now() - tp).count(); tp = now();
    t->primal_sent = std::fmin(t->primal_sent, sum.primal);
    if (sum.incumbent_pos >= 0 && sum.primal < t->primal) {
        t->primal = sum.primal;
        int rc = tree_d2h(t, t->best_x.data(), S.d_x + (size_t)sum.incumbent_pos * n, (size_t)n * 8);
        if (rc) return rc;
        t->have_x = true;
    }
    // anchor mode: the root's optimal tableau (a root that needed no probe comes this way)
    if (t->anchor_mode && !t->anchor_set && S.ids[0] == 0 && (deferred.empty() || deferred[0] != 0)) {
        int32_t st0 = -1;
        int rc = tree_d2h(t, &st0, S.d.status, 4);
        if (rc) return rc;
        if (st0 == 0) {
            std::vector<int8_t> rootv((size_t)t->n + t->m);
            HIP_TRY(ctx, hipMemcpy(rootv.data(), S.d_vout, rootv.size(), hipMemcpyDeviceToHost));
            const int arc = mipx_problem_set_anchor(t->prob, rootv.data());
            if (arc) return arc;
            t->anchor_set = true;
        }
    }
    t->phase_ms[4] += std::chrono::duration<double, std::milli>(now() - tp).count();
    return MIPX_OK;
}

// ---- second half of a step on the host: tree_finish and its phases ------------------------------------------
// What crosses the phases of one host finish.
struct FinishWork {
    using Clock = std::chrono::steady_clock;
    StepBuf &S;
    const bool overlapped;   // a step is in flight on the main stream: probes and re-scoring go to the side stream
    Clock::time_point tp = Clock::now();     // start of the span the next phase_ms[] slot is charged with
    step_layout::StepPack::View<char> h{};   // the host copy of the packed read-back
    // The nodes this finish handles, in order.  The whole batch: the nodes without probe requests first, then those
    // with (each group in batch order) -- the order in which the device finish and the host part share a step, so that
    // both ways end with the same table, ids and queue.  partial (device finish): only the nodes it deferred.
    std::vector<int> todo;
    bool partial = false;
    std::vector<uint8_t> prop_inf;           // bound propagation: the nodes it found infeasible
    int64_t prop_asks = 0, total = 0;        // probe requests in the packed list: of those nodes, of the todo nodes
    std::vector<int32_t> pair_pos, pair_var, pair_slot, pst;   // the probes: parent position, variable, row; LP status
    std::vector<double> xrow, pobj;                            // x of the probed variables; the probes' objectives
    int incumbent_pos = -1;
    std::vector<DfEntry> df_recs, df_infs;   // (dual function: this step's solved and infeasible nodes)
    static double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }
    void charge(double &slot) { slot += ms_since(tp); tp = Clock::now(); }
    // The node at position pos (level pos / B) was followed in place by a dive child at pos + B: it counts when its
    // LP was solved and it needs no strong-branching initialisation of its own (else it is dropped and queued like
    // any other child).  The decision taken after pos is dvar[pos].
    bool dived(int pos) const { return pos < S.dive * S.B && h.dvar[pos] >= 0 && h.status[pos + S.B] >= 0 && h.nprobe[pos + S.B] == 0; }
};

// The pool make_children writes its rows into: the node pool or the probe pool.
struct ChildDst { double *l, *u; int8_t *v; int32_t *ncut, *ids; };

// A branching list (step_layout::PairList) of `count` parents staged at dp, then make_children over it on `cs`: two
// children per parent, from the step's outputs and the parents' pool rows into rows `child` of dst.  hp: pinned
// staging, filled here and sent as one copy; null: four copies straight from the vectors.
int launch_children(mipx_tree *t, StepBuf &S, hipStream_t cs, int count, const std::vector<int32_t> &slot,
                    const std::vector<int32_t> &pos, const std::vector<int32_t> &var, const std::vector<int32_t> &child,
                    int32_t *hp, int32_t *dp, const ChildDst &dst) {
    mipx_ctx *ctx = t->ctx;
    const step_layout::PairList lay((size_t)count);
    const size_t c4 = (size_t)count * 4;   // bytes of a list of one entry per parent
    const auto d = lay.view(dp);
    if (hp) {
        const auto s = lay.view(hp);
        std::memcpy(s.parent_slot, slot.data(), c4); std::memcpy(s.parent_pos, pos.data(), c4);
        std::memcpy(s.var, var.data(), c4); std::memcpy(s.child_slot, child.data(), 2 * c4);
        HIP_TRY(ctx, hipMemcpyAsync(dp, hp, lay.bytes(), hipMemcpyHostToDevice, cs));
    } else {
        HIP_TRY(ctx, hipMemcpyAsync(d.parent_slot, slot.data(), c4, hipMemcpyHostToDevice, cs));
        HIP_TRY(ctx, hipMemcpyAsync(d.parent_pos, pos.data(), c4, hipMemcpyHostToDevice, cs));
        HIP_TRY(ctx, hipMemcpyAsync(d.var, var.data(), c4, hipMemcpyHostToDevice, cs));
        HIP_TRY(ctx, hipMemcpyAsync(d.child_slot, child.data(), 2 * c4, hipMemcpyHostToDevice, cs));
    }
    mipx::ChildArgs ca;
    ca.n = t->n; ca.m = t->m;
    ca.src_l = t->pool_l; ca.src_u = t->pool_u; ca.x = S.d_x; ca.vstat = S.d_vout;
    ca.parent_slot = d.parent_slot; ca.parent_pos = d.parent_pos; ca.var = d.var; ca.child_slot = d.child_slot;
    ca.dst_l = dst.l; ca.dst_u = dst.u; ca.dst_v = dst.v;
    if (t->cuts) {  // a child has its parent's rows, cuts included (base_node.py:602-606)
        ca.mstride = t->mrows; ca.kc = t->kc;
        ca.src_ncut = S.w_ncut; ca.src_ids = S.w_ids; ca.dst_ncut = dst.ncut; ca.dst_ids = dst.ids;
    }
    enqueue_make_children(ca, count, cs);
    HIP_TRY(ctx, hipGetLastError());
    return MIPX_OK;
}

// Phase 1: wait for the batch, then everything the host reads per node.  done: the device finished the whole step.
int finish_collect(mipx_tree *t, FinishWork &W, bool &done) {
    mipx_ctx *ctx = t->ctx; StepBuf &S = W.S;
    const int B = S.B;
    int rc = MIPX_OK;
    done = false;
    if (t->cuts && (rc = tree_cut_rounds(t, S))) return rc;
    HIP_TRY(ctx, hipEventSynchronize(S.done));
    float kms = 0.f;
    if (hipEventElapsedTime(&kms, S.e0, S.e1) == hipSuccess) t->kernel_ms += kms;
    if (S.heur_n > 0 && (rc = heur_step_collect(t, S))) return rc;   // (primal heuristic: its incumbent prunes this step's nodes)
    if (S.fast) {
        mipx::FinishSummary *hs = (mipx::FinishSummary *)finish_block(t, 2 * (1 + (size_t)t->dive)).view(S.h_fin).summary;
        if ((rc = tree_d2h(t, hs, S.d_sum, sizeof(mipx::FinishSummary)))) return rc;
        if (!hs->host_path) {
            if ((rc = tree_finish_fast(t, S, *hs, W.todo))) return rc;
            if (W.todo.empty()) { done = true; return MIPX_OK; }
            W.partial = true;    // (the pack came with the lists)
        } else {
            // more probe requests than the compact list holds: the host finishes the whole step; its children's rows come back
            t->free_slots.insert(t->free_slots.end(), S.budget.begin(), S.budget.end());
            S.budget.clear();
        }
    }
    // one copy (pinned destination) for everything the host reads per node
    if (!W.partial && (rc = tree_d2h(t, S.h_pack, S.d_pack, S.pack.bytes()))) return rc;
    W.h = S.pack.view(S.h_pack);   // (laid out for the tree's dive depth: layout_pack)
    int32_t *status = W.h.status, *nprobe = W.h.nprobe;
    // bound propagation: a node it found infeasible is a node whose LP ended primal infeasible, whatever the LP on
    // its unchanged row returned -- no probes, no children, and its plunge children are dropped
    if (S.prop_n > 0) {
        if ((rc = prop_step_collect(t, S, W.prop_inf))) return rc;
        for (int k = 0; k < B; k++) {
            if (!W.prop_inf[(size_t)k]) continue;
            W.prop_asks += nprobe[k];
            status[k] = 1;
            nprobe[k] = 0;
            if (S.dive > 0) W.h.dvar[k] = -1;
        }
    }
    if (!W.partial) {
        for (int k = 0; k < B; k++)
            if (nprobe[k] == 0) W.todo.push_back(k);
        for (int k = 0; k < B; k++)
            if (nprobe[k] != 0) W.todo.push_back(k);
    }
    t->lps += (int64_t)W.todo.size();
    for (int k : W.todo) t->pivots += W.h.npiv[k];
    W.charge(t->phase_ms[1]);
    return MIPX_OK;
}

// Phase 2 (pseudo costs): the strong-branching probes the todo nodes asked for -- request list, probe records,
// truncated LPs, results.
int finish_probes(mipx_tree *t, FinishWork &W) {
    mipx_ctx *ctx = t->ctx; StepBuf &S = W.S;
    const int B = S.B, n = t->n;
    const int32_t *nprobe = W.h.nprobe;
    int rc = MIPX_OK;
    for (int k : W.todo) W.total += nprobe[k];
    auto request = [&](int pos, int var, double x) {   // one probe pair: under the node at pos, on var with value x
        W.pair_pos.push_back(pos); W.pair_slot.push_back(S.slots[pos]); W.pair_var.push_back(var); W.xrow.push_back(x);
    };
    // a step in flight on the main stream: the probes go to the side stream (K1b streams slabs of its own there)
    hipStream_t ps = W.overlapped ? t->st2 : ctx->stream;
    if (W.total > 0) {
        if (2 * W.total > t->probe_cap) return fail(ctx, MIPX_ENOMEM, "tree: probe pool exhausted");
        // The probe requests came with the packed read-back (K4 writes one compact entry per request); only a step
        // with more than kAskCap of them -- the ramp-up -- reads the per-node lists and solutions in bulk.
        const int32_t asked = *W.h.ask_count;
        if (asked == W.total + W.prop_asks && asked <= kAskCap) {
            const Ask *ask = (const Ask *)W.h.ask;
            std::vector<Ask> es(ask, ask + asked);
            std::sort(es.begin(), es.end(), [](const Ask &a, const Ask &b) { return a.node < b.node || (a.node == b.node && a.k < b.k); });
            for (const Ask &e : es)
                if (W.prop_inf.empty() || !W.prop_inf[(size_t)e.node]) request(e.node, t->int_idx[e.k], e.x);
        } else {
            std::vector<double> xall((size_t)B * n);
            std::vector<int32_t> plist((size_t)B * t->n_int);
            HIP_TRY(ctx, hipMemcpy(plist.data(), S.d_plist, plist.size() * 4, hipMemcpyDeviceToHost));
            HIP_TRY(ctx, hipMemcpy(xall.data(), S.d_x, xall.size() * 8, hipMemcpyDeviceToHost));
            for (int k = 0; k < B; k++) {
                const double *xk = xall.data() + (size_t)k * n;
                for (int e = 0; e < nprobe[k]; e++) {
                    const int var = t->int_idx[plist[(size_t)k * t->n_int + e]];
                    request(k, var, xk[var]);
                }
            }
        }
        auto tq = FinishWork::Clock::now();
        t->probe_ms[0] += FinishWork::ms_since(W.tp);
        const int P = (int)W.pair_pos.size();
        std::vector<int32_t> child_slot(2 * (size_t)P);
        for (int c = 0; c < 2 * P; c++) child_slot[c] = c;
        // (on the side stream when a step is in flight: the probes run beside its node LPs)
        if ((rc = launch_children(t, S, ps, P, W.pair_slot, W.pair_pos, W.pair_var, child_slot, nullptr,
                                  W.overlapped ? t->d_pairs2 : t->d_pairs, {t->pp_l, t->pp_u, t->pp_v, t->pp_ncut, t->pp_ids})))
            return rc;
        CutLaunch pcl;
        if (t->cuts) {  // a probe has its parent's rows
            const CutState cs((size_t)t->max_batch);
            int maxc = 0;
            for (int k = 0; k < B; k++) maxc = std::max(maxc, (int)*cs.field(S.h_cs, CutState::kRowsAfter, (size_t)k));
            pcl.ncut = t->pp_ncut; pcl.ids = t->pp_ids; pcl.m_rows = t->m + maxc;
        }
        // truncated dual simplex on every probe (base_node.py:645-646)
        if ((rc = launch_lp(t, 2 * P, t->pp_l, t->pp_u, t->pp_v, nullptr, t->sb_iters, t->pp_status, t->pp_obj, nullptr, nullptr,
                            nullptr, nullptr, ps, nullptr, nullptr, t->cuts ? &pcl : nullptr)))
            return rc;
        W.pst.resize(2 * (size_t)P); W.pobj.resize(2 * (size_t)P);
        t->probe_ms[1] += FinishWork::ms_since(tq); tq = FinishWork::Clock::now();
        HIP_TRY(ctx, hipStreamSynchronize(ps));
        t->probe_ms[2] += FinishWork::ms_since(tq); tq = FinishWork::Clock::now();
        HIP_TRY(ctx, hipMemcpyAsync(t->h_pres, t->pp_obj, W.pobj.size() * 8, hipMemcpyDeviceToHost, t->st2));
        if ((rc = tree_d2h(t, t->h_pres + (size_t)t->probe_cap * 8, t->pp_status, W.pst.size() * 4))) return rc;
        std::memcpy(W.pobj.data(), t->h_pres, W.pobj.size() * 8);
        std::memcpy(W.pst.data(), t->h_pres + (size_t)t->probe_cap * 8, W.pst.size() * 4);
        t->probe_ms[3] += FinishWork::ms_since(tq);
        t->probes += 2 * P;
    }
    W.charge(t->phase_ms[5]);
    return MIPX_OK;
}

// Phase 3 (pseudo costs): the table updates in the reference's order, the late samples to the device table, and
// the re-scoring of the step with the updated table.
int finish_table(mipx_tree *t, FinishWork &W) {
    mipx_ctx *ctx = t->ctx; StepBuf &S = W.S;
    const int B = S.B, n = t->n;
    const double inf = std::numeric_limits<double>::infinity();
    const auto &h = W.h;
    const int32_t *status = h.status, *nprobe = h.nprobe; const double *obj = h.obj;
    int rc = MIPX_OK;
    // node by node; per node its probes (ascending integer index, left then right), then its own branch unless just initialised
    size_t e = 0;
    bool changed = false;
    const double cut = tree_cutoff(t);
    for (int k : W.todo) {   // (the requests are sorted by node: the nodes with requests come in that order)
        if (!(status[k] == 0 || status[k] == 2)) continue;   // (not lp_feasible)
        const NodeRec &nd = S.recs[k];
        bool own_probed = false;
        for (int q = 0; q < nprobe[k]; q++, e++) {
            const int var = W.pair_var[e];
            const double bv = W.xrow[e];
            pc_update(t, var, 0, W.pst[2 * e], W.pobj[2 * e], obj[k], bv - std::floor(bv));
            pc_update(t, var, 1, W.pst[2 * e + 1], W.pobj[2 * e + 1], obj[k], std::ceil(bv) - bv);
            if (var == nd.b_idx) own_probed = true;
            changed = true;
        }
        // (a seed of a restart inherits no bound: its parent was not solved at this right-hand side)
        if (nd.b_idx >= 0 && !own_probed && !(t->rs.on && nd.dual_bound == -inf)) {
            // variable_change: b_val - u[b_idx] (left) or l[b_idx] - b_val (right)
            const double vc = nd.b_dir == 0 ? nd.b_val - std::floor(nd.b_val) : std::ceil(nd.b_val) - nd.b_val;
            pc_update(t, nd.b_idx, nd.b_dir, status[k], obj[k], nd.dual_bound, vc);
            changed = true;
        }
        // the dive child: the update for the branch that made it -- like any node only if its own LP is feasible
        // (pseudo_cost.py:42-43), and only where the evaluation will accept the dive (the reference never creates that
        // child under a pruned or integral parent); a plunge: level by level, each child under the node before it
        for (int pos = k; W.dived(pos) && obj[pos] < cut && !h.mipf[pos] && (status[pos] == 0 || status[pos] == 2); pos += B) {
            const int cp = pos + B;
            if (!(status[cp] == 0 || status[cp] == 2)) break;
            const double vc = h.ddir[pos] == 0 ? h.dval[pos] - std::floor(h.dval[pos]) : std::ceil(h.dval[pos]) - h.dval[pos];
            pc_update(t, h.dvar[pos], h.ddir[pos], status[cp], obj[cp], obj[pos], vc);
            changed = true;
        }
    }
    if (changed && !t->fast_ok) t->table_dirty = true;   // (device finish: the samples go to the device table below)
    W.charge(t->phase_ms[6]);
    if (t->fast_ok && !t->pend_samples.empty()) {
        // the device holds the table: this step's samples reach it in the order they were applied here
        const size_t cnt = t->pend_samples.size();
        if (cnt > t->samples_cap) return fail(ctx, MIPX_ENOMEM, "tree: more pseudo-cost samples than the staging holds");
        std::memcpy(S.h_samples, t->pend_samples.data(), cnt * sizeof(mipx::PcSample));
        int32_t *hk = (int32_t *)(S.h_samples + t->samples_cap);   // (the keys again, densely, behind the samples)
        for (size_t q = 0; q < cnt; q++) hk[q] = t->pend_samples[q].var_dir;
        t->pend_samples.clear();
        HIP_TRY(ctx, hipMemcpyAsync(S.d_skeys, hk, cnt * 4, hipMemcpyHostToDevice, t->stf));
        // (onto the version at the tail of stf's queue: every later version is copied from it)
        HIP_TRY(ctx, hipMemcpyAsync(S.d_samples, S.h_samples, cnt * sizeof(mipx::PcSample), hipMemcpyHostToDevice, t->stf));
        const TabPtr tb = tab_at(t, t->tab_tail);
        mipx::PcApplyArgs pa;
        pa.n = n; pa.sum = nullptr; pa.count = (int)cnt; pa.samples = S.d_samples; pa.keys = S.d_skeys;
        pa.cost_l = tb.cl; pa.cost_r = tb.cr; pa.has = tb.has; pa.times = tb.times; pa.own = tb.own;
        hipLaunchKernelGGL(mipx::pc_apply, dim3(2 * n), dim3(64), 0, t->stf, pa);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipEventRecord(t->ev_tab[t->tab_tail], t->stf));
        t->tab_late[t->tab_tail] = true;
    }
    if (t->fast_ok) t->tab_host = S.fast ? S.tabv : t->tab_tail;
    // re-score with the updated table: always in the sequential mode (the reference branches with the table its own
    // node just updated); when steps overlap, only if probes created entries that the first scoring had to leave out
    if (changed && (!W.overlapped || W.total > 0)) {
        // (device finish: the re-scoring reads copies of the host's snapshot + this step's updates, the device table
        // itself only ever changes through pc_apply)
        const bool use_side = W.overlapped, side_tab = use_side || t->fast_ok;
        hipStream_t ps = use_side ? t->st2 : ctx->stream;
        const int NB = (S.dive + 1) * B;  // output positions in use: the batch, then its dive children level by level
        double *cl = side_tab ? t->d_cost_l2 : t->d_cost_l, *cr = side_tab ? t->d_cost_r2 : t->d_cost_r;
        uint8_t *ch = side_tab ? t->d_has2 : t->d_has;
        HIP_TRY(ctx, hipMemcpyAsync(cl, t->cost_l.data(), (size_t)n * 8, hipMemcpyHostToDevice, ps));
        HIP_TRY(ctx, hipMemcpyAsync(cr, t->cost_r.data(), (size_t)n * 8, hipMemcpyHostToDevice, ps));
        HIP_TRY(ctx, hipMemcpyAsync(ch, t->has_entry.data(), (size_t)n, hipMemcpyHostToDevice, ps));
        if (!side_tab) t->table_dirty = false;
        if ((rc = launch_score(t, S, NB, side_tab, false, use_side ? 1 : 0))) return rc;
        HIP_TRY(ctx, hipStreamSynchronize(ps));
        if (!W.overlapped) {   // sequential mode: every node branches with the table its step just updated
            if ((rc = tree_d2h(t, h.bidx, S.d.bidx, (size_t)NB * 4))) return rc;
            if ((rc = tree_d2h(t, h.bval, S.d.bval, (size_t)NB * 8))) return rc;
        } else {
            // batches: only the nodes whose probes created the entries their first scoring had to leave out take the new
            // choice; a node that asked for nothing branches as it was scored at the launch (what the device finish does)
            std::vector<int32_t> nb((size_t)B);
            std::vector<double> nvv((size_t)B);
            if ((rc = tree_d2h(t, nb.data(), S.d.bidx, (size_t)B * 4))) return rc;
            if ((rc = tree_d2h(t, nvv.data(), S.d.bval, (size_t)B * 8))) return rc;
            for (int k : W.todo)
                if (nprobe[k] > 0) { h.bidx[k] = nb[(size_t)k]; h.bval[k] = nvv[(size_t)k]; }
        }
    }
    return MIPX_OK;
}

// One evaluated node at output position pos: the reference's _evaluate_node bookkeeping.  level 0: a node of the batch
// (pool row `slot`); level p: a dive child.  Returns the id of the child that was solved in place by the dive (to be
// evaluated next), or -1.  (Best first on the bucket queue: the step's pushes are collected in t->pend, queued together.)
int64_t evaluate_node(mipx_tree *t, FinishWork &W, int64_t id, int pos, int32_t slot, int level, int depth, int32_t anchor, int &err) {
    StepBuf &S = W.S;
    const auto &h = W.h;
    const int32_t *status = h.status; const double *obj = h.obj;
    const double inf = std::numeric_limits<double>::infinity();
    const bool rec = t->df.on, trec = t->tr.on, defer_push = t->use_bq && t->search == 0;
    const CutState cs((size_t)t->max_batch);
    t->evaluated++;
    if (rec && status[pos] == 0) W.df_recs.push_back({pos, slot, id});
    if (rec && status[pos] == 1) W.df_infs.push_back({pos, slot, id});
    if (trec) t->tr.solved(id, status[pos], obj[pos], h.mipf[pos] != 0, h.nprobe[pos] > 0);
    const bool lp_feasible = status[pos] == 0 || status[pos] == 2;
    if (status[pos] == 2) t->unbounded = true;
    int branched_on = -1;
    int64_t dive_child = -1;
    double leaf_value = lp_feasible ? obj[pos] : inf;
    if (lp_feasible && obj[pos] < t->primal) {
        const bool take_dive = W.dived(pos);
        const int bvar = take_dive ? h.dvar[pos] : h.bidx[pos];  // a dive has already branched
        if (h.mipf[pos]) {
            t->primal = obj[pos];
            W.incumbent_pos = pos;
        } else if (!(obj[pos] < tree_cutoff(t))) {
            // (only with an objective step: the node holds nothing below the incumbent, a leaf of that value)
            leaf_value = t->primal;
            t->os.unbranched++;
        } else if (bvar >= 0) {
            if (t->free_slots.size() < 2) { err = fail(t->ctx, MIPX_ENOMEM, "tree: node pool exhausted"); return -1; }
            branched_on = bvar;
            const double xv = take_dive ? h.dval[pos] : h.bval[pos];
            for (int dir = 0; dir < 2; dir++) {
                NodeRec c;
                c.dual_bound = obj[pos];
                c.depth = depth + 1;
                c.key = t->search == 0 ? c.dual_bound : -(double)c.depth;
                c.b_idx = branched_on; c.b_dir = dir; c.b_val = xv;
                c.born = (int32_t)t->steps;
                c.anchor = anchor;
                c.ncut = t->cuts ? *cs.field(S.h_cs, CutState::kRowsAfter, (size_t)pos) : 0;   // the rows of its parent, cuts included
                c.slot = t->free_slots.back();
                t->free_slots.pop_back();
                S.br[(size_t)level].child.push_back(c.slot);
#ifdef MIPX_HOSTPROF
                const unsigned long long r0_ = __rdtsc();
#endif
                t->nodes.push_back(c);
#ifdef MIPX_HOSTPROF
                g_hp_rec += __rdtsc() - r0_;
#endif
                const int64_t cid = (int64_t)t->nodes.size() - 1;
                if (rec) {
                    t->df.parent.push_back(id); t->df.rec.push_back(-1); t->df.haschild.push_back(0);
                    t->df.haschild[(size_t)id] = 1;
                }
                if (trec) t->tr.child(id);
                if (take_dive && dir == h.ddir[pos]) dive_child = cid;  // already solved: never enters the queue
                else if (defer_push) t->pend.push_back({c.key, cid});
                else tree_push(t, cid);
            }
            S.br[(size_t)level].pos.push_back(pos);
            S.br[(size_t)level].slot.push_back(slot);
            S.br[(size_t)level].var.push_back(branched_on);
            leaf_value = inf;  // no longer a leaf
        }
    }
    if (branched_on < 0) t->closed_min = std::fmin(t->closed_min, leaf_value);
    if (t->trace) {
        t->tr_id.push_back(id); t->tr_status.push_back(status[pos]);
        t->tr_bidx.push_back(branched_on); t->tr_obj.push_back(obj[pos]);
        if (t->cuts)   // (the node's cut-round counters, in the order of the trace)
            for (int f = 0; f <= CutState::kRowsAfter; f++) t->tr_cuts.push_back(*cs.field(S.h_cs, f, (size_t)pos));
    }
    return dive_child;
}

// Phase 4: the todo nodes evaluated one by one (a dive child right after its parent: it was solved in the same
// workgroup), their children into the node table and the queue, the incumbent.
int finish_evaluate(mipx_tree *t, FinishWork &W) {
    StepBuf &S = W.S; const auto &h = W.h;
    const int B = S.B, L = t->dive + 1;
    if ((int)S.br.size() < L) S.br.resize((size_t)L);
    for (auto &bl : S.br) { bl.pos.clear(); bl.slot.clear(); bl.var.clear(); bl.child.clear(); }
    S.dive_slots.clear();
    const bool defer_push = t->use_bq && t->search == 0;
    t->pend.clear();
    for (int k : W.todo) {
        int err = MIPX_OK;
        // (a chain reads ten result arrays at every level: more streams than the hardware prefetcher follows)
        if (!W.partial && (k & 7) == 0 && k + 40 < B) {
            for (int lv = 0; lv <= S.dive; lv++) {
                const int pp = lv * B + k + 32;
                __builtin_prefetch(&h.status[pp]); __builtin_prefetch(&h.obj[pp]); __builtin_prefetch(&h.mipf[pp]);
                __builtin_prefetch(&h.bidx[pp]); __builtin_prefetch(&h.bval[pp]); __builtin_prefetch(&h.nprobe[pp]);
                __builtin_prefetch(&h.npiv[pp]);
                if (lv < S.dive) { __builtin_prefetch(&h.dvar[pp]); __builtin_prefetch(&h.ddir[pp]); __builtin_prefetch(&h.dval[pp]); }
            }
        }
        int64_t cid = evaluate_node(t, W, S.ids[k], k, S.slots[k], 0, S.recs[k].depth, S.recs[k].anchor, err);
        if (err) { if (defer_push) t->bq.push_many(t->pend.data(), t->pend.size()); return err; }
        for (int level = 1; cid >= 0; level++) {   // the plunge: every dive child right after its parent
            const int32_t cslot = t->nodes[cid].slot;
            const int pos = level * B + k;
            t->lps++; t->dives++;
            t->pivots += h.npiv[pos];
            const int64_t next = evaluate_node(t, W, cid, pos, cslot, level, S.recs[k].depth + level, S.recs[k].anchor, err);
            if (err) { if (defer_push) t->bq.push_many(t->pend.data(), t->pend.size()); return err; }
            S.dive_slots.push_back(cslot);  // its record row feeds its own children (finish_children)
            t->nodes[cid].slot = -1;
            cid = next;
        }
    }
    if (defer_push) t->bq.push_many(t->pend.data(), t->pend.size());
    if (W.incumbent_pos >= 0) {   // the last improving node of the batch holds the incumbent
        const int rc = tree_d2h(t, t->best_x.data(), S.d_x + (size_t)W.incumbent_pos * t->n, (size_t)t->n * 8);
        if (rc) return rc;
        t->have_x = true;
    }
    W.charge(t->phase_ms[3]);
    return MIPX_OK;
}

// Phase 5: the root's basis where a later solve starts from it, the children records on the device, the dual
// function's records, then the evaluated nodes' rows are free again.
int finish_children(mipx_tree *t, FinishWork &W) {
    mipx_ctx *ctx = t->ctx; StepBuf &S = W.S;
    hipStream_t st = ctx->stream;
    const int nv = t->n + t->m, L = t->dive + 1;
    const bool root_solved = S.ids[0] == 0 && W.h.status[0] == 0;
    int rc = MIPX_OK;
    // anchor mode: the refactorisations of every later node start from the root's optimal tableau
    // (cut rounds: only a root that kept no cut rows has a basis of the shared rows alone)
    if (t->anchor_mode && !t->anchor_set && root_solved && (!W.partial || W.todo[0] == 0) &&
        !(t->cuts && *CutState((size_t)t->max_batch).field(S.h_cs, CutState::kRowsAfter) != 0)) {
        std::vector<int8_t> rootv(nv);
        HIP_TRY(ctx, hipMemcpy(rootv.data(), S.d_vout, (size_t)nv, hipMemcpyDeviceToHost));
        if ((rc = mipx_problem_set_anchor(t->prob, rootv.data()))) return rc;
        t->anchor_set = true;
    }
    // tree record: the root's optimal basis codes, once (the warm start of mipx_tree_node_solve)
    if (t->tr.on && !t->tr.have_root && root_solved) {
        t->tr.root_v.resize(nv);
        if ((rc = tree_d2h(t, t->tr.root_v.data(), S.d_vout, (size_t)nv))) return rc;
        t->tr.have_root = true;
    }
    // when steps overlap the records are written on their own stream, beside the node LPs of the step in flight
    // (fresh pool rows only); the next launch waits for it
    hipStream_t cs = W.overlapped ? t->st3 : st;
    if (!S.br[0].pos.empty()) {
        if (W.overlapped) HIP_TRY(ctx, hipStreamSynchronize(t->st3));  // h_pairs / d_pairs free again
        // reduced-cost tightening: with an incumbent, every level's parents are tightened in place in front of the
        // launch that copies their rows into their children (level p's parents: the rows level p - 1 just wrote)
        const bool tighten = t->rc.on && std::isfinite(t->primal);
        if (tighten && ((rc = rc_step_collect(t, S)) || (rc = rc_step_stage(t, S, cs, L)))) return rc;
        // level by level on one stream: the record of a dive child exists before its children are derived
        const size_t part = step_layout::PairList((size_t)t->max_batch).bytes() / 4;  // staging per level
        for (int level = 0; level < L; level++) {
            const auto &bl = S.br[(size_t)level];
            if (bl.pos.empty()) break;   // (no branching at this level: none below it either)
            if (tighten && (rc = rc_level_launch(t, S, cs, level, (int)bl.pos.size()))) return rc;
            if ((rc = launch_children(t, S, cs, (int)bl.pos.size(), bl.slot, bl.pos, bl.var, bl.child, t->h_pairs + (size_t)level * part,
                                      t->d_pairs + (size_t)level * part, {t->pool_l, t->pool_u, t->pool_v, t->pool_ncut, t->pool_ids})))
                return rc;
        }
        if (W.overlapped) {
            HIP_TRY(ctx, hipEventRecord(t->ev_child, t->st3));
            t->child_pending = true; t->child_recorded = true;
        } else {
            HIP_TRY(ctx, hipStreamSynchronize(st));
            if (tighten && (rc = rc_step_collect(t, S))) return rc;
        }
    }
    if (t->df.on) {   // the step's records, behind its children records (the dive children's rows hold their bounds)
        if ((rc = df_step(t, S, cs, W.df_recs, W.df_infs))) return rc;
        if (W.overlapped && !(W.df_recs.empty() && W.df_infs.empty())) {
            HIP_TRY(ctx, hipEventRecord(t->ev_child, t->st3));   // (the next launch, and so the rows' reuse, waits)
            t->child_pending = true; t->child_recorded = true;
        }
    }
    for (int32_t sl : S.dive_slots) t->free_slots.push_back(sl);
    for (int k : W.todo) t->free_slots.push_back(S.slots[k]);
    W.charge(t->phase_ms[4]);
    return MIPX_OK;
}

// Second half: wait for that batch only, then the reference's bookkeeping and the children.
int tree_finish(mipx_tree *t, StepBuf &S, bool overlapped) {
    FinishWork W{S, overlapped};
    if (!S.in_flight || S.B == 0) return MIPX_OK;
    S.in_flight = false;
    int rc = MIPX_OK; bool done = false;
    if ((rc = finish_collect(t, W, done)) || done) return rc;
    // pseudo costs: strong-branch initialisation + the update for the branch that made the node
    if (t->rule == 1 && ((rc = finish_probes(t, W)) || (rc = finish_table(t, W)))) return rc;
    W.charge(t->phase_ms[2]);
    if ((rc = finish_evaluate(t, W))) return rc;
    return finish_children(t, W);
}

// ---- the exchange between the ranks of one search (mipx_tree_set_comm) --------------------------------
constexpr int kRecHead = 16;         // doubles in front of a record's solution and pseudo-cost samples
constexpr int64_t kMaxMigrate = 4096;  // node records per donation
// cut rows per donation (cut migration): the table of one message is at most 2^14 rows of n + 1 f64,
// 33.7 MB at n = 256 (mipx_cutmig.h)
constexpr int64_t kMaxMigrateCuts = (int64_t)1 << 14;

size_t x_rec_len(const mipx_tree *t) { return (size_t)kRecHead + 5 * (size_t)t->n; }

int64_t tree_open_count(const mipx_tree *t) { return (int64_t)(t->use_bq ? t->bq.size() : t->heap.size()); }

// this rank's state as one record: [primal, dual, open + in flight, stop flag, evaluated, lps, probes,
// pivots (since sharding), has_x, round, frontier batch, ...] [x (n)] [own pseudo-cost samples (4 n)]
void x_fill_record(mipx_tree *t) {
    const size_t n = (size_t)t->n;
    std::vector<double> &r = t->x_rec;
    r.assign(x_rec_len(t), 0.0);
    int64_t inflight = 0;
    // the nodes popped into the steps in flight are neither queued nor closed: their bounds (the lowest
    // of the shard under best first) count, or the shard would report a dual bound it has not proved
    double inflight_min = std::numeric_limits<double>::infinity();
    for (const StepBuf &S : t->buf)
        if (S.in_flight) { inflight += S.B; inflight_min = std::fmin(inflight_min, S.inflight_min); }
    r[0] = t->primal;
    r[1] = std::fmin(tree_dual_bound(t), inflight_min);
    r[2] = (double)(tree_open_count(t) + inflight);
    r[3] = (double)t->x_stop_flag;
    r[4] = (double)(t->evaluated - t->ramp[0]);
    r[5] = (double)(t->lps - t->ramp[1]);
    r[6] = (double)(t->probes - t->ramp[2]);
    r[7] = (double)(t->pivots - t->ramp[3]);
    r[8] = t->have_x ? 1.0 : 0.0;
    r[9] = (double)t->x_rounds;
    r[10] = (double)t->x_batch;
    // pool rows this rank can take from a donor: what is free beyond the children the steps in flight
    // (up to three) and the steps until the record is applied may still claim
    {
        const int64_t per = 2 * (1 + (int64_t)t->dive) * (int64_t)t->max_batch;
        const int64_t room = (int64_t)t->free_slots.size() - (3 + (int64_t)t->x_every) * per;
        r[11] = (double)(room > 0 ? room : 0);
    }
    r[12] = inflight_min;
    if (t->cuts) {   // (zero in a tree without cut rounds)
        r[13] = t->cm_rows > 0 ? (double)(t->cm_rows - t->cm_used) : 0.0;   // migration region rows still free
        r[14] = t->cm_rows > 0 ? (double)t->kc : 0.0;
        r[15] = 1.0;
    }
    if (t->have_x) std::memcpy(r.data() + kRecHead, t->best_x.data(), n * 8);
    if (t->rule == 1 && t->fast_ok) {
        // A record never takes back a sample (mipx.h, the pseudo-cost merge).  Under the device finish with steps
        // overlapped pc_own is a snapshot of the table version of the step finished last, and the samples of the
        // nodes the host finished for the step before (deferred strong-branching probes) reach the version at the
        // tail of the ring: for one step the snapshot lacks them.  Per entry the pair with the highest times is
        // posted; the tail lineage holds every sample, so the posted pair is caught up with one step later.
        if (t->pc_posted.size() != 4 * n) t->pc_posted.assign(4 * n, 0.0);
        for (size_t e = 0; e < 2 * n; e++)
            if (t->pc_own[2 * n + e] > t->pc_posted[2 * n + e]) {
                t->pc_posted[e] = t->pc_own[e];
                t->pc_posted[2 * n + e] = t->pc_own[2 * n + e];
            }
        std::memcpy(r.data() + kRecHead + n, t->pc_posted.data(), 4 * n * 8);
    } else {
        std::memcpy(r.data() + kRecHead + n, t->pc_own.data(), 4 * n * 8);
    }
}

// A donation: `amount` node records from rank `from` to rank `to` (decided from the same records on
// every rank).  The donor gives every second of its best 2 * amount open nodes, so that both keep
// good ones; fewer if it has consumed them since it posted (the message has the planned size, a
// count in front says how many records are real).
//
// With cut rounds (cut migration on at both ends) the message also carries each record's cut list as refs
// into a table of the cut rows themselves, every store id once; ctab, the table's planned rows, is computed
// by both ends from the same records (mig_table_rows).  Layout:
//   [amount rows: l, u (n f64 each), basis codes (nvs int8, padded to 8)]
//   cut mode: [amount x (1 + kc) int32: ncut, refs into the table, list order] (padded to 8)
//             [ctab x n f64: pi] [ctab f64: pi0]
//   [meta f64: count, then 5 per record (dual bound, b_val, depth, b_idx, b_dir); cut mode: 6 (+ ncut) and,
//    after the records, the table rows used]
// and behind the message the scratch of the kernels: the pool rows (amount int32), in cut mode the store ids
// of the table rows (ctab int32) and a flag.
struct MigLayout {
    size_t rowbytes, meta_off, bytes;
    size_t refs_off = 0, tab_off = 0, nmeta = 0, scratch = 0;
    int64_t ctab = 0;
    int kc = 0;   // > 0: cut mode
};
size_t pad8(size_t b) { return (b + 7) / 8 * 8; }
MigLayout mig_layout(const mipx_tree *t, int64_t amount, int64_t ctab = 0) {
    const size_t n = (size_t)t->n, nvs = n + (size_t)t->mrows;
    MigLayout L;
    L.rowbytes = 16 * n + (nvs + 7) / 8 * 8;
    if (!t->cuts) {
        L.meta_off = (size_t)amount * L.rowbytes;
        L.nmeta = 1 + 5 * (size_t)amount;
        L.bytes = L.meta_off + L.nmeta * 8;
        L.scratch = (size_t)amount * 4;
        return L;
    }
    L.kc = t->kc;
    L.ctab = ctab;
    L.refs_off = (size_t)amount * L.rowbytes;
    L.tab_off = L.refs_off + pad8((size_t)amount * (1 + (size_t)L.kc) * 4);
    L.meta_off = L.tab_off + (size_t)ctab * (n + 1) * 8;
    L.nmeta = 1 + 6 * (size_t)amount + 1;
    L.bytes = L.meta_off + L.nmeta * 8;
    L.scratch = pad8((size_t)amount * 4) + pad8((size_t)ctab * 4) + 8;
    return L;
}
// the table rows of a donation: what the receiver's region can still take ([13] of its record), at most
// kMaxMigrateCuts, and never more than the records can refer to
int64_t mig_table_rows(double region_free, int64_t amount, int kc) {
    int64_t c = std::min<int64_t>((int64_t)region_free, kMaxMigrateCuts);
    c = std::min<int64_t>(c, amount * (int64_t)kc);
    return c > 0 ? c : 0;
}
mipx::PackArgs mig_args(mipx_tree *t, const MigLayout &L, char *msg, int32_t *d_slots) {
    mipx::PackArgs pa;
    pa.n = t->n; pa.nvs = t->n + t->mrows; pa.rowbytes = L.rowbytes; pa.slot = d_slots;
    pa.pool_l = t->pool_l; pa.pool_u = t->pool_u; pa.pool_v = t->pool_v; pa.msg = msg;
    pa.count = 0;
    return pa;
}

// donor half: up to `amount` records leave the queue and are packed into msg (device memory)
int mig_pack(mipx_tree *t, const MigLayout &L, char *msg, int32_t *d_slots, int64_t amount, std::vector<int32_t> &slots,
             int64_t *count) {
    mipx_ctx *ctx = t->ctx;
    std::vector<double> meta(1 + 5 * (size_t)amount, 0.0);
    mipx::PackArgs pa = mig_args(t, L, msg, d_slots);
    // the child records of the last finished step may still be in the making on st3: the donor must not
    // pack rows before they are written
    if (t->child_recorded) HIP_TRY(ctx, hipStreamWaitEvent(t->st2, t->ev_child, 0));
    const int64_t have = tree_open_count(t);
    const int64_t give = std::max<int64_t>(0, std::min<int64_t>(amount, (have - t->x_batch) / 2));
    std::vector<int64_t> ids;
    if (t->use_bq) {
        t->popped.clear();
        t->bq.pop_batch((size_t)(2 * give), t->popped);
        for (const auto &it : t->popped) ids.push_back(it.id);
    } else {
        for (int64_t k = 0; k < 2 * give && !t->heap.empty(); k++) ids.push_back(t->heap.pop());
    }
    int64_t cnt = 0;
    for (size_t k = 0; k < ids.size(); k++) {
        NodeRec &nd = t->nodes[ids[k]];
        if (t->search != 0) t->is_open[ids[k]] = 0;
        if ((k & 1) == 0 || cnt >= give) { tree_push(t, ids[k]); continue; }   // kept
        double *mrec = meta.data() + 1 + 5 * cnt;
        mrec[0] = nd.dual_bound; mrec[1] = nd.b_val; mrec[2] = (double)nd.depth;
        mrec[3] = (double)nd.b_idx; mrec[4] = (double)nd.b_dir;
        slots.push_back(nd.slot);
        nd.slot = -1;
        cnt++;
    }
    meta[0] = (double)cnt;
    if (cnt > 0) {
        HIP_TRY(ctx, hipMemcpyAsync(d_slots, slots.data(), (size_t)cnt * 4, hipMemcpyHostToDevice, t->st2));
        enqueue_pack_nodes(pa, (int)cnt, t->st2);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipMemcpyAsync(msg + L.meta_off, meta.data(), meta.size() * 8, hipMemcpyHostToDevice, t->st2));
    HIP_TRY(ctx, hipStreamSynchronize(t->st2));
    *count = cnt;
    return MIPX_OK;
}

// receiver half: the records of msg (device memory) get pool rows and join the queue
int mig_unpack(mipx_tree *t, const MigLayout &L, char *msg, int32_t *d_slots, int64_t amount, int64_t *count) {
    mipx_ctx *ctx = t->ctx;
    std::vector<double> meta(1 + 5 * (size_t)amount, 0.0);
    std::vector<int32_t> slots;
    mipx::PackArgs pa = mig_args(t, L, msg, d_slots);
    HIP_TRY(ctx, hipMemcpy(meta.data(), msg + L.meta_off, meta.size() * 8, hipMemcpyDeviceToHost));
    const int64_t cnt = (int64_t)meta[0];
    if (cnt < 0 || cnt > amount) return fail(ctx, MIPX_EHIP, "tree: corrupt migration message");
    // (the amount was capped by the room this rank reported in its record -- x_decide -- which left the
    // claims of the steps in flight aside; batch_size() keeps later steps within what is left)
    if ((int64_t)t->free_slots.size() < cnt)
        return fail(ctx, MIPX_ENOMEM, "tree: node pool too small for the migrated nodes (raise pool_capacity)");
    // the parents' rows freed by the last finished step may still be read by its make_children on st3
    if (t->child_recorded) HIP_TRY(ctx, hipStreamWaitEvent(t->st2, t->ev_child, 0));
    for (int64_t k = 0; k < cnt; k++) {
        const double *mrec = meta.data() + 1 + 5 * k;
        NodeRec nd;
        nd.dual_bound = mrec[0]; nd.b_val = mrec[1]; nd.depth = (int32_t)mrec[2];
        nd.b_idx = (int32_t)mrec[3]; nd.b_dir = (int32_t)mrec[4];
        nd.key = t->search == 0 ? nd.dual_bound : -(double)nd.depth;
        nd.anchor = -1; nd.born = (int32_t)t->steps; nd.ncut = 0;
        nd.slot = t->free_slots.back();
        t->free_slots.pop_back();
        slots.push_back(nd.slot);
        t->nodes.push_back(nd);
        tree_push(t, (int64_t)t->nodes.size() - 1);
    }
    if (cnt > 0) {
        HIP_TRY(ctx, hipMemcpyAsync(d_slots, slots.data(), (size_t)cnt * 4, hipMemcpyHostToDevice, t->st2));
        enqueue_unpack_nodes(pa, (int)cnt, t->st2);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipStreamSynchronize(t->st2));
    }
    *count = cnt;
    return MIPX_OK;
}

// Cut mode (mipx_tree_set_cut_migration).  scratch: the kernels' scratch behind the message (MigLayout).
int32_t *mig_src(int32_t *scratch, int64_t amount) { return (int32_t *)((char *)scratch + pad8((size_t)amount * 4)); }
int32_t *mig_bad(const MigLayout &L, int32_t *scratch, int64_t amount) {
    return (int32_t *)((char *)mig_src(scratch, amount) + pad8((size_t)L.ctab * 4));
}

// donor half, cut mode: the candidates are chosen as in mig_pack; their cut lists come to the host, and in
// candidate order a node travels if the distinct store ids it adds to the table still fit in L.ctab rows
// (a node without cut rows always does), else it is kept and goes back into the queue
int mig_pack_cuts(mipx_tree *t, const MigLayout &L, char *msg, int32_t *scratch, int64_t amount,
                  std::vector<int32_t> &slots, int64_t *count, int64_t *table_rows) {
    mipx_ctx *ctx = t->ctx;
    const int K = L.kc;
    const size_t W = 1 + (size_t)K;
    std::vector<double> meta(L.nmeta, 0.0);
    if (t->child_recorded) HIP_TRY(ctx, hipStreamWaitEvent(t->st2, t->ev_child, 0));
    const int64_t have = tree_open_count(t);
    const int64_t give = std::max<int64_t>(0, std::min<int64_t>(amount, (have - t->x_batch) / 2));
    std::vector<int64_t> ids, cand;
    if (t->use_bq) {
        t->popped.clear();
        t->bq.pop_batch((size_t)(2 * give), t->popped);
        for (const auto &it : t->popped) ids.push_back(it.id);
    } else {
        for (int64_t k = 0; k < 2 * give && !t->heap.empty(); k++) ids.push_back(t->heap.pop());
    }
    for (size_t k = 0; k < ids.size(); k++) {
        if (t->search != 0) t->is_open[ids[k]] = 0;
        if ((k & 1) == 0 || (int64_t)cand.size() >= give) tree_push(t, ids[k]);   // kept
        else cand.push_back(ids[k]);
    }
    // the candidates' cut lists, staged in the message's refs section
    int32_t *d_lists = (int32_t *)(msg + L.refs_off);
    std::vector<int32_t> lists(cand.size() * W);
    if (!cand.empty()) {
        for (int64_t id : cand) slots.push_back(t->nodes[id].slot);
        HIP_TRY(ctx, hipMemcpyAsync(scratch, slots.data(), slots.size() * 4, hipMemcpyHostToDevice, t->st2));
        mipx::CutMigArgs ca;
        ca.kc = K; ca.slot = scratch; ca.pool_ncut = t->pool_ncut; ca.pool_ids = t->pool_ids;
        ca.lists = d_lists;
        enqueue_cutmig_lists(ca, (int)cand.size(), t->st2);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(lists.data(), d_lists, lists.size() * 4, hipMemcpyDeviceToHost, t->st2));
        HIP_TRY(ctx, hipStreamSynchronize(t->st2));
        slots.clear();
    }
    std::unordered_map<int32_t, int32_t> ref;   // store id -> table row
    std::vector<int32_t> src, refs;             // table rows' store ids; the records' [ncut, refs]
    int64_t cnt = 0, with_cuts = 0;
    for (size_t i = 0; i < cand.size(); i++) {
        const int32_t *li = lists.data() + i * W;
        const int nc = li[0];
        if (nc < 0 || nc > K) return fail(ctx, MIPX_EHIP, "tree: corrupt cut list in the node pool");
        int64_t fresh = 0;
        for (int j = 0; j < nc; j++) {
            if (li[1 + j] < 0 || li[1 + j] >= t->store_cap) return fail(ctx, MIPX_EHIP, "tree: corrupt cut list in the node pool");
            bool seen = ref.count(li[1 + j]) > 0;
            for (int q = 0; q < j && !seen; q++) seen = li[1 + q] == li[1 + j];
            fresh += seen ? 0 : 1;
        }
        if ((int64_t)src.size() + fresh > L.ctab) { tree_push(t, cand[i]); continue; }   // kept: its rows do not fit
        NodeRec &nd = t->nodes[cand[i]];
        refs.push_back(nc);
        for (int j = 0; j < nc; j++) {
            auto it = ref.find(li[1 + j]);
            if (it == ref.end()) {
                it = ref.emplace(li[1 + j], (int32_t)src.size()).first;
                src.push_back(li[1 + j]);
            }
            refs.push_back(it->second);
        }
        for (int j = nc; j < K; j++) refs.push_back(0);
        double *mrec = meta.data() + 1 + 6 * cnt;
        mrec[0] = nd.dual_bound; mrec[1] = nd.b_val; mrec[2] = (double)nd.depth;
        mrec[3] = (double)nd.b_idx; mrec[4] = (double)nd.b_dir; mrec[5] = (double)nc;
        slots.push_back(nd.slot);
        nd.slot = -1;
        with_cuts += nc > 0;
        cnt++;
    }
    meta[0] = (double)cnt;
    meta[L.nmeta - 1] = (double)src.size();
    if (cnt > 0) {
        mipx::PackArgs pa = mig_args(t, L, msg, scratch);
        HIP_TRY(ctx, hipMemcpyAsync(scratch, slots.data(), (size_t)cnt * 4, hipMemcpyHostToDevice, t->st2));
        enqueue_pack_nodes(pa, (int)cnt, t->st2);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(d_lists, refs.data(), refs.size() * 4, hipMemcpyHostToDevice, t->st2));
    }
    if (!src.empty()) {
        int32_t *d_src = mig_src(scratch, amount);
        HIP_TRY(ctx, hipMemcpyAsync(d_src, src.data(), src.size() * 4, hipMemcpyHostToDevice, t->st2));
        mipx::CutMigArgs ca;
        ca.n = t->n; ca.src = d_src; ca.store_pi = t->store_pi; ca.store_pi0 = t->store_pi0;
        ca.tab_pi = (double *)(msg + L.tab_off); ca.tab_pi0 = ca.tab_pi + (size_t)L.ctab * t->n;
        enqueue_cutmig_gather(ca, (int)src.size(), t->st2);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipMemcpyAsync(msg + L.meta_off, meta.data(), meta.size() * 8, hipMemcpyHostToDevice, t->st2));
    HIP_TRY(ctx, hipStreamSynchronize(t->st2));
    t->cm_nodes_sent += with_cuts;
    t->cm_rows_sent += (int64_t)src.size();
    *count = cnt;
    *table_rows = (int64_t)src.size();
    return MIPX_OK;
}

// receiver half, cut mode: as mig_unpack, and the table fills the next rows of this rank's migration region
int mig_unpack_cuts(mipx_tree *t, const MigLayout &L, char *msg, int32_t *scratch, int64_t amount, int64_t *count) {
    mipx_ctx *ctx = t->ctx;
    std::vector<double> meta(L.nmeta, 0.0);
    std::vector<int32_t> slots;
    HIP_TRY(ctx, hipMemcpy(meta.data(), msg + L.meta_off, meta.size() * 8, hipMemcpyDeviceToHost));
    const int64_t cnt = (int64_t)meta[0], rows = (int64_t)meta[L.nmeta - 1];
    if (cnt < 0 || cnt > amount || rows < 0 || rows > L.ctab) return fail(ctx, MIPX_EHIP, "tree: corrupt migration message");
    for (int64_t k = 0; k < cnt; k++) {
        const double nc = meta[1 + 6 * (size_t)k + 5];
        if (!(nc >= 0 && nc <= L.kc)) return fail(ctx, MIPX_EHIP, "tree: corrupt migration message");
    }
    // (the table was capped by the region rows this rank reported in its record, [13])
    if (rows > t->cm_rows - t->cm_used)
        return fail(ctx, MIPX_ENOMEM, "tree: cut store region too small for the migrated nodes (raise the rows of "
                                      "mipx_tree_set_cut_migration)");
    if ((int64_t)t->free_slots.size() < cnt)
        return fail(ctx, MIPX_ENOMEM, "tree: node pool too small for the migrated nodes (raise pool_capacity)");
    if (t->child_recorded) HIP_TRY(ctx, hipStreamWaitEvent(t->st2, t->ev_child, 0));
    for (int64_t k = 0; k < cnt; k++) {
        const double *mrec = meta.data() + 1 + 6 * k;
        NodeRec nd;
        nd.dual_bound = mrec[0]; nd.b_val = mrec[1]; nd.depth = (int32_t)mrec[2];
        nd.b_idx = (int32_t)mrec[3]; nd.b_dir = (int32_t)mrec[4];
        nd.key = t->search == 0 ? nd.dual_bound : -(double)nd.depth;
        nd.anchor = -1; nd.born = (int32_t)t->steps; nd.ncut = (int32_t)mrec[5];
        nd.slot = t->free_slots.back();
        t->free_slots.pop_back();
        slots.push_back(nd.slot);
        t->nodes.push_back(nd);
        tree_push(t, (int64_t)t->nodes.size() - 1);
    }
    if (cnt > 0) {
        const int64_t base = t->store_cap - t->cm_rows + t->cm_used;
        int32_t *d_bad = mig_bad(L, scratch, amount);
        int32_t bad = 0;
        HIP_TRY(ctx, hipMemcpyAsync(scratch, slots.data(), (size_t)cnt * 4, hipMemcpyHostToDevice, t->st2));
        HIP_TRY(ctx, hipMemsetAsync(d_bad, 0, 4, t->st2));
        mipx::PackArgs pa = mig_args(t, L, msg, scratch);
        enqueue_unpack_nodes(pa, (int)cnt, t->st2);
        HIP_TRY(ctx, hipGetLastError());
        mipx::CutMigArgs ca;
        ca.n = t->n; ca.kc = L.kc; ca.slot = scratch; ca.pool_ncut = t->pool_ncut; ca.pool_ids = t->pool_ids;
        ca.lists = (int32_t *)(msg + L.refs_off); ca.store_pi = t->store_pi; ca.store_pi0 = t->store_pi0;
        ca.tab_pi = (double *)(msg + L.tab_off); ca.tab_pi0 = ca.tab_pi + (size_t)L.ctab * t->n;
        ca.base = base; ca.ctab = (int)rows; ca.bad = d_bad;
        enqueue_cutmig_unpack_lists(ca, (int)cnt, t->st2);
        HIP_TRY(ctx, hipGetLastError());
        if (rows > 0) {
            enqueue_cutmig_scatter(ca, (int)rows, t->st2);
            HIP_TRY(ctx, hipGetLastError());
        }
        HIP_TRY(ctx, hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, t->st2));
        HIP_TRY(ctx, hipStreamSynchronize(t->st2));
        t->cm_used += rows;
        t->cm_rows_received += rows;
        if (bad) return fail(ctx, MIPX_EHIP, "tree: corrupt cut lists in a migration message");
    }
    *count = cnt;
    return MIPX_OK;
}

int x_migrate(mipx_tree *t, int from, int to, int64_t amount, int64_t ctab) {
    mipx_comm *c = t->comm;
    const int me = c->rank;
    if (me != from && me != to) return MIPX_OK;
    const MigLayout L = mig_layout(t, amount, ctab);
    char *msg = nullptr;
    int rc = comm_msg_buffer(c, L.bytes + L.scratch, &msg);   // (+ the slot list of the pack kernels)
    if (rc) return rc;
    int32_t *d_slots = (int32_t *)(msg + L.bytes);
    int64_t cnt = 0;
    if (me == from) {
        std::vector<int32_t> slots;
        int64_t rows = 0;
        if (L.kc > 0) rc = mig_pack_cuts(t, L, msg, d_slots, amount, slots, &cnt, &rows);
        else rc = mig_pack(t, L, msg, d_slots, amount, slots, &cnt);
        if (rc) return rc;
        if ((rc = comm_send_dev(c, to, msg, L.bytes))) return rc;
        for (int32_t sl : slots) t->free_slots.push_back(sl);
        t->nodes_sent += cnt;
    } else {
        if ((rc = comm_recv_dev(c, from, msg, L.bytes))) return rc;
        if (L.kc > 0) rc = mig_unpack_cuts(t, L, msg, d_slots, amount, &cnt);
        else rc = mig_unpack(t, L, msg, d_slots, amount, &cnt);
        if (rc) return rc;
        t->nodes_received += cnt;
    }
    return MIPX_OK;
}

// What every rank concludes from one gathered set of records -- a pure function of the records, so
// that all ranks conclude the same (exposed as mipx_exchange_decide for the CPU tests).
void x_decide(int W, int n, const double *records, double mip_gap, bool allow_migration,
              mipx_exchange_decision *out) {
    const size_t len = (size_t)kRecHead + 5 * (size_t)n;
    const double inf = std::numeric_limits<double>::infinity();
    auto rec = [&](int r) { return records + (size_t)r * len; };
    // incumbent: the best value of any rank, and the lowest rank that holds a solution for it
    double best = inf, dual = inf;
    int who = -1;
    int64_t sums[5] = {0, 0, 0, 0, 0};
    // stop flags: 1 = a limit that ends the search for everybody (node_limit, max_seconds, unbounded,
    // a full pool); 2 = this rank has done the steps it was asked for (max_steps is a per-rank quota:
    // the others finish theirs)
    bool any_stop = false, all_finished = true, any_fatal = false;
    for (int r = 0; r < W; r++) {
        const double *q = rec(r);
        if (q[0] < best) best = q[0];
        dual = std::fmin(dual, q[1]);
        sums[0] += (int64_t)q[4]; sums[1] += (int64_t)q[5]; sums[2] += (int64_t)q[6]; sums[3] += (int64_t)q[7];
        sums[4] += (int64_t)q[2];
        any_stop |= q[3] == 1.0;
        any_fatal |= q[3] == 3.0;
        all_finished &= q[3] == 2.0 || q[2] == 0.0;
    }
    for (int r = 0; r < W && who < 0; r++)
        if (rec(r)[0] == best && rec(r)[8] != 0.0 && best < inf) who = r;
    double gap = -1.0;   // reference current_gap (branch_and_bound.py:203-213); -1 encodes None
    if (best < inf) {
        if (best == 0 && dual == 0) gap = 0.0;
        else if (best == 0) gap = inf;
        else gap = std::fabs(best - dual) / std::fabs(best);
    }
    out->primal = best; out->dual = dual; out->gap = gap; out->incumbent_rank = who;
    for (int k = 0; k < 4; k++) out->sums[k] = sums[k];
    out->open_nodes = sums[4];
    out->reason = any_fatal ? 5 : sums[4] == 0 ? 1 : any_stop ? 2 : (gap >= 0 && gap <= mip_gap) ? 3 : all_finished ? 4 : 0;
    out->done = out->reason != 0;
    out->n_moves = 0;
    // with cut rounds ([15]) nodes move only when every rank takes cut rows the same way ([14]: kc, 0 = off)
    bool cut_ok = true;
    for (int r = 0; r < W; r++)
        if (rec(r)[15] != 0.0) cut_ok = false;
    if (!cut_ok) {
        cut_ok = rec(0)[14] > 0.0;
        for (int r = 0; r < W; r++) cut_ok = cut_ok && rec(r)[15] != 0.0 && rec(r)[14] == rec(0)[14];
    }
    // migration: a rank that cannot fill a batch gets half the surplus of the fullest rank
    if (!out->done && allow_migration && cut_ok && W > 1) {
        std::vector<int64_t> open((size_t)W), low((size_t)W), room((size_t)W);
        for (int r = 0; r < W; r++) {
            open[(size_t)r] = (int64_t)rec(r)[2]; low[(size_t)r] = std::max<int64_t>(1, (int64_t)rec(r)[10]);
            room[(size_t)r] = (int64_t)rec(r)[11];
        }
        for (int d = 0; d < W && out->n_moves < 64; d++) {
            if (open[(size_t)d] >= low[(size_t)d]) continue;
            int src = 0;
            for (int r = 1; r < W; r++)
                if (open[(size_t)r] > open[(size_t)src]) src = r;
            if (src == d || open[(size_t)src] < 2 * low[(size_t)src]) continue;
            // (never more than the receiver said it has room for: it cannot refuse once the donor has sent)
            const int64_t amount = std::min<int64_t>(std::min<int64_t>((open[(size_t)src] - open[(size_t)d]) / 2, kMaxMigrate),
                                                     room[(size_t)d]);
            if (amount <= 0) continue;
            room[(size_t)d] -= amount;
            int32_t *mv = out->moves + 3 * out->n_moves++;
            mv[0] = src; mv[1] = d; mv[2] = (int32_t)amount;
            open[(size_t)src] -= amount;
            open[(size_t)d] += amount;
        }
    }
}

// Apply one gathered set of records (identical on every rank).  last: the closing exchange -- merge
// only, no decisions.
int x_apply(mipx_tree *t, const char *gathered, bool last) {
    const mipx_comm *c = t->comm;
    const int W = c->world, me = c->rank;
    const size_t n = (size_t)t->n, len = x_rec_len(t);
    const double inf = std::numeric_limits<double>::infinity();
    auto rec = [&](int r) { return (const double *)(gathered + (size_t)r * len * 8); };
    mipx_exchange_decision D;
    x_decide(W, t->n, (const double *)gathered, t->x_mip_gap, true, &D);
    const double best = D.primal;
    const int who = D.incumbent_rank;
    if (best < t->primal || (best == t->primal && best < inf && !t->have_x && who >= 0)) {
        t->primal = best;
        if (who >= 0) {
            std::memcpy(t->best_x.data(), rec(who) + kRecHead, n * 8);
            t->have_x = true;
        }
    }
    if (t->primal == best) t->g_inc_rank = (t->primal < inf && who >= 0) ? who : (t->have_x && t->primal < inf ? me : -1);
    else t->g_inc_rank = t->have_x ? me : -1;   // (this rank found a better one since it posted)
    t->g_dual = D.dual;
    for (int k = 0; k < 4; k++) t->g_counts[k] = t->ramp[k] + D.sums[k];
    t->g_counts[4] = D.open_nodes;
    // pseudo costs: what all ranks agreed on at sharding time + every other rank's samples as of its
    // record + this rank's own samples as of now
    if (t->rule == 1) {
        std::fill(t->pc_others.begin(), t->pc_others.end(), 0.0);
        for (int r = 0; r < W; r++) {
            if (r == me) continue;
            const double *o = rec(r) + kRecHead + n;
            for (size_t j = 0; j < 4 * n; j++) t->pc_others[j] += o[j];
        }
    }
    if (t->rule == 1 && t->fast_ok) {
        // Device finish: the table lives on the device and holds this rank's samples up to the steps in flight.
        // What the OTHER ranks sampled since the last exchange joins it in sum form (pc_merge, queued on stf
        // behind the finishes already there); the host's snapshot is merged the same way.
        if (t->pc_others_prev.size() != 4 * n) t->pc_others_prev.assign(4 * n, 0.0);
        double *hd = t->h_delta + (size_t)(t->delta_turn & 3) * 4 * n;
        // Per entry the increase since the HIGHEST times merged so far, and only there does pc_others_prev
        // advance: a peer's record whose times fall back for an exchange and recover (mipx.h, the pseudo-cost
        // merge) is neither merged twice nor lost.  An entry that is not merged sends a zero delta.
        bool any = false;
        for (size_t e = 0; e < 2 * n; e++) {
            const size_t js = e, jt = 2 * n + e;
            const double dt = t->pc_others[jt] - t->pc_others_prev[jt];
            if (dt > 0.0) {
                hd[js] = t->pc_others[js] - t->pc_others_prev[js];
                hd[jt] = dt;
                t->pc_others_prev[js] = t->pc_others[js];
                t->pc_others_prev[jt] = t->pc_others[jt];
                any = true;
            } else {
                hd[js] = 0.0; hd[jt] = 0.0;
            }
        }
        if (any) {
            for (size_t e = 0; e < 2 * n; e++) {
                const size_t dir = e / n, var = e - dir * n;
                const double ds = hd[dir * n + var], dt = hd[(2 + dir) * n + var];
                if (!(dt > 0.0)) continue;
                double &cost = dir ? t->cost_r[var] : t->cost_l[var];
                int32_t &times = dir ? t->times_r[var] : t->times_l[var];
                cost = (cost * (double)times + ds) / ((double)times + dt);
                times += (int32_t)dt;
                t->has_entry[var] = 1;
            }
            double *dd = t->d_delta + (size_t)(t->delta_turn & 3) * 4 * n;
            t->delta_turn++;
            mipx_ctx *ctx = t->ctx;
            HIP_TRY(ctx, hipMemcpyAsync(dd, hd, 4 * n * 8, hipMemcpyHostToDevice, t->stf));
            const TabPtr tb = tab_at(t, t->tab_tail);
            mipx::PcMergeArgs ma;
            ma.n = t->n; ma.delta = dd; ma.cost_l = tb.cl; ma.cost_r = tb.cr; ma.has = tb.has; ma.times = tb.times;
            hipLaunchKernelGGL(mipx::pc_merge, dim3((2 * t->n + 255) / 256), dim3(256), 0, t->stf, ma);
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipEventRecord(t->ev_tab[t->tab_tail], t->stf));
            t->tab_late[t->tab_tail] = true;
        }
    } else if (t->rule == 1) {
        for (size_t j = 0; j < n; j++) {
            const double tl = t->pc_base[2 * n + j] + t->pc_others[2 * n + j] + t->pc_own[2 * n + j];
            const double tr = t->pc_base[3 * n + j] + t->pc_others[3 * n + j] + t->pc_own[3 * n + j];
            const double sl = t->pc_base[j] + t->pc_others[j] + t->pc_own[j];
            const double sr = t->pc_base[n + j] + t->pc_others[n + j] + t->pc_own[n + j];
            t->times_l[j] = (int32_t)tl; t->times_r[j] = (int32_t)tr;
            t->cost_l[j] = tl > 0 ? sl / tl : 0.0;
            t->cost_r[j] = tr > 0 ? sr / tr : 0.0;
            t->has_entry[j] = (tl > 0 || tr > 0) ? 1 : 0;
        }
        t->table_dirty = true;
        t->times_dirty = true;
    }
    t->x_rounds++;
    if (last) return MIPX_OK;
    if (D.done) {   // every rank idle, a rank's limit, the global gap, or a rank that failed: the same on every rank
        t->x_done = true;
        t->x_fatal = D.reason == 5;
        return MIPX_OK;
    }
    for (int k = 0; k < D.n_moves; k++) {
        // (cut mode: the table rows follow from the receiver's record, the same on both ends; a receiver
        // gets at most one donation per exchange, so [13] is what its region can take)
        const int to = D.moves[3 * k + 1];
        const int64_t ctab = t->cuts ? mig_table_rows(rec(to)[13], D.moves[3 * k + 2], t->kc) : 0;
        const int rc = x_migrate(t, D.moves[3 * k], to, D.moves[3 * k + 2], ctab);
        if (rc) return rc;
    }
    return MIPX_OK;
}

// One call at an exchange point.  Collects the all-gather posted last time (by then long finished on
// a busy rank) and posts the next; a rank with nothing to do (blocking) waits for that one as well.
int x_tick(mipx_tree *t, bool blocking) {
    mipx_comm *c = t->comm;
    const char *g = nullptr;
    int rc;
    if (c->pending) {
        if ((rc = comm_collect(c, &g))) return rc;
        if ((rc = x_apply(t, g, false))) return rc;
        if (t->x_done) return MIPX_OK;
    }
    x_fill_record(t);
    if ((rc = comm_post(c, t->x_rec.data(), x_rec_len(t) * 8))) return rc;
    if (blocking) {
        if ((rc = comm_collect(c, &g))) return rc;
        if ((rc = x_apply(t, g, false))) return rc;
    }
    return MIPX_OK;
}

// The closing exchange after the ranks agreed to stop: what each found since its last record.
int x_close(mipx_tree *t) {
    mipx_comm *c = t->comm;
    const char *g = nullptr;
    int rc;
    x_fill_record(t);
    if ((rc = comm_post(c, t->x_rec.data(), x_rec_len(t) * 8))) return rc;
    if ((rc = comm_collect(c, &g))) return rc;
    return x_apply(t, g, true);
}

// This rank is about to return an error from the step loop: tell the others, or they would wait for it
// in the next all-gather for ever.  The sequence of all-gathers stays aligned: what was posted is
// collected and applied, a record with the fatal flag follows (every rank that applies it stops, reason
// 5), then the closing exchange the others run.  Best effort: an error in here is dropped (the rank is
// failing already); a failure inside a migration's send / recv cannot be announced this way.
void x_fail(mipx_tree *t) {
    mipx_comm *c = t->comm;
    const char *g = nullptr;
    t->x_stop_flag = 3;
    if (c->pending) {
        if (comm_collect(c, &g)) return;
        if (x_apply(t, g, false)) return;
    }
    if (!t->x_done) {
        x_fill_record(t);
        if (comm_post(c, t->x_rec.data(), x_rec_len(t) * 8)) return;
        if (comm_collect(c, &g)) return;
        if (x_apply(t, g, false)) return;
    }
    if (t->x_done) (void)x_close(t);
}

}  // namespace

extern "C" {

int mipx_tree_create(mipx_problem *p, const int32_t *int_idx, int n_int, const double *l,
                     const double *u, int branch_rule, int search_rule, int strong_branch_iters,
                     int max_batch, int64_t pool_capacity, mipx_tree **out) {
    return mipx_tree_create_ex(p, int_idx, n_int, l, u, branch_rule, search_rule, strong_branch_iters,
                               max_batch, pool_capacity, nullptr, out);
}

int mipx_tree_create_ex(mipx_problem *p, const int32_t *int_idx, int n_int, const double *l,
                        const double *u, int branch_rule, int search_rule, int strong_branch_iters,
                        int max_batch, int64_t pool_capacity, const mipx_cut_params *cuts,
                        mipx_tree **out) {
    if (!p || !out || n_int < 0 || (n_int && !int_idx) || !l || !u || max_batch < 1 ||
        branch_rule < 0 || branch_rule > 1 || search_rule < 0 || search_rule > 1 ||
        strong_branch_iters < 1)
        return fail(p ? p->ctx : nullptr, MIPX_EINVAL, "mipx_tree_create: bad argument");
    mipx_ctx *ctx = p->ctx;
    *out = nullptr;
    int kc = 0;
    if (cuts != nullptr) {
        kc = cuts->max_cuts_per_node > 0 ? cuts->max_cuts_per_node : mipx::kMaxNodeCuts;
        if (kc > mipx::kMaxNodeCuts || cuts->max_cut_generation_iterations < 1 || cuts->max_nonzero_coefs < 1 ||
            !(cuts->cutting_plane_progress_tolerance > 0) || !(cuts->min_cut_depth > 0) || !(cuts->max_term > 0) ||
            cuts->store_capacity < 0)
            return fail(ctx, MIPX_EINVAL, "mipx_tree_create_ex: bad cut parameter");
        if (pick_cfg(p->m, p->n) != nullptr) {
            // register tiles: the rows of a node must fit one; keep as many cut rows as the largest tile takes
            // (all launches of the tree then price alike: the tiles' steepest edge)
            while (kc > 0 && pick_cfg(p->m + kc, p->n) == nullptr) kc--;
        } else {
            // above them every launch streams its tableau (K1b): the slabs take the cut rows too
            while (kc > 0 && !big_fits(p->m + kc, p->n)) kc--;
        }
        if (kc == 0)
            return fail(ctx, MIPX_ETOOBIG, "mipx_tree_create_ex: no room for a cut row (m + cuts <= 192 rows on the register "
                                            "tiles, <= 1024 above them)");
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    mipx_tree *t = new (std::nothrow) mipx_tree();
    if (!t) return fail(ctx, MIPX_ENOMEM, "mipx_tree_create: host alloc");
    t->prob = p; t->ctx = ctx; t->n = p->n; t->m = p->m; t->n_int = n_int;
    t->rule = branch_rule; t->search = search_rule; t->sb_iters = strong_branch_iters;
    t->max_batch = max_batch;
    t->use_bq = max_batch > 1 && search_rule == 0;
    t->capacity = pool_capacity > 2 * (int64_t)max_batch + 2 ? pool_capacity : 2 * (int64_t)max_batch + 2;
    t->int_idx.assign(int_idx, int_idx + n_int);
    for (int i = 0; i < n_int; i++)
        if (int_idx[i] < 0 || int_idx[i] >= t->n) { delete t; return fail(ctx, MIPX_EINVAL, "mipx_tree_create: integer index out of range"); }
    t->cuts = cuts != nullptr;
    t->kc = kc;
    t->mrows = t->m + kc;
    if (t->cuts) {
        t->cp = *cuts;
        t->store_cap = cuts->store_capacity > 0 ? cuts->store_capacity : ((int64_t)1 << 20);
        if (t->store_cap > 0x7fffffff) t->store_cap = 0x7fffffff;
        // candidate cuts of one node while it is bounded: every round adds at most one per row; K3
        // keeps three doubles and two ints per candidate in LDS (64 KiB)
        int64_t rows = (int64_t)cuts->max_cut_generation_iterations * t->mrows;
        if (rows > 2040) rows = 2040;
        if (rows < t->mrows) rows = t->mrows;
        t->slab_rows = (int)rows;
        t->pipeline = false;   // (the cut loop of a step reads back per round: steps do not overlap)
    }
    const size_t n = t->n, nv = (size_t)t->n + t->mrows, cap = (size_t)t->capacity, B = (size_t)max_batch;
    t->probe_cap = 2 * (int64_t)B * (n_int ? n_int : 1);
    if (t->probe_cap > (int64_t)1 << 18) t->probe_cap = (int64_t)1 << 18;  // 2^18 probe records (~1.2 GB at 256x128)
    const size_t pc = (size_t)t->probe_cap;
    int rc = 0;
    rc |= dmalloc(ctx, &t->pool_l, cap * n); rc |= dmalloc(ctx, &t->pool_u, cap * n);
    rc |= dmalloc(ctx, &t->pool_v, cap * nv);
    rc |= dmalloc(ctx, &t->d_int_idx, (size_t)n_int);
    const size_t LC = (size_t)kMaxDive + 1;   // output levels the buffers are sized for
    const size_t pairs = step_layout::PairList(pc / 2 > LC * B ? pc / 2 : LC * B).bytes() / 4;   // (one part per dive level)
    rc |= dmalloc(ctx, &t->d_pairs, pairs);
    rc |= dmalloc(ctx, &t->d_pairs2, pairs);
    rc |= dmalloc(ctx, &t->d_cost_l2, n); rc |= dmalloc(ctx, &t->d_cost_r2, n); rc |= dmalloc(ctx, &t->d_has2, n);
    // The side streams carry short, latency-critical work (probes, re-scoring, child records) that
    // must overtake the 2 ms node-LP launch queued on the main stream.  HIP multiplexes the streams
    // of one priority onto a few hardware queues, so in a process that owns more streams (a framework +
    // RCCL in a multi-GPU rank) a normal-priority side stream can land behind the main stream's
    // queue; high-priority streams come from their own queue pool.
    int prio_least = 0, prio_greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) != hipSuccess) prio_greatest = 0;
    if (hipStreamCreateWithPriority(&t->st2, hipStreamNonBlocking, prio_greatest) != hipSuccess) rc |= MIPX_EHIP;
    if (hipStreamCreateWithPriority(&t->stf, hipStreamNonBlocking, prio_greatest) != hipSuccess) rc |= MIPX_EHIP;
    if (hipStreamCreateWithPriority(&t->st3, hipStreamNonBlocking, prio_greatest) != hipSuccess ||
        hipEventCreateWithFlags(&t->ev_child, hipEventDisableTiming) != hipSuccess ||
        hipHostMalloc((void **)&t->h_pairs, step_layout::PairList(LC * B).bytes(), hipHostMallocDefault) != hipSuccess) rc |= MIPX_EHIP;
    if (t->cuts) {
        const size_t M = (size_t)t->mrows, K = (size_t)t->kc, SR = (size_t)t->slab_rows;
        rc |= dmalloc(ctx, &t->store_pi, (size_t)t->store_cap * n); rc |= dmalloc(ctx, &t->store_pi0, (size_t)t->store_cap);
        rc |= dmalloc(ctx, &t->store_count, 4);
        rc |= dmalloc(ctx, &t->pool_ncut, cap); rc |= dmalloc(ctx, &t->pool_ids, cap * K);
        rc |= dmalloc(ctx, &t->pp_ncut, pc); rc |= dmalloc(ctx, &t->pp_ids, pc * K);
        rc |= dmalloc(ctx, &t->d_is_int, n);
        for (StepBuf &S : t->buf) {
            rc |= dmalloc(ctx, &S.w_ncut, B); rc |= dmalloc(ctx, &S.w_ids, B * K);
            rc |= dmalloc(ctx, &S.cs_state, (size_t)mipx::CF_FIELDS * B);
            rc |= dmalloc(ctx, &S.cs_active, B); rc |= dmalloc(ctx, &S.cs_resolve, B);
            rc |= dmalloc(ctx, &S.cs_need_tab, B);
            rc |= dmalloc(ctx, &S.cs_counters, 4); rc |= dmalloc(ctx, &S.k2_ncuts, B);
            rc |= dmalloc(ctx, &S.k3_nadded, B); rc |= dmalloc(ctx, &S.k3_added, B * SR);
            rc |= dmalloc(ctx, &S.k3_term, B); rc |= dmalloc(ctx, &S.pool_list, B * SR);
            rc |= dmalloc(ctx, &S.d_y, B * M); rc |= dmalloc(ctx, &S.cs_before, B);
            rc |= dmalloc(ctx, &S.slab_pi, B * SR * n); rc |= dmalloc(ctx, &S.slab_pi0, B * SR);
            rc |= dmalloc(ctx, &S.dump_T, B * M * n); rc |= dmalloc(ctx, &S.dump_vec, B * (n + 3 * M));
            rc |= dmalloc(ctx, &S.dump_idx, B * (2 * n + M));
            if (hipHostMalloc((void **)&S.h_cs, CutState(B).bytes(), hipHostMallocDefault) != hipSuccess) rc |= MIPX_EHIP;
            if (!t->pipeline) break;   // steps do not overlap: one buffer set is in use
        }
    }
    for (StepBuf &S : t->buf) {
        rc |= dmalloc(ctx, &S.d_slot, 2 * B);   // [pool rows | anchor-table entries] of the batch
        // per-node outputs have one row per output level: the batch, then its dive children level by
        // level (allocated for the deepest plunge, laid out for the depth in use: layout_pack)
        rc |= dmalloc(ctx, &S.d_iters, LC * B);
        const size_t pack_cap = step_pack(t, 1 + kMaxDive).bytes();
        rc |= dmalloc(ctx, &S.d_pack, pack_cap);
        if (hipHostMalloc((void **)&S.h_pack, pack_cap, hipHostMallocDefault) != hipSuccess ||
            hipHostMalloc((void **)&S.h_slot, 2 * B * 4, hipHostMallocDefault) != hipSuccess) rc |= MIPX_EHIP;
        if (S.d_pack) layout_pack(t, S, 1);
        rc |= dmalloc(ctx, &S.d_plist, LC * B * (size_t)(n_int ? n_int : 1));
        rc |= dmalloc(ctx, &S.d_x, LC * B * n);
        rc |= dmalloc(ctx, &S.d_vout, LC * B * nv);
        if (hipEventCreate(&S.e0) != hipSuccess || hipEventCreate(&S.e1) != hipSuccess ||
            hipEventCreate(&S.done) != hipSuccess) rc |= MIPX_EHIP;
        if (t->cuts && (hipEventCreate(&S.k2a) != hipSuccess || hipEventCreate(&S.k2b) != hipSuccess ||
                        hipEventCreate(&S.k3b) != hipSuccess)) rc |= MIPX_EHIP;
    }
    // Steps are finished on the device (finish_kernels.hip.h) in the batched modes without cut rounds;
    // MIPX_HOST_FINISH=1 keeps the host loop (A/B runs).  The exact mode (max_batch = 1) reproduces the
    // reference's node order on the host.
    t->fast_ok = max_batch > 1 && !t->cuts && !(std::getenv("MIPX_HOST_FINISH") && std::atoi(std::getenv("MIPX_HOST_FINISH")) != 0);
    {   // [cost_l | cost_r | has_entry] in one allocation: one upload per step; behind them (device finish)
        // [times_l | times_r | own sums], and kTabV versions of the whole block
        char *tab = nullptr;
        t->tab_off2 = (17 * n + 7) / 8 * 8;
        t->tab_bytes = t->tab_off2 + 8 * n + 32 * n;
        t->tab_stride = (t->tab_bytes + 255) / 256 * 256;
        rc |= dmalloc(ctx, &tab, t->tab_stride * (t->fast_ok ? (size_t)kTabV : 1));
        t->d_cost_l = (double *)tab;
        t->d_cost_r = tab ? (double *)(tab + 8 * n) : nullptr;
        t->d_has = tab ? (uint8_t *)(tab + 16 * n) : nullptr;
        if (hipHostMalloc((void **)&t->h_tab, 4 * 17 * n + 4 * 8 * n, hipHostMallocDefault) != hipSuccess) rc |= MIPX_EHIP;
        rc |= dmalloc(ctx, &t->d_primal, 1);
    }
    if (t->fast_ok) {
        const size_t per = 2 * LC;
        rc |= dmalloc(ctx, &t->d_delta, 4 * 4 * n);
        if (hipHostMalloc((void **)&t->h_delta, 4 * 4 * n * 8, hipHostMallocDefault) != hipSuccess) rc |= MIPX_EHIP;
        static_assert(kTabV == 8, "ev_tab / tab_late are sized for the version ring");
        for (int v = 0; v < kTabV; v++)
            if (hipEventCreateWithFlags(&t->ev_tab[v], hipEventDisableTiming) != hipSuccess) rc |= MIPX_EHIP;
        t->samples_cap = (size_t)t->probe_cap + LC * B;
        for (StepBuf &S : t->buf) {
            const size_t par_bytes = step_layout::ParentBlock(B, per).bytes();
            rc |= dmalloc(ctx, &S.d_par, par_bytes);
            rc |= dmalloc(ctx, &S.c_info, B); rc |= dmalloc(ctx, &S.c_cnt, 3 * B); rc |= dmalloc(ctx, &S.c_eval, 2 * B);
            rc |= dmalloc(ctx, &S.c_flag, B); rc |= dmalloc(ctx, &S.c_val, 3 * B);
            rc |= dmalloc(ctx, &S.d_sum, 1);
            rc |= dmalloc(ctx, &S.d_open, per * B); rc |= dmalloc(ctx, &S.d_dead, per * B);
            rc |= dmalloc(ctx, &S.d_samples, t->samples_cap);
            rc |= dmalloc(ctx, &S.d_skeys, t->samples_cap);
            const size_t fin_bytes = finish_block(t, per).bytes();
            if (hipHostMalloc((void **)&S.h_par, par_bytes, hipHostMallocDefault) != hipSuccess ||
                hipHostMalloc((void **)&S.h_fin, fin_bytes, hipHostMallocDefault) != hipSuccess ||
                hipHostMalloc((void **)&S.h_samples, t->samples_cap * (sizeof(mipx::PcSample) + 4), hipHostMallocDefault) != hipSuccess)
                rc |= MIPX_EHIP;
        }
    }
    if (branch_rule == 1) {
        rc |= dmalloc(ctx, &t->pp_l, pc * n); rc |= dmalloc(ctx, &t->pp_u, pc * n);
        rc |= dmalloc(ctx, &t->pp_v, pc * nv); rc |= dmalloc(ctx, &t->pp_obj, pc);
        rc |= dmalloc(ctx, &t->pp_status, pc);
        if (hipHostMalloc((void **)&t->h_pres, pc * 12, hipHostMallocDefault) != hipSuccess) rc |= MIPX_EHIP;
    }
    if (rc) { mipx_tree_destroy(t); return MIPX_EHIP; }
    t->cost_l.assign(n, 0.0); t->cost_r.assign(n, 0.0);
    t->times_l.assign(n, 0); t->times_r.assign(n, 0);
    t->has_entry.assign(n, 0);
    t->best_x.assign(n, 0.0);
    HIP_TRY(ctx, hipMemcpy(t->d_int_idx, int_idx, (size_t)n_int * 4, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemset(t->d_cost_l, 0, t->tab_stride * (t->fast_ok ? (size_t)kTabV : 1)));   // costs, entries, times, own sums
    {
        const double inf_ = std::numeric_limits<double>::infinity();
        HIP_TRY(ctx, hipMemcpy(t->d_primal, &inf_, 8, hipMemcpyHostToDevice));
    }
    // root record in slot 0: cold start (all status codes 0 -> slack basis, sides from d_j)
    t->root_l.assign(l, l + n);
    t->root_u.assign(u, u + n);
    HIP_TRY(ctx, hipMemcpy(t->pool_l, l, n * 8, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(t->pool_u, u, n * 8, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemset(t->pool_v, 0, nv));
    if (t->cuts) {
        std::vector<uint8_t> is_int(n, 0);
        for (int i = 0; i < n_int; i++) is_int[(size_t)int_idx[i]] = 1;
        HIP_TRY(ctx, hipMemcpy(t->d_is_int, is_int.data(), n, hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemset(t->store_count, 0, 4));
        HIP_TRY(ctx, hipMemset(t->pool_ncut, 0, 4));   // the root carries no cut
    }
    t->free_slots.reserve(cap);
    for (int64_t s = (int64_t)cap - 1; s >= 1; s--) t->free_slots.push_back((int32_t)s);
    NodeRec root;
    root.dual_bound = -std::numeric_limits<double>::infinity();
    root.depth = 0; root.key = search_rule == 0 ? root.dual_bound : 0.0;
    root.b_idx = -1; root.b_dir = 0; root.b_val = 0.0; root.slot = 0; root.born = 0; root.anchor = -1;
    root.ncut = 0;
    t->nodes.push_back(root);
    *out = t;
    return MIPX_OK;
}

void mipx_tree_destroy(mipx_tree *t) {
    if (!t) return;
    if (std::getenv("MIPX_TREE_PROFILE"))
        std::fprintf(stderr, "[mipx_tree] steps %lld  pop %.1f ms  lp+score+d2h %.1f ms  pseudo-cost %.1f ms  "
                     "bookkeeping %.1f ms  children %.1f ms  (lp kernel %.1f ms)\n", (long long)t->steps,
                     t->phase_ms[0], t->phase_ms[1], t->phase_ms[2], t->phase_ms[3], t->phase_ms[4], t->kernel_ms);
    if (t->ctx) (void)hipSetDevice(t->ctx->device);
    if (t->ctx && t->ctx->stream) (void)hipStreamSynchronize(t->ctx->stream);
    if (t->st2) { (void)hipStreamSynchronize(t->st2); (void)hipStreamDestroy(t->st2); }
    if (t->st3) { (void)hipStreamSynchronize(t->st3); (void)hipStreamDestroy(t->st3); }
    if (t->stf) { (void)hipStreamSynchronize(t->stf); (void)hipStreamDestroy(t->stf); }
    if (t->ev_child) (void)hipEventDestroy(t->ev_child);
    if (t->hs.st) { (void)hipStreamSynchronize(t->hs.st); (void)hipStreamDestroy(t->hs.st); }
    {
        HostSpill &h = t->hs;
        void *hp[] = {h.d_root, h.d_slot, h.d_id, h.d_off, h.d_rec};
        for (void *q : hp)
            if (q) (void)hipFree(q);
        for (char *q : h.dead) (void)hipHostFree(q);
        for (const SpillSeg &g : h.segs)
            if (g.host) (void)hipHostFree(g.host);
        for (StepBuf &S : t->buf) {
            if (S.h_rl) (void)hipHostFree(S.h_rl);
            if (S.d_rl) (void)hipFree(S.d_rl);
        }
    }
    {
        DualFn &df = t->df;
        void *dp[] = {df.d_y, df.d_t, df.d_il, df.d_iu, df.d_iv, df.d_prec, df.d_order, df.d_lvl, df.d_leaf, df.d_V, df.d_W, df.d_out};
        for (void *q : dp)
            if (q) (void)hipFree(q);
        for (StepBuf &S : t->buf) {
            if (S.df_y) (void)hipFree(S.df_y);
            if (S.df_d) (void)hipFree(S.df_d);
            if (S.df_h) (void)hipHostFree(S.df_h);
            if (S.df_e0) (void)hipEventDestroy(S.df_e0);
            if (S.df_e1) (void)hipEventDestroy(S.df_e1);
        }
    }
    {
        TreeRec &tr = t->tr;
        void *dp[] = {tr.d_nodes, tr.d_root, tr.d_root_v, tr.d_ids, tr.d_l, tr.d_u, tr.d_solve};
        for (void *q : dp)
            if (q) (void)hipFree(q);
        if (tr.e0) (void)hipEventDestroy(tr.e0);
        if (tr.e1) (void)hipEventDestroy(tr.e1);
    }
    // the step options: their one-off buffers, and the ring behind each one's packed block
    void *ob[] = {t->hr.d_lu, t->cu.d_ws, t->cc.d_ws, t->ld.d_ws, t->ld.d_locks};
    for (void *q : ob)
        if (q) (void)hipFree(q);
    for (StepRing *r : {&t->hr.ring, &t->pg.ring, &t->ls.ring, &t->fp.ring, &t->wr.ring, &t->cu.ring, &t->cc.ring, &t->ld.ring})
        r->release();
    {
        RcState &rs = t->rc;
        for (int k = 0; k < 3; k++) {
            if (rs.d_y[k]) (void)hipFree(rs.d_y[k]);
            if (rs.d_io[k]) (void)hipFree(rs.d_io[k]);
            if (rs.h_io[k]) (void)hipHostFree(rs.h_io[k]);
            for (int q = 0; q < kRcLevels; q++) {
                if (rs.e0[k][q]) (void)hipEventDestroy(rs.e0[k][q]);
                if (rs.e1[k][q]) (void)hipEventDestroy(rs.e1[k][q]);
            }
        }
    }
    if (t->h_pairs) (void)hipHostFree(t->h_pairs);
    if (t->h_pres) (void)hipHostFree(t->h_pres);
    if (t->h_tab) (void)hipHostFree(t->h_tab);
    void *cptrs[] = {t->store_pi, t->store_pi0, t->store_count, t->pool_ncut, t->pool_ids, t->pp_ncut, t->pp_ids, t->d_is_int};
    for (void *q : cptrs)
        if (q) (void)hipFree(q);
    for (StepBuf &S : t->buf) {
        void *sp[] = {S.w_ncut, S.w_ids, S.cs_state, S.cs_active, S.cs_resolve, S.cs_counters, S.k2_ncuts, S.k3_nadded,
                      S.k3_added, S.k3_term, S.pool_list, S.d_y, S.cs_before, S.slab_pi, S.slab_pi0, S.dump_T, S.dump_vec,
                      S.dump_idx, S.cs_need_tab};
        for (void *q : sp)
            if (q) (void)hipFree(q);
        if (S.h_cs) (void)hipHostFree(S.h_cs);
    }
    void *ptrs[] = {t->atab_T, t->atab_vec, t->atab_idx, t->pool_l, t->pool_u, t->pool_v, t->d_int_idx, t->d_pairs, t->d_pairs2, t->d_cost_l,
                    t->d_cost_l2, t->d_cost_r2, t->d_has2, t->pp_l, t->pp_u, t->pp_v, t->pp_obj, t->pp_status};
    for (void *q : ptrs)
        if (q) (void)hipFree(q);
    if (t->d_primal) (void)hipFree(t->d_primal);
    if (t->d_delta) (void)hipFree(t->d_delta);
    if (t->h_delta) (void)hipHostFree(t->h_delta);
    for (hipEvent_t e : t->ev_tab)
        if (e) (void)hipEventDestroy(e);
    for (StepBuf &S : t->buf) {
        void *fp[] = {S.d_par, S.c_info, S.c_cnt, S.c_eval, S.c_flag, S.c_val, S.d_sum, S.d_open, S.d_dead, S.d_samples, S.d_skeys};
        for (void *q : fp)
            if (q) (void)hipFree(q);
        if (S.h_par) (void)hipHostFree(S.h_par);
        if (S.h_fin) (void)hipHostFree(S.h_fin);
        if (S.h_samples) (void)hipHostFree(S.h_samples);
    }
    for (StepBuf &S : t->buf) {
        void *sp[] = {S.d_slot, S.d_iters, S.d_pack, S.d_plist, S.d_x, S.d_vout};
        for (void *q : sp)
            if (q) (void)hipFree(q);
        if (S.h_pack) (void)hipHostFree(S.h_pack);
        if (S.h_slot) (void)hipHostFree(S.h_slot);
        if (S.e0) (void)hipEventDestroy(S.e0);
        if (S.e1) (void)hipEventDestroy(S.e1);
        if (S.done) (void)hipEventDestroy(S.done);
        if (S.k2a) (void)hipEventDestroy(S.k2a);
        if (S.k2b) (void)hipEventDestroy(S.k2b);
        if (S.k3b) (void)hipEventDestroy(S.k3b);
    }
    delete t;
}

int mipx_tree_set_anchor_mode(mipx_tree *t, int on) {
    if (!t) return MIPX_EINVAL;
    t->anchor_mode = on != 0;
    return MIPX_OK;
}

int mipx_tree_set_trace(mipx_tree *t, int on) {
    if (!t) return MIPX_EINVAL;
    t->trace = on != 0;
    return MIPX_OK;
}

int mipx_tree_set_primal_bound(mipx_tree *t, double bound) {
    if (!t) return MIPX_EINVAL;
    t->primal = bound;
    return MIPX_OK;
}

/*
 * Run (or continue) the search; mirrors BranchAndBound.solve (branch_and_bound.py:215-241).
 * node_limit <= 0 and max_seconds <= 0 and max_steps <= 0 mean "no limit".
 */
int mipx_tree_solve(mipx_tree *t, int64_t node_limit, double mip_gap, double max_seconds,
                    int frontier_batch, int64_t max_steps, mipx_tree_stats *out) {
    if (!t || frontier_batch < 1 || frontier_batch > t->max_batch)
        return fail(t ? t->ctx : nullptr, MIPX_EINVAL, "mipx_tree_solve: bad argument");
    mipx_ctx *ctx = t->ctx;
    if (t->hs.cap > 0 && t->capacity < 2 * spill_headroom(t) + 1)
        return fail(ctx, MIPX_EINVAL, "mipx_tree_solve: pool_capacity below the host spill headroom (see mipx_spill.h)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (t->df.on) {
        const int drc = df_prepare(t);
        if (drc) return drc;
    }
    const auto t0 = std::chrono::steady_clock::now();
    const double inf = std::numeric_limits<double>::infinity();
    double ph0[8], pr0[4];
    for (int k = 0; k < 8; k++) ph0[k] = t->phase_ms[k];
    for (int k = 0; k < 4; k++) pr0[k] = t->probe_ms[k];
    const double k0 = t->kernel_ms;
    if (!t->started) {
        t->started = true;
        tree_push(t, 0);
    }
    if (t->rs.on && t->anchor_mode && !t->anchor_set && t->tr.have_root && t->steps == 0) {
        // restart: the seeds warm-start from the source's root basis, and its tableau at this b is the anchor
        const int arc = mipx_problem_set_anchor(t->prob, t->tr.root_v.data());
        if (arc) return arc;
        t->anchor_set = true;
    }
    int64_t steps = 0, hooked_at = 0, xchg_at = 0;
    bool hook_stop = false;
    if (t->comm) {
        t->x_mip_gap = mip_gap; t->x_batch = frontier_batch; t->x_stop_flag = 0; t->x_done = false; t->x_fatal = false;
    }
    t->fault_step = std::getenv("MIPX_FAULT_STEP") ? std::atoi(std::getenv("MIPX_FAULT_STEP")) : 0;
    // an error of this rank's own step loop: the peers are told before it returns (x_fail)
    auto bail = [&](int rc) {
        if (t->comm && !t->x_done) x_fail(t);
        return rc;
    };
    // With frontier batches > 1 the host half of step k (bookkeeping, children) overlaps the GPU
    // halves of steps k+1 and k+2, whose batches are popped before the children of step k exist: a ring
    // of three step buffers.  Two steps queued ahead rather than one absorb a slow host half (the host
    // half is about as long as the node-LP kernel; with one step ahead every hiccup of the host idled
    // the GPU).
    const bool overlap = t->pipeline && frontier_batch > 1;
    const int NBUF = overlap ? 3 : 1;
    int head = 0, next = 0, nfl = 0;   // oldest step in flight, next free buffer, steps in flight
    auto inflight_nodes = [&]() {
        int64_t s = 0;
        for (int k = 0; k < nfl; k++) s += t->buf[(head + k) % NBUF].B;
        return s;
    };
    // this rank's own limits: 1 = one that ends the search, 2 = its step quota is done, 0 = none
    auto limit_kind = [&](int64_t inflight) {
        if (t->unbounded || hook_stop || t->pool_exhausted) return 1;
        if (node_limit > 0 && t->evaluated + inflight >= node_limit) return 1;
        const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (max_seconds > 0 && el > max_seconds) return 1;
        if (max_steps > 0 && steps >= max_steps) return 2;
        return 0;
    };
    auto limit_now = [&](int64_t inflight) { return limit_kind(inflight) != 0; };
    auto stop_now = [&](int64_t inflight) {
        if (limit_now(inflight)) return true;
        if (t->comm) return t->x_done;   // (the gap is the ranks' joint decision: x_apply)
        const double gap = tree_gap(t);
        return gap >= 0 && gap <= mip_gap;
    };
    auto batch_size = [&](int64_t inflight) {
        int64_t want = frontier_batch;
        if (node_limit > 0 && node_limit - t->evaluated - inflight < want)
            want = node_limit - t->evaluated - inflight;
        // every evaluated node may need pool rows for two children per output level (the child solved
        // in place branches too); the steps in flight have the same claim.  When the pool cannot take
        // a single node's children the search stops (status 4, stats.pool_exhausted).
        const int64_t per = 2 * (1 + (int64_t)t->dive);
        // (device finish: the steps in flight took their rows out of the free list when they were launched)
        const int64_t avail = (int64_t)t->free_slots.size() - (t->fast_ok ? 0 : per * inflight);
        // host spill: a node of the batch may come back from the host and need a row of its own besides its
        // children's (while any node is on the host, whether or not the spill is still on)
        const int64_t room = avail / (t->hs.on_host > 0 ? per + 1 : per);
        if (room < want) {
            want = room > 0 ? room : 0;
            if (want == 0 && inflight == 0) {
                t->pool_exhausted = true;
                (void)fail(ctx, MIPX_ENOMEM, "tree: node pool exhausted (search stopped; raise pool_capacity)");
            }
        }
        return (int)want;
    };
    for (;;) {
    for (;;) {
        // queue steps ahead: the first unconditionally (an empty batch launches nothing), the others only
        // with nodes to take
        while (nfl < NBUF && !tree_queue_empty(t)) {
            const int64_t fl = inflight_nodes();
            if (stop_now(fl)) break;
            if (t->hs.cap > 0) {   // host spill: rows for a whole batch before batch_size() counts them
                const int src = spill_room(t, frontier_batch, fl);
                if (src) return bail(src);
                if (t->pool_exhausted) break;
            }
            const int want = batch_size(fl);
            if (nfl > 0 && want <= 0) break;
            StepBuf &N = t->buf[next];
            int rc = tree_launch(t, N, want);
            if (rc) return bail(rc);
            if (!N.in_flight) break;
            steps++;
            nfl++;
            next = (next + 1) % NBUF;
        }
        if (nfl == 0) break;
        if (t->hook && steps > 0 && steps % t->hook_every == 0 && steps != hooked_at) {
            hooked_at = steps;  // the GPU is busy with the queued steps while the ranks exchange
            if (t->hook(t->hook_user)) hook_stop = true;
        }
        if (t->comm && steps > 0 && steps % t->x_every == 0 && steps != xchg_at) {
            xchg_at = steps;  // collect the exchange posted x_every steps ago, post the next
            const int xrc = x_tick(t, false);
            if (xrc) return xrc;
        }
        int rc = tree_finish(t, t->buf[head], overlap);
        if (rc == MIPX_OK && t->fault_step > 0 && t->steps >= t->fault_step)
            rc = fail(ctx, MIPX_EHIP, "tree: injected fault (MIPX_FAULT_STEP)");
        if (rc) return bail(rc);
        head = (head + 1) % NBUF;
        nfl--;
    }
    if (!t->comm || t->x_done) break;
    // Nothing in flight: out of open nodes, or at one of this rank's limits.  The other ranks may
    // still work: wait for them in the exchange (it blocks until every rank has posted), where open
    // nodes may arrive from a fuller rank or the joint decision to stop is taken.
    t->x_stop_flag = limit_kind(0);
    const int xrc = x_tick(t, true);
    if (xrc) return xrc;
    if (t->x_done) break;
    }
    HIP_TRY(ctx, hipStreamSynchronize(t->st3));
    HIP_TRY(ctx, hipStreamSynchronize(t->stf));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (t->comm) {
        const int xrc = x_close(t);
        if (xrc) return xrc;
    }
    t->solve_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (std::getenv("MIPX_TREE_PROFILE")) {
        const double wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        std::fprintf(stderr, "[mipx_tree] call: %lld steps in %.2f ms | pop %.2f  wait+d2h %.2f  pseudo-cost %.2f  "
                     "bookkeeping %.2f  children %.2f | lp kernel %.2f | pc: probes %.2f updates %.2f rescoring %.2f\n", (long long)steps, wall,
                     t->phase_ms[0] - ph0[0], t->phase_ms[1] - ph0[1], t->phase_ms[2] - ph0[2] + t->phase_ms[5] - ph0[5] + t->phase_ms[6] - ph0[6],
                     t->phase_ms[3] - ph0[3], t->phase_ms[4] - ph0[4], t->kernel_ms - k0,
                     t->phase_ms[5] - ph0[5], t->phase_ms[6] - ph0[6], t->phase_ms[2] - ph0[2]);
#ifdef MIPX_HOSTPROF
        std::fprintf(stderr, "[mipx_tree]   hostprof: %llu queue pushes %.1f ms (%.0f cycles each), node records %.1f ms\n",
                     g_hp_n, g_hp_push / 2.0e6, g_hp_n ? (double)g_hp_push / g_hp_n : 0.0, g_hp_rec / 2.0e6);
        g_hp_push = g_hp_rec = g_hp_n = 0;
#endif
        std::fprintf(stderr, "[mipx_tree]   popped so far by age in steps: 1:%lld 2:%lld 3:%lld 4:%lld 5:%lld 6:%lld 7+:%lld  mean depth %.1f\n",
                     (long long)t->age_hist[1], (long long)t->age_hist[2], (long long)t->age_hist[3], (long long)t->age_hist[4],
                     (long long)t->age_hist[5], (long long)t->age_hist[6], (long long)t->age_hist[7],
                     (double)t->depth_sum / (double)std::max<int64_t>(1, t->age_hist[1] + t->age_hist[2] + t->age_hist[3] + t->age_hist[4] + t->age_hist[5] + t->age_hist[6] + t->age_hist[7] + t->age_hist[0]));
        std::fprintf(stderr, "[mipx_tree]   probes: read-back %.2f  enqueue %.2f  wait %.2f  results %.2f\n",
                     t->probe_ms[0] - pr0[0], t->probe_ms[1] - pr0[1], t->probe_ms[2] - pr0[2], t->probe_ms[3] - pr0[3]);
    }
    const double gap = tree_gap(t);   // (with a communicator: of the global bounds)
    const bool nothing_open = t->comm ? t->g_counts[4] == 0 : tree_queue_empty(t);
    if (t->unbounded) t->status = 3;
    else if (nothing_open && t->primal == inf) t->status = 2;
    else if (t->primal < inf && gap >= 0 && gap <= mip_gap) t->status = 1;
    else t->status = 4;
    if (out) mipx_tree_get_stats(t, out);
    if (hook_stop) return fail(ctx, MIPX_EHOOK, "mipx_tree_solve: stopped by the step hook");
    if (t->comm && t->x_fatal) return fail(ctx, MIPX_EPEER, "mipx_tree_solve: another rank failed; the search was stopped");
    return MIPX_OK;
}

/* Re-anchoring: the first `max_nodes` open nodes in queue order each get an anchor of their own --
 * the tableau of their warm-start basis, built by one refactor-only launch from the current
 * anchors -- and their descendants inherit it (their bases stay a few pivots away from it, where
 * the root's tableau drifts further away with every level).  Every other open node goes back to
 * the problem's single anchor.  288 GB of HBM hold a million 256 x 128 anchors; 8192 take 2.1 GB. */
int mipx_tree_reanchor(mipx_tree *t, int64_t max_nodes) {
    if (!t || max_nodes < 1) return MIPX_EINVAL;
    mipx_ctx *ctx = t->ctx;
    // (with cut rounds a root that kept cut rows leaves no root anchor: the launch below then refactors
    // from the slack basis)
    if (!t->anchor_mode || (!t->anchor_set && !(t->cuts && t->evaluated > 0)))
        return fail(ctx, MIPX_EINVAL, "mipx_tree_reanchor: needs the anchor mode and a solved root");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(t->st3));
    HIP_TRY(ctx, hipStreamSynchronize(t->st2));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<int64_t> order;
    tree_queue_ids(t, order);
    if (t->cuts) {   // an anchor is a tableau of the shared rows: only nodes that carry no cut row get one
        auto plain_node = [&](int64_t id) { return t->nodes[id].ncut == 0; };
        std::stable_partition(order.begin(), order.end(), plain_node);
        int64_t plain = 0;
        for (int64_t id : order) plain += plain_node(id);
        max_nodes = std::min<int64_t>(max_nodes, plain);
    }
    const int64_t K = std::min<int64_t>(max_nodes, (int64_t)order.size());
    if (K == 0) {
        for (int64_t id : order) t->nodes[id].anchor = -1;
        return MIPX_OK;
    }
    const size_t m = t->m, n = t->n;
    double *nT = nullptr, *nvec = nullptr;
    int32_t *nidx = nullptr, *d_sl = nullptr;
    HIP_TRY(ctx, hipMalloc((void **)&nT, (size_t)K * m * n * 8));
    HIP_TRY(ctx, hipMalloc((void **)&nvec, (size_t)K * (n + 3 * m) * 8));
    HIP_TRY(ctx, hipMalloc((void **)&nidx, (size_t)K * (2 * n + m) * 4));
    HIP_TRY(ctx, hipMalloc((void **)&d_sl, (size_t)K * 8));
    std::vector<int32_t> sl(2 * (size_t)K);  // [pool rows | the anchors the nodes have now]
    for (int64_t k = 0; k < K; k++) {
        sl[(size_t)k] = t->nodes[order[(size_t)k]].slot;
        sl[(size_t)(K + k)] = t->nodes[order[(size_t)k]].anchor;
    }
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipMemcpyAsync(d_sl, sl.data(), (size_t)K * 8, hipMemcpyHostToDevice, st));
    // host spill: spilled nodes among the K are decoded into a scratch block shaped like the pool (row k for
    // the k-th node), the resident ones copied beside them -- every one of the K gets the anchor it would get
    // in a pool that never filled
    const double *src_l = t->pool_l, *src_u = t->pool_u;
    const int8_t *src_v = t->pool_v;
    double *sc_l = nullptr, *sc_u = nullptr;
    int8_t *sc_v = nullptr;
    char *sc_rec = nullptr;
    std::vector<int32_t> pos, idn;
    std::vector<int64_t> roff(1, 0);
    std::vector<char> recs;
    for (int64_t k = 0; k < K; k++) {
        if (!spilled(sl[(size_t)k])) continue;
        const SpillLoc &lc = t->hs.loc[(size_t)(-2 - sl[(size_t)k])];
        const char *src = t->hs.segs[(size_t)lc.seg].host + lc.off;
        recs.insert(recs.end(), src, src + lc.bytes);
        roff.push_back((int64_t)recs.size());
        pos.push_back((int32_t)k);
    }
    if (!pos.empty()) {
        const size_t nvs = n + (size_t)t->mrows, R = pos.size(), o_pos = (R + 1) * 8, o_rec = o_pos + (R * 4 + 7) / 8 * 8;
        HIP_TRY(ctx, hipMalloc((void **)&sc_l, (size_t)K * n * 8));
        HIP_TRY(ctx, hipMalloc((void **)&sc_u, (size_t)K * n * 8));
        HIP_TRY(ctx, hipMalloc((void **)&sc_v, (size_t)K * nvs));
        HIP_TRY(ctx, hipMalloc((void **)&sc_rec, o_rec + recs.size()));
        mipx::SpillArgs a = spill_args(t);
        a.kc = 0;   // (the K are plain nodes or no cut rounds run: only bounds and basis codes are needed)
        a.l = sc_l; a.u = sc_u; a.v = sc_v; a.ncut = nullptr; a.ids = nullptr;
        a.slot = d_sl;
        enqueue_spill_gather_rows(a, (int)K, st, t->pool_l, t->pool_u, t->pool_v);
        HIP_TRY(ctx, hipMemcpyAsync(sc_rec, roff.data(), (R + 1) * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(sc_rec + o_pos, pos.data(), R * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(sc_rec + o_rec, recs.data(), recs.size(), hipMemcpyHostToDevice, st));
        a.off = (int64_t *)sc_rec; a.slot = (const int32_t *)(sc_rec + o_pos); a.rec = sc_rec + o_rec;
        enqueue_spill_unpack(a, (int)R, st);
        HIP_TRY(ctx, hipGetLastError());
        idn.resize((size_t)K);
        for (int64_t k = 0; k < K; k++) idn[(size_t)k] = (int32_t)k;
        HIP_TRY(ctx, hipMemcpyAsync(d_sl, idn.data(), (size_t)K * 4, hipMemcpyHostToDevice, st));
        src_l = sc_l; src_u = sc_u; src_v = sc_v;
    }
    // refactor-only solves of the K nodes (from the anchors they have now), every final tableau dumped
    mipx::LpArgs a = problem_args(t->prob);
    a.l = src_l; a.u = src_u; a.vstat_in = src_v; a.slot = d_sl;
    double *gl = nullptr, *gu = nullptr;
    int8_t *gv = nullptr;
    if (t->cuts) {   // (the pool's basis rows are n + mrows wide: dense copies over the shared rows)
        HIP_TRY(ctx, hipMalloc((void **)&gl, (size_t)K * n * 8));
        HIP_TRY(ctx, hipMalloc((void **)&gu, (size_t)K * n * 8));
        HIP_TRY(ctx, hipMalloc((void **)&gv, (size_t)K * (n + m)));
        mipx::PlainGatherArgs ga;
        ga.n = (int)n; ga.m = (int)m; ga.nvs_pool = t->n + t->mrows; ga.slot = d_sl;
        ga.pool_l = src_l; ga.pool_u = src_u; ga.pool_v = src_v; ga.l = gl; ga.u = gu; ga.v = gv;
        enqueue_gather_plain_nodes(ga, (int)K, st);
        a.l = gl; a.u = gu; a.vstat_in = gv; a.slot = nullptr;
    }
    if (t->atab_T != nullptr) { a.anchor_sel = d_sl + K; a.atab_T = t->atab_T; a.atab_vec = t->atab_vec; a.atab_idx = t->atab_idx; }
    a.refactor_only = 1; a.batch = (int)K;
    a.dbg_T = nT; a.dbg_vec = nvec; a.dbg_idx = nidx; a.dbg_all = 1;
    int rc = launch_lp_any(t->prob, a, (int)K, st);
    if (rc == MIPX_OK && hipStreamSynchronize(st) != hipSuccess) rc = fail(ctx, MIPX_EHIP, "mipx_tree_reanchor: launch failed");
    (void)hipFree(d_sl);
    if (gl) { (void)hipFree(gl); (void)hipFree(gu); (void)hipFree(gv); }
    if (sc_l) { (void)hipFree(sc_l); (void)hipFree(sc_u); (void)hipFree(sc_v); (void)hipFree(sc_rec); }
    if (rc != MIPX_OK) { (void)hipFree(nT); (void)hipFree(nvec); (void)hipFree(nidx); return rc; }
    if (t->atab_T) { (void)hipFree(t->atab_T); (void)hipFree(t->atab_vec); (void)hipFree(t->atab_idx); }
    t->atab_T = nT; t->atab_vec = nvec; t->atab_idx = nidx; t->atab_count = K;
    // the old table is gone: every open node back to the root's anchor, then the K new entries
    // (the host's node records are the authority; a step uploads its batch's entries with the rows)
    for (size_t pos = 0; pos < order.size(); pos++) t->nodes[order[pos]].anchor = pos < (size_t)K ? (int32_t)pos : -1;
    return MIPX_OK;
}

int mipx_tree_set_dive(mipx_tree *t, int on) {
    if (!t) return MIPX_EINVAL;
    if (on && t->max_batch == 1)
        return fail(t->ctx, MIPX_EINVAL, "mipx_tree_set_dive: the exact mode (max_batch = 1) reproduces the "
                                         "reference's node order and cannot dive");
    if (on && t->cuts)
        return fail(t->ctx, MIPX_EINVAL, "mipx_tree_set_dive: a dive child would be solved before its parent's cut "
                                         "rounds; not available with cut rounds");
    if (on < 0 || on > kMaxDive) return fail(t->ctx, MIPX_EINVAL, "mipx_tree_set_dive: depth out of range (0..8)");
    for (const StepBuf &S : t->buf)
        if (S.in_flight) return fail(t->ctx, MIPX_EINVAL, "mipx_tree_set_dive: a step is in flight");
    t->dive = on;
    for (StepBuf &S : t->buf) layout_pack(t, S, 1 + on);
    return MIPX_OK;
}

int mipx_tree_set_step_hook(mipx_tree *t, mipx_tree_hook fn, void *user, int every_steps) {
    if (!t || (fn && every_steps < 1)) return MIPX_EINVAL;
    t->hook = fn;
    t->hook_user = user;
    t->hook_every = fn ? every_steps : 0;
    return MIPX_OK;
}

int mipx_tree_get_stats(mipx_tree *t, mipx_tree_stats *out) {
    if (!t || !out) return MIPX_EINVAL;
    out->evaluated_nodes = t->evaluated;
    out->lp_solved = t->lps;
    out->probes_solved = t->probes;
    out->pivots = t->pivots;
    out->open_nodes = (int64_t)(t->use_bq ? t->bq.size() : t->heap.size());
    out->created_nodes = (int64_t)t->nodes.size();
    out->steps = t->steps;
    out->primal_bound = t->primal;
    out->dual_bound = t->comm ? t->g_dual : tree_dual_bound(t);
    out->gap = tree_gap(t);
    out->solve_seconds = t->solve_seconds;
    out->kernel_ms = t->kernel_ms;
    out->status = t->status;
    out->has_solution = t->have_x ? 1 : 0;
    out->dives = t->dives;
    out->pool_exhausted = t->pool_exhausted ? 1 : 0;
    out->reserved = 0;
    return MIPX_OK;
}

int mipx_exchange_record_len(int n) { return n > 0 ? kRecHead + 5 * n : MIPX_EINVAL; }

int mipx_tree_exchange_record(mipx_tree *t, double *record) {
    if (!t || !record) return MIPX_EINVAL;
    if (!t->comm) return fail(t->ctx, MIPX_EINVAL, "mipx_tree_exchange_record: no communicator attached");
    x_fill_record(t);
    std::memcpy(record, t->x_rec.data(), x_rec_len(t) * 8);
    return MIPX_OK;
}

int mipx_exchange_decide(int world, int n, const double *records, double mip_gap, int allow_migration,
                         mipx_exchange_decision *out) {
    if (world < 1 || n < 1 || !records || !out) return MIPX_EINVAL;
    x_decide(world, n, records, mip_gap, allow_migration != 0, out);
    return MIPX_OK;
}

int mipx_tree_set_comm(mipx_tree *t, mipx_comm *c, int every_steps) {
    if (!t || (c && every_steps < 1)) return MIPX_EINVAL;
    if (c && c->ctx != t->ctx) return fail(t->ctx, MIPX_EINVAL, "mipx_tree_set_comm: communicator of another context");
    if (c && (t->hs.cap > 0 || t->hs.on_host > 0))
        return fail(t->ctx, MIPX_EINVAL, "mipx_tree_set_comm: not with the host spill (mipx_tree_set_host_spill)");
    if (c && t->df.on) return fail(t->ctx, MIPX_EINVAL, "mipx_tree_set_comm: not with the dual function (mipx_tree_set_dual_record)");
    if (c && t->tr.on) return fail(t->ctx, MIPX_EINVAL, "mipx_tree_set_comm: not with the tree record (mipx_tree_set_tree_record)");
    if (c && t->hr.on) return fail(t->ctx, MIPX_EINVAL, "mipx_tree_set_comm: not with the primal heuristic (mipx_tree_set_heuristic)");
    if (c && t->pg.on) return fail(t->ctx, MIPX_EINVAL, "mipx_tree_set_comm: not with the bound propagation (mipx_tree_set_propagation)");
    if (c && t->rc.on) return fail(t->ctx, MIPX_EINVAL, "mipx_tree_set_comm: not with the reduced-cost tightening (mipx_tree_set_reduced_cost)");
    if (c && t->os.on) return fail(t->ctx, MIPX_EINVAL, "mipx_tree_set_comm: not with the objective step (mipx_tree_set_objective_step)");
    t->comm = c;
    t->x_every = c ? every_steps : 0;
    if (!c) return MIPX_OK;
    const size_t n = (size_t)t->n;
    // what every rank holds at sharding time (replicated ramp-up) is counted once
    t->ramp[0] = t->evaluated; t->ramp[1] = t->lps; t->ramp[2] = t->probes; t->ramp[3] = t->pivots;
    t->pc_base.assign(4 * n, 0.0);
    t->pc_own.assign(4 * n, 0.0);
    t->pc_others.assign(4 * n, 0.0);
    for (size_t j = 0; j < n; j++) {
        t->pc_base[j] = t->cost_l[j] * (double)t->times_l[j];
        t->pc_base[n + j] = t->cost_r[j] * (double)t->times_r[j];
        t->pc_base[2 * n + j] = (double)t->times_l[j];
        t->pc_base[3 * n + j] = (double)t->times_r[j];
    }
    if (t->fast_ok) {   // (nothing is in flight between two solves: the tail version is the one every later one copies)
        HIP_TRY(t->ctx, hipStreamSynchronize(t->ctx->stream));
        HIP_TRY(t->ctx, hipStreamSynchronize(t->stf));
        HIP_TRY(t->ctx, hipMemset(tab_at(t, t->tab_tail).own, 0, 4 * n * 8));
        t->pc_others_prev.assign(4 * n, 0.0);
        t->pc_posted.assign(4 * n, 0.0);
    }
    t->g_dual = tree_dual_bound(t);
    for (int k = 0; k < 4; k++) t->g_counts[k] = t->ramp[k];
    t->g_counts[4] = tree_open_count(t);
    t->x_rounds = 0;
    t->x_done = false;
    return MIPX_OK;
}

/* Test hook: a donation of up to `amount` open nodes from this rank to ITSELF through the communicator's
 * point-to-point path -- pack kernel, ncclSend + ncclRecv to the own rank inside one ncclGroupStart /
 * ncclGroupEnd (custom transport: a device copy), unpack kernel -- so that the wrappers of a migration
 * run on RCCL on a one-GPU box.  The nodes come back under new ids in fresh pool rows; the search is
 * otherwise unchanged.  Returns the number of records moved (>= 0) or an error. */
int64_t mipx_tree_migrate_self(mipx_tree *t, int64_t amount) {
    if (!t || amount < 1) return MIPX_EINVAL;
    if (!t->comm) return fail(t->ctx, MIPX_EINVAL, "mipx_tree_migrate_self: no communicator attached");
    if (t->cuts && t->cm_rows == 0)
        return fail(t->ctx, MIPX_EINVAL, "mipx_tree_migrate_self: cut rounds without cut migration (mipx_tree_set_cut_migration)");
    for (const StepBuf &S : t->buf)
        if (S.in_flight) return fail(t->ctx, MIPX_EINVAL, "mipx_tree_migrate_self: a step is in flight");
    mipx_comm *c = t->comm;
    mipx_ctx *ctx = t->ctx;
    if (amount > kMaxMigrate) amount = kMaxMigrate;
    const int64_t ctab = t->cuts ? mig_table_rows((double)(t->cm_rows - t->cm_used), amount, t->kc) : 0;
    const MigLayout L = mig_layout(t, amount, ctab);
    const size_t half = (L.bytes + 255) / 256 * 256;
    char *msg = nullptr;
    int rc = comm_msg_buffer(c, 2 * half + L.scratch, &msg);
    if (rc) return rc;
    int32_t *d_slots = (int32_t *)(msg + 2 * half);
    std::vector<int32_t> slots;
    int64_t sent = 0, got = 0, rows = 0;
    const int keep_batch = t->x_batch;
    t->x_batch = 0;   // (a test may move every open node)
    if (L.kc > 0) rc = mig_pack_cuts(t, L, msg, d_slots, amount, slots, &sent, &rows);
    else rc = mig_pack(t, L, msg, d_slots, amount, slots, &sent);
    t->x_batch = keep_batch;
    if (rc) return rc;
    if ((rc = comm_sendrecv_self(c, msg, msg + half, L.bytes))) return rc;
    for (int32_t sl : slots) t->free_slots.push_back(sl);
    if (L.kc > 0) rc = mig_unpack_cuts(t, L, msg + half, d_slots, amount, &got);
    else rc = mig_unpack(t, L, msg + half, d_slots, amount, &got);
    if (rc) return rc;
    if (got != sent) return fail(ctx, MIPX_EHIP, "mipx_tree_migrate_self: the count did not survive the round trip");
    t->nodes_sent += sent;
    t->nodes_received += got;
    return got;
}

int mipx_tree_global_stats(mipx_tree *t, mipx_tree_global_stats_t *out) {
    if (!t || !out) return MIPX_EINVAL;
    out->primal_bound = t->primal;
    out->dual_bound = t->comm ? t->g_dual : tree_dual_bound(t);
    out->gap = tree_gap(t);
    if (t->comm) {
        out->evaluated_nodes = t->g_counts[0]; out->lp_solved = t->g_counts[1];
        out->probes_solved = t->g_counts[2]; out->pivots = t->g_counts[3]; out->open_nodes = t->g_counts[4];
    } else {
        out->evaluated_nodes = t->evaluated; out->lp_solved = t->lps; out->probes_solved = t->probes;
        out->pivots = t->pivots; out->open_nodes = tree_open_count(t);
    }
    out->exchanges = t->x_rounds;
    out->nodes_sent = t->nodes_sent;
    out->nodes_received = t->nodes_received;
    out->world = t->comm ? t->comm->world : 1;
    out->incumbent_rank = t->comm ? t->g_inc_rank : (t->have_x ? 0 : -1);
    return MIPX_OK;
}

int mipx_tree_kernel_ms(mipx_tree *t, double out[4]) {
    if (!t || !out) return MIPX_EINVAL;
    out[0] = t->kernel_ms; out[1] = t->k2_ms; out[2] = t->k3_ms; out[3] = 0.0;
    return MIPX_OK;
}

int mipx_tree_cut_stats(mipx_tree *t, int64_t out[8]) {
    if (!t || !out) return MIPX_EINVAL;
    for (int k = 0; k < 8; k++) out[k] = t->cut_totals[k];
    return MIPX_OK;
}

int mipx_tree_solution(mipx_tree *t, double *x) {
    if (!t || !x) return MIPX_EINVAL;
    if (!t->have_x) return fail(t->ctx, MIPX_EINVAL, "mipx_tree_solution: no incumbent");
    std::memcpy(x, t->best_x.data(), (size_t)t->n * 8);
    return MIPX_OK;
}

int mipx_tree_pseudo_costs(mipx_tree *t, double *cost_l, double *cost_r, int32_t *times_l,
                           int32_t *times_r) {
    if (!t || !cost_l || !cost_r || !times_l || !times_r) return MIPX_EINVAL;
    std::memcpy(cost_l, t->cost_l.data(), (size_t)t->n * 8);
    std::memcpy(cost_r, t->cost_r.data(), (size_t)t->n * 8);
    std::memcpy(times_l, t->times_l.data(), (size_t)t->n * 4);
    std::memcpy(times_r, t->times_r.data(), (size_t)t->n * 4);
    return MIPX_OK;
}

/* Replace the pseudo-cost table (multi-GPU: the ranks all-reduce their updates -- the table is a
 * running mean, hence sum-decomposable -- and install the merged table). */
int mipx_tree_set_pseudo_costs(mipx_tree *t, const double *cost_l, const double *cost_r,
                               const int32_t *times_l, const int32_t *times_r) {
    if (!t || !cost_l || !cost_r || !times_l || !times_r) return MIPX_EINVAL;
    std::memcpy(t->cost_l.data(), cost_l, (size_t)t->n * 8);
    std::memcpy(t->cost_r.data(), cost_r, (size_t)t->n * 8);
    std::memcpy(t->times_l.data(), times_l, (size_t)t->n * 4);
    std::memcpy(t->times_r.data(), times_r, (size_t)t->n * 4);
    for (int j = 0; j < t->n; j++) t->has_entry[j] = (times_l[j] > 0 || times_r[j] > 0) ? 1 : 0;
    t->table_dirty = true;
    t->times_dirty = true;
    return MIPX_OK;
}

/* Copy the records (bounds + warm-start basis) of up to max_nodes open nodes, in queue-array
 * order, to host buffers without removing them; returns how many were copied. */
int64_t mipx_tree_peek_open(mipx_tree *t, int64_t max_nodes, double *l, double *u, int8_t *vstat,
                            double *dual_bound) {
    if (!t || max_nodes < 0) return MIPX_EINVAL;
    mipx_ctx *ctx = t->ctx;
    const size_t n = t->n, nv = t->n + t->m, nvs = (size_t)t->n + t->mrows;   // (cut rows of the basis are not copied)
    int64_t k = 0;
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return MIPX_EHIP;
    std::vector<int64_t> order;
    tree_queue_ids(t, order);
    for (size_t pos = 0; pos < order.size() && k < max_nodes; pos++, k++) {
        const NodeRec &nd = t->nodes[order[pos]];
        if (dual_bound) dual_bound[k] = nd.dual_bound;
        if (spilled(nd.slot)) {   // (decoded from its compact record)
            std::vector<int8_t> row(vstat ? nvs : 0);
            spill_decode(t, nd.slot, l ? l + k * n : nullptr, u ? u + k * n : nullptr, vstat ? row.data() : nullptr, nullptr);
            if (vstat) std::memcpy(vstat + k * nv, row.data(), nv);
            continue;
        }
        const size_t s = (size_t)nd.slot;
        if (l && hipMemcpy(l + k * n, t->pool_l + s * n, n * 8, hipMemcpyDeviceToHost) != hipSuccess) return MIPX_EHIP;
        if (u && hipMemcpy(u + k * n, t->pool_u + s * n, n * 8, hipMemcpyDeviceToHost) != hipSuccess) return MIPX_EHIP;
        if (vstat && hipMemcpy(vstat + k * nv, t->pool_v + s * nvs, nv, hipMemcpyDeviceToHost) != hipSuccess) return MIPX_EHIP;
    }
    return k;
}

/* Anchor-table entries of the open nodes, in the order of mipx_tree_peek_open (-1: the single anchor). */
int64_t mipx_tree_peek_anchors(mipx_tree *t, int64_t max_nodes, int32_t *anchor) {
    if (!t || max_nodes < 0 || !anchor) return MIPX_EINVAL;
    std::vector<int64_t> order;
    tree_queue_ids(t, order);
    int64_t k = 0;
    for (size_t pos = 0; pos < order.size() && k < max_nodes; pos++, k++)
        anchor[k] = t->atab_T ? t->nodes[order[pos]].anchor : -1;
    return k;
}

/* The anchor table of mipx_tree_reanchor: returns the number of entries; copies them to HOST buffers
 * where given (T: count x m x n, vec: count x (n + 3m), idx: count x (2n + m)). */
int64_t mipx_tree_anchor_table(mipx_tree *t, double *T, double *vec, int32_t *idx) {
    if (!t) return MIPX_EINVAL;
    const size_t K = (size_t)t->atab_count, m = t->m, n = t->n;
    if (K == 0 || !t->atab_T) return 0;
    if (hipStreamSynchronize(t->ctx->stream) != hipSuccess) return MIPX_EHIP;
    if (T && hipMemcpy(T, t->atab_T, K * m * n * 8, hipMemcpyDeviceToHost) != hipSuccess) return MIPX_EHIP;
    if (vec && hipMemcpy(vec, t->atab_vec, K * (n + 3 * m) * 8, hipMemcpyDeviceToHost) != hipSuccess) return MIPX_EHIP;
    if (idx && hipMemcpy(idx, t->atab_idx, K * (2 * n + m) * 4, hipMemcpyDeviceToHost) != hipSuccess) return MIPX_EHIP;
    return (int64_t)K;
}

/* Multi-GPU sharding: after a replicated, deterministic ramp-up every rank
 * keeps the open nodes whose position in the queue array is congruent to its rank and drops the
 * others (they live on the other ranks).  The dual bound of the whole tree is then the MIN over
 * ranks of mipx_tree_stats.dual_bound. */
int mipx_tree_keep_shard(mipx_tree *t, int rank, int world) {
    if (!t || world < 1 || rank < 0 || rank >= world) return MIPX_EINVAL;
    std::vector<int64_t> old;
    tree_queue_ids(t, old);
    t->heap.h.clear();
    t->bq.clear();
    while (!t->open_bounds.empty()) t->open_bounds.pop();
    for (size_t pos = 0; pos < old.size(); pos++) {
        const int64_t id = old[pos];
        if (t->search != 0) t->is_open[id] = 0;
        if ((int)(pos % (size_t)world) == rank) {
            tree_push(t, id);
        } else {
            const int32_t sl = t->nodes[id].slot;
            if (spilled(sl)) spill_release(t, sl);
            else t->free_slots.push_back(sl);
            t->nodes[id].slot = -1;
        }
    }
    if (rank != 0) t->closed_min = std::numeric_limits<double>::infinity();  // counted once, on rank 0
    return MIPX_OK;
}

int64_t mipx_tree_trace_cuts(mipx_tree *t, int64_t capacity, int32_t *counters) {
    if (!t) return MIPX_EINVAL;
    const int64_t have = (int64_t)t->tr_cuts.size() / 8;
    const int64_t k = have < capacity ? have : capacity;
    if (counters && k > 0) std::memcpy(counters, t->tr_cuts.data(), (size_t)k * 8 * 4);
    return have;
}

/* Test hooks of the cut rounds: the open nodes' ids, cut lists (ids into the cut store) and the basis
 * codes of their cut rows, in the order of mipx_tree_peek_open; and the cut store itself. */
int64_t mipx_tree_peek_cuts(mipx_tree *t, int64_t max_nodes, int64_t *node_id, int32_t *ncut, int32_t *cut_ids,
                            int8_t *cut_vstat) {
    if (!t || max_nodes < 0) return MIPX_EINVAL;
    mipx_ctx *ctx = t->ctx;
    if (hipStreamSynchronize(t->st3) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) return MIPX_EHIP;
    std::vector<int64_t> order;
    tree_queue_ids(t, order);
    const size_t n = t->n, m = t->m, nvs = n + (size_t)t->mrows, K = (size_t)t->kc;
    int64_t k = 0;
    for (size_t pos = 0; pos < order.size() && k < max_nodes; pos++, k++) {
        const NodeRec &nd = t->nodes[order[pos]];
        const size_t s = (size_t)nd.slot;
        if (node_id) node_id[k] = order[pos];
        if (ncut) ncut[k] = t->cuts ? nd.ncut : 0;
        if (t->cuts && K > 0 && spilled(nd.slot)) {   // (decoded from its compact record)
            std::vector<int8_t> row(nvs);
            std::vector<int32_t> idl(K, 0);
            spill_decode(t, nd.slot, nullptr, nullptr, row.data(), idl.data());
            if (cut_ids) std::memcpy(cut_ids + k * K, idl.data(), K * 4);
            if (cut_vstat) std::memcpy(cut_vstat + k * K, row.data() + n + m, K);
        } else if (t->cuts && K > 0) {
            if (cut_ids && hipMemcpy(cut_ids + k * K, t->pool_ids + s * K, K * 4, hipMemcpyDeviceToHost) != hipSuccess) return MIPX_EHIP;
            if (cut_vstat && hipMemcpy(cut_vstat + k * K, t->pool_v + s * nvs + n + m, K, hipMemcpyDeviceToHost) != hipSuccess) return MIPX_EHIP;
        }
    }
    return k;
}

int64_t mipx_tree_cut_store(mipx_tree *t, int64_t capacity, double *pi, double *pi0) {
    if (!t) return MIPX_EINVAL;
    if (!t->cuts) return 0;
    if (hipStreamSynchronize(t->ctx->stream) != hipSuccess) return MIPX_EHIP;
    int32_t cnt = 0;
    if (hipMemcpy(&cnt, t->store_count, 4, hipMemcpyDeviceToHost) != hipSuccess) return MIPX_EHIP;
    const int64_t own = t->store_cap - t->cm_rows;   // (the rank's own appends: not the migration region)
    int64_t have = cnt < own ? cnt : own;
    const int64_t k = have < capacity ? have : capacity;
    if (pi && k > 0 && hipMemcpy(pi, t->store_pi, (size_t)k * t->n * 8, hipMemcpyDeviceToHost) != hipSuccess) return MIPX_EHIP;
    if (pi0 && k > 0 && hipMemcpy(pi0, t->store_pi0, (size_t)k * 8, hipMemcpyDeviceToHost) != hipSuccess) return MIPX_EHIP;
    return have;
}

int mipx_tree_cut_rows_per_node(const mipx_tree *t) { return t ? t->kc : MIPX_EINVAL; }

int64_t mipx_tree_trace(mipx_tree *t, int64_t capacity, int64_t *node_id, int32_t *lp_status,
                        int32_t *branch_var, double *objective) {
    if (!t) return MIPX_EINVAL;
    const int64_t k = (int64_t)t->tr_id.size() < capacity ? (int64_t)t->tr_id.size() : capacity;
    for (int64_t i = 0; i < k; i++) {
        if (node_id) node_id[i] = t->tr_id[i];
        if (lp_status) lp_status[i] = t->tr_status[i];
        if (branch_var) branch_var[i] = t->tr_bidx[i];
        if (objective) objective[i] = t->tr_obj[i];
    }
    return (int64_t)t->tr_id.size();
}

int mipx_tree_set_host_spill(mipx_tree *t, int64_t max_host_bytes) {
    if (!t) return MIPX_EINVAL;
    mipx_ctx *ctx = t->ctx;
    if (max_host_bytes < 0) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_host_spill: negative byte cap");
    if (max_host_bytes == 0) { t->hs.cap = 0; return MIPX_OK; }   // (nodes already on the host still come back)
    if (t->comm) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_host_spill: not with a communicator");
    if (t->capacity < 2 * spill_headroom(t) + 1)
        return fail(ctx, MIPX_EINVAL, "mipx_tree_set_host_spill: pool_capacity below the minimum (2 x headroom + 1, mipx_spill.h)");
    HostSpill &h = t->hs;
    if (!h.st) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        const size_t n = (size_t)t->n, MB = (size_t)t->max_batch;
        HIP_TRY(ctx, hipStreamCreateWithFlags(&h.st, hipStreamNonBlocking));
        int rc = dmalloc(ctx, &h.d_root, 2 * n);
        if (rc) return rc;
        HIP_TRY(ctx, hipMemcpy(h.d_root, t->root_l.data(), n * 8, hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(h.d_root + n, t->root_u.data(), n * 8, hipMemcpyHostToDevice));
        // reload staging per step buffer: [offsets | rows | max_batch records of the largest size]
        h.rl_cap = (MB + 1) * 8 + (MB * 4 + 7) / 8 * 8 + MB * (size_t)spill_max_record(t);
        for (StepBuf &S : t->buf) {
            HIP_TRY(ctx, hipHostMalloc((void **)&S.h_rl, h.rl_cap, hipHostMallocDefault));
            if ((rc = dmalloc(ctx, &S.d_rl, h.rl_cap))) return rc;
        }
    }
    h.cap = max_host_bytes;
    return MIPX_OK;
}

int mipx_tree_set_cut_migration(mipx_tree *t, int64_t rows) {
    if (!t) return MIPX_EINVAL;
    mipx_ctx *ctx = t->ctx;
    if (!t->cuts) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_cut_migration: the tree runs no cut rounds");
    if (rows < 0) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_cut_migration: negative rows");
    for (const StepBuf &S : t->buf)
        if (S.in_flight) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_cut_migration: a step is in flight");
    if (rows == t->cm_rows) return MIPX_OK;
    if (t->cm_used > 0)
        return fail(ctx, MIPX_EINVAL, "mipx_tree_set_cut_migration: the region holds migrated cut rows already");
    if (rows >= t->store_cap)
        return fail(ctx, MIPX_EINVAL, "mipx_tree_set_cut_migration: the region must leave rows of the cut store (store_capacity)");
    if (rows > 0) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        int32_t cnt = 0;
        HIP_TRY(ctx, hipMemcpy(&cnt, t->store_count, 4, hipMemcpyDeviceToHost));
        if ((int64_t)cnt > t->store_cap - rows)
            return fail(ctx, MIPX_EINVAL, "mipx_tree_set_cut_migration: the cut store holds more than store_capacity - rows cuts");
    }
    t->cm_rows = rows;
    return MIPX_OK;
}

int mipx_tree_cut_rows(mipx_tree *t, int64_t count, const int32_t *ids, double *pi, double *pi0) {
    if (!t || count < 0 || (count > 0 && !ids)) return MIPX_EINVAL;
    mipx_ctx *ctx = t->ctx;
    if (!t->cuts) return fail(ctx, MIPX_EINVAL, "mipx_tree_cut_rows: the tree runs no cut rounds");
    for (int64_t k = 0; k < count; k++)
        if (ids[k] < 0 || ids[k] >= t->store_cap) return fail(ctx, MIPX_EINVAL, "mipx_tree_cut_rows: id outside the cut store");
    if (count == 0) return MIPX_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const size_t n = (size_t)t->n;
    char *blk = nullptr;   // [ids | pi | pi0]
    const size_t ids_b = pad8((size_t)count * 4);
    HIP_TRY(ctx, hipMalloc((void **)&blk, ids_b + (size_t)count * (n + 1) * 8));
    mipx::CutMigArgs ca;
    ca.n = t->n; ca.src = (const int32_t *)blk; ca.store_pi = t->store_pi; ca.store_pi0 = t->store_pi0;
    ca.tab_pi = (double *)(blk + ids_b); ca.tab_pi0 = ca.tab_pi + (size_t)count * n;
    int rc = MIPX_OK;
    if (hipMemcpy(blk, ids, (size_t)count * 4, hipMemcpyHostToDevice) != hipSuccess) rc = MIPX_EHIP;
    if (!rc) {
        enqueue_cutmig_gather(ca, (int)count, ctx->stream);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) rc = MIPX_EHIP;
    }
    if (!rc && pi && hipMemcpy(pi, ca.tab_pi, (size_t)count * n * 8, hipMemcpyDeviceToHost) != hipSuccess) rc = MIPX_EHIP;
    if (!rc && pi0 && hipMemcpy(pi0, ca.tab_pi0, (size_t)count * 8, hipMemcpyDeviceToHost) != hipSuccess) rc = MIPX_EHIP;
    (void)hipFree(blk);
    return rc ? fail(ctx, rc, "mipx_tree_cut_rows: HIP error") : MIPX_OK;
}

int mipx_tree_cut_migration_stats(mipx_tree *t, int64_t out[4]) {
    if (!t || !out) return MIPX_EINVAL;
    out[0] = t->cm_nodes_sent; out[1] = t->cm_rows_sent; out[2] = t->cm_rows_received; out[3] = t->cm_used;
    return MIPX_OK;
}

int mipx_tree_spill_stats(mipx_tree *t, int64_t out[8]) {
    if (!t || !out) return MIPX_EINVAL;
    const HostSpill &h = t->hs;
    out[0] = h.spilled; out[1] = h.reloaded; out[2] = h.on_host; out[3] = h.bytes; out[4] = h.peak; out[5] = h.events;
    out[6] = (int64_t)h.spill_us; out[7] = (int64_t)h.reload_us;
    return MIPX_OK;
}

}  // extern "C"

#include "dualfn_api.hip.h"
#include "dualfn_batch_api.hip.h"
#include "treerec_api.hip.h"
#include "cglp_api.hip.h"
#include "restart_api.hip.h"
#include "noderows_api.hip.h"
#include "supportkernels_api.hip.h"
#include "heur_api.hip.h"
#include "prop_api.hip.h"
#include "rcfix_api.hip.h"
#include "lsearch_api.hip.h"
#include "fixprop_api.hip.h"
#include "wrepair_api.hip.h"
#include "cube_api.hip.h"
#include "complete_api.hip.h"
#include "lpdive_api.hip.h"
#include "objstep_api.hip.h"
#include "finish_api.hip.h"
#include "cutround_api.hip.h"
