// noderows_api.hip.h -- the C entries of include/mipx_noderows.h (included at the end of tree_engine.hip.h, whose
// enqueue_* functions are the one launch site of each kernel): the kernels that move node rows on a caller's pools.
// Test scaffolding: no product code calls them.

namespace {

// every index of a list inside [lo, rows)
template <typename T>
bool nr_rows_ok(const T *idx, size_t count, int64_t rows, int64_t lo = 0) {
    for (size_t e = 0; e < count; e++)
        if (idx[e] < lo || idx[e] >= rows) return false;
    return true;
}

// no row >= 0 named twice (the kernels' blocks or waves would race for it)
bool nr_distinct(const int32_t *idx, size_t count) {
    std::vector<int32_t> s;
    for (size_t e = 0; e < count; e++)
        if (idx[e] >= 0) s.push_back(idx[e]);
    std::sort(s.begin(), s.end());
    return std::adjacent_find(s.begin(), s.end()) == s.end();
}

// in and out: uploaded whole, copied back whole
size_t nr_inout(Staging &S, void *p, size_t bytes) {
    const size_t o = S.in(p, bytes);
    S.down(p, o, bytes);
    return o;
}

int nr_launched(Staging &S, int rc) {
    if (rc != MIPX_OK) return rc;
    if (hipError_t e = hipGetLastError()) return S.err("launch", e);
    return MIPX_OK;
}

// the lineage entries' shared checks and the mirror as the engine's 16-byte entries
int nr_lineage_check(mipx_ctx *ctx, const char *who, int n, int nv, int64_t nodes_count, const int32_t *parent,
                     const int32_t *vd, const double *val, int count, const int64_t *ids, const double *root_l,
                     const double *root_u, std::vector<mipx::TrNode> &mirror) {
    if (n < 1 || n > 1024 || nv < 1) return refuse(ctx, who, "n outside 1 .. 1024, or nv < 1");
    if (count < 0 || nodes_count < 0) return refuse(ctx, who, "count or nodes_count < 0");
    if (!root_l || !root_u || (nodes_count > 0 && (!parent || !vd || !val)) || (count > 0 && !ids))
        return refuse(ctx, who, "a null argument");
    for (int k = 0; k < count; k++)
        if (ids[k] < 0) return refuse(ctx, who, "an id < 0");
    mirror.resize((size_t)nodes_count);
    for (size_t i = 0; i < mirror.size(); i++) { mirror[i].parent = parent[i]; mirror[i].vd = vd[i]; mirror[i].val = val[i]; }
    return MIPX_OK;
}

}  // namespace

extern "C" {

int mipx_noderows_children(mipx_ctx *ctx, int n, int m, int mstride, int kc, int count, int src_rows,
                           const double *src_l, const double *src_u, int batch_rows, const double *x,
                           const int8_t *vstat, const int32_t *src_ncut, const int32_t *src_ids,
                           const int32_t *parent_slot, const int32_t *parent_pos, const int32_t *var,
                           const int32_t *child_slot, int dst_rows, double *dst_l, double *dst_u, int8_t *dst_v,
                           int32_t *dst_ncut, int32_t *dst_ids) {
    if (!ctx) return MIPX_EINVAL;
    const char *who = "mipx_noderows_children";
    if (n < 1 || m < 1 || src_rows < 1 || batch_rows < 1 || dst_rows < 1 || count < 0)
        return refuse(ctx, who, "n, m, src_rows, batch_rows or dst_rows < 1, or count < 0");
    if (mstride < 0 || kc < 0 || kc > mipx::kMaxNodeCuts) return refuse(ctx, who, "mstride < 0, or kc outside 0 .. 64");
    const bool cut = mstride > 0;
    if (!cut && (kc != 0 || src_ncut || src_ids || dst_ncut || dst_ids))
        return refuse(ctx, who, "plain mode (mstride = 0) with kc != 0 or a cut array");
    if (cut && (int64_t)m + kc > mstride) return refuse(ctx, who, "m + kc > mstride");
    if (!src_l || !src_u || !x || !vstat || !dst_l || !dst_u || !dst_v ||
        (count > 0 && (!parent_slot || !parent_pos || !var || !child_slot)) ||
        (cut && (!src_ncut || !dst_ncut || (kc > 0 && (!src_ids || !dst_ids)))))
        return refuse(ctx, who, "a null argument");
    const size_t cnt = (size_t)count;
    if (!nr_rows_ok(parent_slot, cnt, src_rows)) return refuse(ctx, who, "a parent_slot outside the source pool");
    if (!nr_rows_ok(parent_pos, cnt, batch_rows)) return refuse(ctx, who, "a parent_pos outside the batch");
    if (!nr_rows_ok(var, cnt, n)) return refuse(ctx, who, "a var outside 0 .. n-1");
    if (!nr_rows_ok(child_slot, 2 * cnt, dst_rows)) return refuse(ctx, who, "a child_slot outside the destination pool");
    if (!nr_distinct(child_slot, 2 * cnt)) return refuse(ctx, who, "two equal child slots");
    for (size_t p = 0; cut && p < cnt; p++)
        if (src_ncut[parent_pos[p]] < 0 || src_ncut[parent_pos[p]] > kc) return refuse(ctx, who, "a src_ncut outside 0 .. kc");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)n, vs = nn + (size_t)(cut ? mstride : m), SR = (size_t)src_rows, BR = (size_t)batch_rows,
                 DR = (size_t)dst_rows, K = (size_t)kc;
    Staging S(ctx, who);
    const size_t o_sl = S.in(src_l, SR * nn * 8), o_su = S.in(src_u, SR * nn * 8), o_x = S.in(x, BR * nn * 8),
                 o_vs = S.in(vstat, BR * vs), o_sn = S.in(src_ncut, BR * 4), o_si = S.in(src_ids, BR * K * 4),
                 o_ps = S.in(parent_slot, cnt * 4), o_pp = S.in(parent_pos, cnt * 4), o_var = S.in(var, cnt * 4),
                 o_cs = S.in(child_slot, 2 * cnt * 4);
    const size_t o_dl = nr_inout(S, dst_l, DR * nn * 8), o_du = nr_inout(S, dst_u, DR * nn * 8), o_dv = nr_inout(S, dst_v, DR * vs),
                 o_dn = nr_inout(S, dst_ncut, DR * 4), o_di = nr_inout(S, dst_ids, DR * K * 4);
    int rc = S.alloc();
    if (rc == MIPX_OK) rc = S.upload();
    if (rc == MIPX_OK && count > 0) {
        mipx::ChildArgs a;
        a.n = n; a.m = m;
        a.src_l = S.at<const double>(o_sl); a.src_u = S.at<const double>(o_su); a.x = S.at<const double>(o_x);
        a.vstat = S.at<const int8_t>(o_vs); a.parent_slot = S.at<const int32_t>(o_ps); a.parent_pos = S.at<const int32_t>(o_pp);
        a.var = S.at<const int32_t>(o_var); a.child_slot = S.at<const int32_t>(o_cs);
        a.dst_l = S.at<double>(o_dl); a.dst_u = S.at<double>(o_du); a.dst_v = S.at<int8_t>(o_dv);
        if (cut) {
            a.mstride = mstride; a.kc = kc;
            a.src_ncut = S.at<const int32_t>(o_sn); a.src_ids = S.at<const int32_t>(o_si);
            a.dst_ncut = S.at<int32_t>(o_dn); a.dst_ids = S.at<int32_t>(o_di);
        }
        enqueue_make_children(a, count, ctx->stream);
        rc = nr_launched(S, rc);
    }
    return S.finish(rc);
}

int mipx_noderows_pack(mipx_ctx *ctx, int n, int nvs, int count, const int32_t *slot, int pool_rows,
                       const double *pool_l, const double *pool_u, const int8_t *pool_v, void *msg) {
    if (!ctx) return MIPX_EINVAL;
    const char *who = "mipx_noderows_pack";
    if (n < 1 || nvs < 1 || pool_rows < 1 || count < 0) return refuse(ctx, who, "n, nvs or pool_rows < 1, or count < 0");
    if (!pool_l || !pool_u || !pool_v || (count > 0 && (!slot || !msg))) return refuse(ctx, who, "a null argument");
    if (!nr_rows_ok(slot, (size_t)count, pool_rows)) return refuse(ctx, who, "a slot outside the pool");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)n, nv = (size_t)nvs, PR = (size_t)pool_rows, cnt = (size_t)count, rowbytes = pad8(16 * nn + nv);
    Staging S(ctx, who);
    const size_t o_sl = S.in(slot, cnt * 4), o_l = S.in(pool_l, PR * nn * 8), o_u = S.in(pool_u, PR * nn * 8),
                 o_v = S.in(pool_v, PR * nv), o_msg = nr_inout(S, msg, cnt * rowbytes);
    int rc = S.alloc();
    if (rc == MIPX_OK) rc = S.upload();
    if (rc == MIPX_OK && count > 0) {
        mipx::PackArgs a;
        a.n = n; a.nvs = nvs; a.rowbytes = rowbytes; a.slot = S.at<const int32_t>(o_sl);
        a.pool_l = S.at<double>(o_l); a.pool_u = S.at<double>(o_u); a.pool_v = S.at<int8_t>(o_v); a.msg = S.at<char>(o_msg);
        enqueue_pack_nodes(a, count, ctx->stream);
        rc = nr_launched(S, rc);
    }
    return S.finish(rc);
}

int mipx_noderows_unpack(mipx_ctx *ctx, int n, int nvs, int count, const int32_t *slot, const void *msg, int pool_rows,
                         double *pool_l, double *pool_u, int8_t *pool_v) {
    if (!ctx) return MIPX_EINVAL;
    const char *who = "mipx_noderows_unpack";
    if (n < 1 || nvs < 1 || pool_rows < 1 || count < 0) return refuse(ctx, who, "n, nvs or pool_rows < 1, or count < 0");
    if (!pool_l || !pool_u || !pool_v || (count > 0 && (!slot || !msg))) return refuse(ctx, who, "a null argument");
    if (!nr_rows_ok(slot, (size_t)count, pool_rows)) return refuse(ctx, who, "a slot outside the pool");
    if (!nr_distinct(slot, (size_t)count)) return refuse(ctx, who, "two equal slots");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)n, nv = (size_t)nvs, PR = (size_t)pool_rows, cnt = (size_t)count, rowbytes = pad8(16 * nn + nv);
    Staging S(ctx, who);
    const size_t o_sl = S.in(slot, cnt * 4), o_msg = S.in(msg, cnt * rowbytes), o_l = nr_inout(S, pool_l, PR * nn * 8),
                 o_u = nr_inout(S, pool_u, PR * nn * 8), o_v = nr_inout(S, pool_v, PR * nv);
    int rc = S.alloc();
    if (rc == MIPX_OK) rc = S.upload();
    if (rc == MIPX_OK && count > 0) {
        mipx::PackArgs a;
        a.n = n; a.nvs = nvs; a.rowbytes = rowbytes; a.slot = S.at<const int32_t>(o_sl);
        a.pool_l = S.at<double>(o_l); a.pool_u = S.at<double>(o_u); a.pool_v = S.at<int8_t>(o_v); a.msg = S.at<char>(o_msg);
        enqueue_unpack_nodes(a, count, ctx->stream);
        rc = nr_launched(S, rc);
    }
    return S.finish(rc);
}

int mipx_noderows_gather_plain(mipx_ctx *ctx, int n, int m, int nvs_pool, int count, const int32_t *slot, int pool_rows,
                               const double *pool_l, const double *pool_u, const int8_t *pool_v, double *l, double *u,
                               int8_t *v) {
    if (!ctx) return MIPX_EINVAL;
    const char *who = "mipx_noderows_gather_plain";
    if (n < 1 || m < 1 || pool_rows < 1 || count < 0) return refuse(ctx, who, "n, m or pool_rows < 1, or count < 0");
    if ((int64_t)nvs_pool < (int64_t)n + m) return refuse(ctx, who, "nvs_pool < n + m");
    if (!pool_l || !pool_u || !pool_v || (count > 0 && (!slot || !l || !u || !v))) return refuse(ctx, who, "a null argument");
    if (!nr_rows_ok(slot, (size_t)count, pool_rows)) return refuse(ctx, who, "a slot outside the pool");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)n, nv = nn + (size_t)m, PR = (size_t)pool_rows, cnt = (size_t)count;
    Staging S(ctx, who);
    const size_t o_sl = S.in(slot, cnt * 4), o_pl = S.in(pool_l, PR * nn * 8), o_pu = S.in(pool_u, PR * nn * 8),
                 o_pv = S.in(pool_v, PR * (size_t)nvs_pool), o_l = nr_inout(S, l, cnt * nn * 8), o_u = nr_inout(S, u, cnt * nn * 8),
                 o_v = nr_inout(S, v, cnt * nv);
    int rc = S.alloc();
    if (rc == MIPX_OK) rc = S.upload();
    if (rc == MIPX_OK && count > 0) {
        mipx::PlainGatherArgs a;
        a.n = n; a.m = m; a.nvs_pool = nvs_pool; a.slot = S.at<const int32_t>(o_sl);
        a.pool_l = S.at<const double>(o_pl); a.pool_u = S.at<const double>(o_pu); a.pool_v = S.at<const int8_t>(o_pv);
        a.l = S.at<double>(o_l); a.u = S.at<double>(o_u); a.v = S.at<int8_t>(o_v);
        enqueue_gather_plain_nodes(a, count, ctx->stream);
        rc = nr_launched(S, rc);
    }
    return S.finish(rc);
}

int mipx_noderows_lineage_bounds(mipx_ctx *ctx, int n, int nv, int64_t nodes_count, const int32_t *parent,
                                 const int32_t *vd, const double *val, int count, const int64_t *ids,
                                 const double *root_l, const double *root_u, const int8_t *root_v, double *out_l,
                                 double *out_u, int8_t *out_v) {
    if (!ctx) return MIPX_EINVAL;
    const char *who = "mipx_noderows_lineage_bounds";
    std::vector<mipx::TrNode> mirror;
    if (int rc = nr_lineage_check(ctx, who, n, nv, nodes_count, parent, vd, val, count, ids, root_l, root_u, mirror)) return rc;
    if (count > 0 && (!out_l || !out_u || !out_v)) return refuse(ctx, who, "a null argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)n, vv = (size_t)nv, cnt = (size_t)count;
    Staging S(ctx, who);
    const size_t o_nd = S.in(mirror.data(), mirror.size() * sizeof(mipx::TrNode)), o_id = S.in(ids, cnt * 8),
                 o_rl = S.in(root_l, nn * 8), o_ru = S.in(root_u, nn * 8), o_rv = S.in(root_v, vv),
                 o_l = nr_inout(S, out_l, cnt * nn * 8), o_u = nr_inout(S, out_u, cnt * nn * 8), o_v = nr_inout(S, out_v, cnt * vv);
    int rc = S.alloc();
    if (rc == MIPX_OK) rc = S.upload();
    for (int64_t k0 = 0; rc == MIPX_OK && k0 < count; k0 += kTrChunk) {
        mipx::TrBoundsArgs a;
        a.n = n; a.nv = nv; a.nodes_count = nodes_count; a.nodes = S.at<const mipx::TrNode>(o_nd);
        a.ids = S.at<const int64_t>(o_id) + k0;
        a.root_l = S.at<const double>(o_rl); a.root_u = S.at<const double>(o_ru);
        a.root_v = root_v ? S.at<const int8_t>(o_rv) : nullptr;
        a.out_l = S.at<double>(o_l) + (size_t)k0 * nn; a.out_u = S.at<double>(o_u) + (size_t)k0 * nn;
        a.out_v = S.at<int8_t>(o_v) + (size_t)k0 * vv;
        enqueue_treerec_bounds(a, (int)std::min(kTrChunk, (int64_t)count - k0), ctx->stream);
        rc = nr_launched(S, rc);
    }
    return S.finish(rc);
}

int mipx_noderows_lineage_seed(mipx_ctx *ctx, int n, int nv, int64_t nodes_count, const int32_t *parent,
                               const int32_t *vd, const double *val, int count, const int64_t *ids,
                               const int32_t *slots, int64_t capacity, const double *root_l, const double *root_u,
                               const int8_t *root_v, double *pool_l, double *pool_u, int8_t *pool_v) {
    if (!ctx) return MIPX_EINVAL;
    const char *who = "mipx_noderows_lineage_seed";
    std::vector<mipx::TrNode> mirror;
    if (int rc = nr_lineage_check(ctx, who, n, nv, nodes_count, parent, vd, val, count, ids, root_l, root_u, mirror)) return rc;
    if (capacity < 1 || capacity > INT32_MAX) return refuse(ctx, who, "capacity < 1");
    if (!pool_l || !pool_u || !pool_v || (count > 0 && !slots)) return refuse(ctx, who, "a null argument");
    {   // (slots outside the pool write nothing: only those inside can collide)
        std::vector<int32_t> in;
        for (int k = 0; k < count; k++)
            if (slots[k] >= 0 && slots[k] < capacity) in.push_back(slots[k]);
        if (!nr_distinct(in.data(), in.size())) return refuse(ctx, who, "two equal slots inside the pool");
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)n, vv = (size_t)nv, cnt = (size_t)count, cap = (size_t)capacity;
    Staging S(ctx, who);
    const size_t o_nd = S.in(mirror.data(), mirror.size() * sizeof(mipx::TrNode)), o_id = S.in(ids, cnt * 8),
                 o_sl = S.in(slots, cnt * 4), o_rl = S.in(root_l, nn * 8), o_ru = S.in(root_u, nn * 8), o_rv = S.in(root_v, vv),
                 o_l = nr_inout(S, pool_l, cap * nn * 8), o_u = nr_inout(S, pool_u, cap * nn * 8), o_v = nr_inout(S, pool_v, cap * vv);
    int rc = S.alloc();
    if (rc == MIPX_OK) rc = S.upload();
    for (int64_t k0 = 0; rc == MIPX_OK && k0 < count; k0 += kTrChunk) {
        mipx::RestartSeedArgs a;
        a.n = n; a.nv = nv; a.nodes_count = nodes_count; a.capacity = capacity; a.nodes = S.at<const mipx::TrNode>(o_nd);
        a.ids = S.at<const int64_t>(o_id) + k0; a.slots = S.at<const int32_t>(o_sl) + k0;
        a.root_l = S.at<const double>(o_rl); a.root_u = S.at<const double>(o_ru);
        a.root_v = root_v ? S.at<const int8_t>(o_rv) : nullptr;
        a.pool_l = S.at<double>(o_l); a.pool_u = S.at<double>(o_u); a.pool_v = S.at<int8_t>(o_v);
        enqueue_restart_seed(a, (int)std::min(kTrChunk, (int64_t)count - k0), ctx->stream);
        rc = nr_launched(S, rc);
    }
    return S.finish(rc);
}

int mipx_noderows_cut_lists(mipx_ctx *ctx, int kc, int count, const int32_t *slot, int pool_rows,
                            const int32_t *pool_ncut, const int32_t *pool_ids, int32_t *lists) {
    if (!ctx) return MIPX_EINVAL;
    const char *who = "mipx_noderows_cut_lists";
    if (kc < 1 || kc > mipx::kMaxNodeCuts || pool_rows < 1 || count < 0)
        return refuse(ctx, who, "kc outside 1 .. 64, pool_rows < 1 or count < 0");
    if (!pool_ncut || !pool_ids || (count > 0 && (!slot || !lists))) return refuse(ctx, who, "a null argument");
    if (!nr_rows_ok(slot, (size_t)count, pool_rows)) return refuse(ctx, who, "a slot outside the pool");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t K = (size_t)kc, PR = (size_t)pool_rows, cnt = (size_t)count;
    Staging S(ctx, who);
    const size_t o_sl = S.in(slot, cnt * 4), o_nc = S.in(pool_ncut, PR * 4), o_id = S.in(pool_ids, PR * K * 4),
                 o_li = nr_inout(S, lists, cnt * (1 + K) * 4);
    int rc = S.alloc();
    if (rc == MIPX_OK) rc = S.upload();
    if (rc == MIPX_OK && count > 0) {
        mipx::CutMigArgs a;
        a.kc = kc; a.slot = S.at<const int32_t>(o_sl); a.pool_ncut = S.at<int32_t>(o_nc); a.pool_ids = S.at<int32_t>(o_id);
        a.lists = S.at<int32_t>(o_li);
        enqueue_cutmig_lists(a, count, ctx->stream);
        rc = nr_launched(S, rc);
    }
    return S.finish(rc);
}

int mipx_noderows_cut_gather(mipx_ctx *ctx, int n, int count, const int32_t *src, int64_t store_rows,
                             const double *store_pi, const double *store_pi0, double *tab_pi, double *tab_pi0) {
    if (!ctx) return MIPX_EINVAL;
    const char *who = "mipx_noderows_cut_gather";
    if (n < 1 || store_rows < 1 || count < 0) return refuse(ctx, who, "n or store_rows < 1, or count < 0");
    if (!store_pi || !store_pi0 || (count > 0 && (!src || !tab_pi || !tab_pi0))) return refuse(ctx, who, "a null argument");
    if (!nr_rows_ok(src, (size_t)count, store_rows)) return refuse(ctx, who, "a src outside the store");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)n, SR = (size_t)store_rows, cnt = (size_t)count;
    Staging S(ctx, who);
    const size_t o_src = S.in(src, cnt * 4), o_sp = S.in(store_pi, SR * nn * 8), o_s0 = S.in(store_pi0, SR * 8),
                 o_tp = nr_inout(S, tab_pi, cnt * nn * 8), o_t0 = nr_inout(S, tab_pi0, cnt * 8);
    int rc = S.alloc();
    if (rc == MIPX_OK) rc = S.upload();
    if (rc == MIPX_OK && count > 0) {
        mipx::CutMigArgs a;
        a.n = n; a.src = S.at<const int32_t>(o_src); a.store_pi = S.at<double>(o_sp); a.store_pi0 = S.at<double>(o_s0);
        a.tab_pi = S.at<double>(o_tp); a.tab_pi0 = S.at<double>(o_t0);
        enqueue_cutmig_gather(a, count, ctx->stream);
        rc = nr_launched(S, rc);
    }
    return S.finish(rc);
}

int mipx_noderows_cut_scatter(mipx_ctx *ctx, int n, int count, int64_t base, const double *tab_pi, const double *tab_pi0,
                              int64_t store_rows, double *store_pi, double *store_pi0) {
    if (!ctx) return MIPX_EINVAL;
    const char *who = "mipx_noderows_cut_scatter";
    if (n < 1 || store_rows < 1 || count < 0 || base < 0) return refuse(ctx, who, "n or store_rows < 1, or count or base < 0");
    if (base + count > store_rows) return refuse(ctx, who, "base + count > store_rows");
    if (!store_pi || !store_pi0 || (count > 0 && (!tab_pi || !tab_pi0))) return refuse(ctx, who, "a null argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)n, SR = (size_t)store_rows, cnt = (size_t)count;
    Staging S(ctx, who);
    const size_t o_tp = S.in(tab_pi, cnt * nn * 8), o_t0 = S.in(tab_pi0, cnt * 8), o_sp = nr_inout(S, store_pi, SR * nn * 8),
                 o_s0 = nr_inout(S, store_pi0, SR * 8);
    int rc = S.alloc();
    if (rc == MIPX_OK) rc = S.upload();
    if (rc == MIPX_OK && count > 0) {
        mipx::CutMigArgs a;
        a.n = n; a.base = base; a.store_pi = S.at<double>(o_sp); a.store_pi0 = S.at<double>(o_s0);
        a.tab_pi = S.at<double>(o_tp); a.tab_pi0 = S.at<double>(o_t0);
        enqueue_cutmig_scatter(a, count, ctx->stream);
        rc = nr_launched(S, rc);
    }
    return S.finish(rc);
}

int mipx_noderows_cut_unpack_lists(mipx_ctx *ctx, int kc, int count, const int32_t *slot, const int32_t *lists,
                                   int64_t base, int ctab, int pool_rows, int32_t *pool_ncut, int32_t *pool_ids,
                                   int32_t *bad) {
    if (!ctx) return MIPX_EINVAL;
    const char *who = "mipx_noderows_cut_unpack_lists";
    if (kc < 1 || kc > mipx::kMaxNodeCuts || pool_rows < 1 || count < 0 || base < 0 || ctab < 0)
        return refuse(ctx, who, "kc outside 1 .. 64, pool_rows < 1, or count, base or ctab < 0");
    if (base + ctab > INT32_MAX) return refuse(ctx, who, "base + ctab > INT32_MAX");
    if (!pool_ncut || !pool_ids || !bad || (count > 0 && (!slot || !lists))) return refuse(ctx, who, "a null argument");
    if (!nr_rows_ok(slot, (size_t)count, pool_rows)) return refuse(ctx, who, "a slot outside the pool");
    if (!nr_distinct(slot, (size_t)count)) return refuse(ctx, who, "two equal slots");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t K = (size_t)kc, PR = (size_t)pool_rows, cnt = (size_t)count;
    int32_t zero = 0;
    Staging S(ctx, who);
    const size_t o_sl = S.in(slot, cnt * 4), o_li = S.in(lists, cnt * (1 + K) * 4), o_nc = nr_inout(S, pool_ncut, PR * 4),
                 o_id = nr_inout(S, pool_ids, PR * K * 4), o_bad = S.in(&zero, 4);
    S.down(bad, o_bad, 4);
    int rc = S.alloc();
    if (rc == MIPX_OK) rc = S.upload();
    if (rc == MIPX_OK && count > 0) {
        mipx::CutMigArgs a;
        a.kc = kc; a.slot = S.at<const int32_t>(o_sl); a.lists = S.at<int32_t>(o_li); a.pool_ncut = S.at<int32_t>(o_nc);
        a.pool_ids = S.at<int32_t>(o_id); a.base = base; a.ctab = ctab; a.bad = S.at<int32_t>(o_bad);
        enqueue_cutmig_unpack_lists(a, count, ctx->stream);
        rc = nr_launched(S, rc);
    }
    return S.finish(rc);
}

int mipx_noderows_spill_pack(mipx_ctx *ctx, int n, int nv, int kc, int count, const double *root_l, const double *root_u,
                             int pool_rows, const double *l, const double *u, const int8_t *v, const int32_t *ncut,
                             const int32_t *ids, const int32_t *slot, const int64_t *node_id, int64_t *out_offsets,
                             void *out_bytes, int64_t cap, int64_t *used) {
    if (!ctx) return MIPX_EINVAL;
    const char *who = "mipx_noderows_spill_pack";
    if (n < 1 || nv < 1 || pool_rows < 1 || count < 0 || cap < 0 || kc < 0 || kc > mipx::kMaxNodeCuts)
        return refuse(ctx, who, "n, nv or pool_rows < 1, count or cap < 0, or kc outside 0 .. 64");
    if (!root_l || !root_u || !l || !u || !v || !out_offsets || !used || (cap > 0 && !out_bytes) || (kc > 0 && (!ncut || !ids)))
        return refuse(ctx, who, "a null argument");
    if (slot ? !nr_rows_ok(slot, (size_t)count, pool_rows) : count > pool_rows) return refuse(ctx, who, "a slot outside the pool");
    for (int r = 0; kc > 0 && r < count; r++) {
        const int32_t nc = ncut[slot ? slot[r] : r];
        if (nc < 0 || nc > kc) return refuse(ctx, who, "an ncut outside 0 .. kc");
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)n, vv = (size_t)nv, K = (size_t)kc, PR = (size_t)pool_rows, cnt = (size_t)count;
    Staging S(ctx, who);
    const size_t o_rl = S.in(root_l, nn * 8), o_ru = S.in(root_u, nn * 8), o_l = S.in(l, PR * nn * 8), o_u = S.in(u, PR * nn * 8),
                 o_v = S.in(v, PR * vv), o_nc = S.in(kc ? ncut : nullptr, PR * 4), o_id = S.in(kc ? ids : nullptr, PR * K * 4),
                 o_sl = S.in(slot, cnt * 4), o_ni = S.in(node_id, cnt * 8), o_off = nr_inout(S, out_offsets, (cnt + 1) * 8),
                 o_rec = S.in(out_bytes, (size_t)cap);
    int rc = S.alloc();
    if (rc == MIPX_OK) rc = S.upload();
    mipx::SpillArgs a;
    a.n = n; a.nv = nv; a.kc = kc;
    a.root_l = S.at<const double>(o_rl); a.root_u = S.at<const double>(o_ru);
    a.l = S.at<double>(o_l); a.u = S.at<double>(o_u); a.v = S.at<int8_t>(o_v);
    a.ncut = S.at<int32_t>(o_nc); a.ids = S.at<int32_t>(o_id);
    a.slot = slot ? S.at<const int32_t>(o_sl) : nullptr; a.node_id = node_id ? S.at<const int64_t>(o_ni) : nullptr;
    a.off = S.at<int64_t>(o_off); a.rec = S.at<char>(o_rec);
    hipStream_t st = ctx->stream;
    int64_t total = 0;
    if (rc == MIPX_OK && count > 0) {   // as a spill event: sizes and offsets, the total to the host, then the records
        enqueue_spill_count(a, count, st);
        enqueue_spill_scan(a, count, st);
        rc = nr_launched(S, rc);
        if (rc == MIPX_OK && hipMemcpyAsync(&total, a.off + cnt, 8, hipMemcpyDeviceToHost, st) != hipSuccess) rc = S.err("download", hipGetLastError());
        if (rc == MIPX_OK && hipStreamSynchronize(st) != hipSuccess) rc = S.err("sync", hipGetLastError());
        if (rc == MIPX_OK && total <= cap) {
            enqueue_spill_pack(a, count, st);
            rc = nr_launched(S, rc);
        }
    }
    const bool small = rc == MIPX_OK && total > cap;   // (the offsets still come back, out_bytes stays as it was)
    if (rc == MIPX_OK) {
        *used = total;
        if (!small) S.down(out_bytes, o_rec, (size_t)cap);
    }
    rc = S.finish(rc);
    return rc == MIPX_OK && small ? fail(ctx, MIPX_ENOMEM, "mipx_noderows_spill_pack: out_bytes too small (see *used)") : rc;
}

int mipx_noderows_spill_unpack(mipx_ctx *ctx, int n, int nv, int kc, int count, const double *root_l,
                               const double *root_u, const int64_t *offsets, const void *in_bytes, const int32_t *slot,
                               int pool_rows, double *l, double *u, int8_t *v, int32_t *ncut, int32_t *ids) {
    if (!ctx) return MIPX_EINVAL;
    const char *who = "mipx_noderows_spill_unpack";
    if (n < 1 || nv < 1 || pool_rows < 1 || count < 0 || kc < 0 || kc > mipx::kMaxNodeCuts)
        return refuse(ctx, who, "n, nv or pool_rows < 1, count < 0, or kc outside 0 .. 64");
    if (!root_l || !root_u || !l || !u || !v || !offsets || (count > 0 && !in_bytes) || (kc > 0 && (!ncut || !ids)))
        return refuse(ctx, who, "a null argument");
    if (slot ? !nr_rows_ok(slot, (size_t)count, pool_rows) : count > pool_rows) return refuse(ctx, who, "a slot outside the pool");
    if (slot && !nr_distinct(slot, (size_t)count)) return refuse(ctx, who, "two equal slots");
    if (count == 0) return MIPX_OK;
    if (int rc = spill_check_records(ctx, who, n, nv, kc, (size_t)count, offsets, (const char *)in_bytes)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)n, vv = (size_t)nv, K = (size_t)kc, PR = (size_t)pool_rows, cnt = (size_t)count;
    Staging S(ctx, who);
    const size_t o_rl = S.in(root_l, nn * 8), o_ru = S.in(root_u, nn * 8), o_off = S.in(offsets, (cnt + 1) * 8),
                 o_rec = S.in(in_bytes, (size_t)offsets[cnt]), o_sl = S.in(slot, cnt * 4), o_l = nr_inout(S, l, PR * nn * 8),
                 o_u = nr_inout(S, u, PR * nn * 8), o_v = nr_inout(S, v, PR * vv),
                 o_nc = nr_inout(S, kc ? ncut : nullptr, PR * 4), o_id = nr_inout(S, kc ? ids : nullptr, PR * K * 4);
    int rc = S.alloc();
    if (rc == MIPX_OK) rc = S.upload();
    if (rc == MIPX_OK) {
        mipx::SpillArgs a;
        a.n = n; a.nv = nv; a.kc = kc;
        a.root_l = S.at<const double>(o_rl); a.root_u = S.at<const double>(o_ru);
        a.l = S.at<double>(o_l); a.u = S.at<double>(o_u); a.v = S.at<int8_t>(o_v);
        a.ncut = S.at<int32_t>(o_nc); a.ids = S.at<int32_t>(o_id);
        a.slot = slot ? S.at<const int32_t>(o_sl) : nullptr; a.off = S.at<int64_t>(o_off); a.rec = S.at<char>(o_rec);
        enqueue_spill_unpack(a, count, ctx->stream);
        rc = nr_launched(S, rc);
    }
    return S.finish(rc);
}

int mipx_noderows_spill_gather_rows(mipx_ctx *ctx, int n, int nv, int count, const int32_t *slot, int src_rows,
                                    const double *src_l, const double *src_u, const int8_t *src_v, double *l, double *u,
                                    int8_t *v) {
    if (!ctx) return MIPX_EINVAL;
    const char *who = "mipx_noderows_spill_gather_rows";
    if (n < 1 || nv < 1 || src_rows < 1 || count < 0) return refuse(ctx, who, "n, nv or src_rows < 1, or count < 0");
    if (!src_l || !src_u || !src_v || (count > 0 && (!slot || !l || !u || !v))) return refuse(ctx, who, "a null argument");
    if (!nr_rows_ok(slot, (size_t)count, src_rows, INT32_MIN)) return refuse(ctx, who, "a slot >= src_rows");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)n, vv = (size_t)nv, SR = (size_t)src_rows, cnt = (size_t)count;
    Staging S(ctx, who);
    const size_t o_sl = S.in(slot, cnt * 4), o_sL = S.in(src_l, SR * nn * 8), o_sU = S.in(src_u, SR * nn * 8),
                 o_sV = S.in(src_v, SR * vv), o_l = nr_inout(S, l, cnt * nn * 8), o_u = nr_inout(S, u, cnt * nn * 8),
                 o_v = nr_inout(S, v, cnt * vv);
    int rc = S.alloc();
    if (rc == MIPX_OK) rc = S.upload();
    if (rc == MIPX_OK && count > 0) {
        mipx::SpillArgs a;
        a.n = n; a.nv = nv; a.slot = S.at<const int32_t>(o_sl);
        a.l = S.at<double>(o_l); a.u = S.at<double>(o_u); a.v = S.at<int8_t>(o_v);
        enqueue_spill_gather_rows(a, count, ctx->stream, S.at<const double>(o_sL), S.at<const double>(o_sU), S.at<const int8_t>(o_sV));
        rc = nr_launched(S, rc);
    }
    return S.finish(rc);
}

}  // extern "C"
