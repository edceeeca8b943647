// treerec_api.hip.h -- host side and C entries of include/mipx_treerec.h (included at the end of
// tree_engine.hip.h): the device mirror's upload, the bounds launch, the batched re-solve.

namespace {

constexpr int64_t kTrChunk = 1 << 14;   // nodes per launch of a query (bounds: 2 x chunk x n f64 on the device)

// nothing of the search is in flight between two solves; a query still waits for every stream that writes
int tr_quiesce(mipx_tree *t) {
    mipx_ctx *ctx = t->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(t->st3));
    HIP_TRY(ctx, hipStreamSynchronize(t->st2));
    if (t->stf) HIP_TRY(ctx, hipStreamSynchronize(t->stf));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return MIPX_OK;
}

// the mirror's tail, the root's rows (once), the query buffers for `chunk` nodes
int tr_prepare(mipx_tree *t, int64_t chunk) {
    mipx_ctx *ctx = t->ctx;
    TreeRec &tr = t->tr;
    const size_t n = (size_t)t->n, nv = n + (size_t)t->m;
    const int64_t N = (int64_t)t->nodes.size();
    if (!tr.e0) {
        HIP_TRY(ctx, hipEventCreate(&tr.e0));
        HIP_TRY(ctx, hipEventCreate(&tr.e1));
    }
    if (!tr.d_root) {
        int rc = dmalloc(ctx, &tr.d_root, 2 * n);
        if (rc) return rc;
        HIP_TRY(ctx, hipMemcpy(tr.d_root, t->root_l.data(), n * 8, hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(tr.d_root + n, t->root_u.data(), n * 8, hipMemcpyHostToDevice));
        if ((rc = dmalloc(ctx, &tr.d_root_v, nv))) return rc;
    }
    if (tr.have_root && !tr.root_v_up) {
        HIP_TRY(ctx, hipMemcpy(tr.d_root_v, tr.root_v.data(), nv, hipMemcpyHostToDevice));
        tr.root_v_up = true;
    }
    if (N > tr.d_cap) {   // grow by doubling, the entries there are kept
        const int64_t want = std::max<int64_t>(N, std::max<int64_t>(1024, 2 * tr.d_cap));
        mipx::TrNode *q = nullptr;
        int rc = dmalloc(ctx, &q, (size_t)want);
        if (rc) return rc;
        if (tr.d_nodes && tr.d_count > 0)
            HIP_TRY(ctx, hipMemcpy(q, tr.d_nodes, (size_t)tr.d_count * sizeof(mipx::TrNode), hipMemcpyDeviceToDevice));
        if (tr.d_nodes) (void)hipFree(tr.d_nodes);
        tr.d_nodes = q;
        tr.d_cap = want;
    }
    if (N > tr.d_count) {   // only the tail new since the last query goes up
        std::vector<mipx::TrNode> tail((size_t)(N - tr.d_count));
        for (int64_t id = tr.d_count; id < N; id++) {
            const NodeRec &nd = t->nodes[(size_t)id];
            mipx::TrNode &e = tail[(size_t)(id - tr.d_count)];
            e.parent = tr.parent[(size_t)id];
            e.vd = nd.b_idx < 0 ? -2 : 2 * nd.b_idx + nd.b_dir;
            e.val = nd.b_val;
        }
        HIP_TRY(ctx, hipMemcpy(tr.d_nodes + tr.d_count, tail.data(), tail.size() * sizeof(mipx::TrNode), hipMemcpyHostToDevice));
        tr.d_count = N;
    }
    if (chunk > tr.qcap) {
        void *old[] = {tr.d_ids, tr.d_l, tr.d_u};
        for (void *q : old)
            if (q) (void)hipFree(q);
        tr.d_ids = nullptr; tr.d_l = tr.d_u = nullptr; tr.qcap = 0;
        int rc = dmalloc(ctx, &tr.d_ids, (size_t)chunk) | dmalloc(ctx, &tr.d_l, (size_t)chunk * n) |
                 dmalloc(ctx, &tr.d_u, (size_t)chunk * n);
        if (rc) return rc;
        tr.qcap = chunk;
    }
    return MIPX_OK;
}

int tr_check_ids(mipx_tree *t, const char *who, int64_t K, const int64_t *ids) {
    if (!t->tr.on) return fail(t->ctx, MIPX_EINVAL, (std::string(who) + ": recording is off (mipx_tree_set_tree_record)").c_str());
    if (K < 0 || (K > 0 && !ids)) return fail(t->ctx, MIPX_EINVAL, (std::string(who) + ": bad argument").c_str());
    const int64_t N = (int64_t)t->nodes.size();
    for (int64_t k = 0; k < K; k++)
        if (ids[k] < 0 || ids[k] >= N) return fail(t->ctx, MIPX_EINVAL, (std::string(who) + ": node id outside the tree").c_str());
    return MIPX_OK;
}

// bounds of ids[0..cnt) into tr.d_l / tr.d_u (and the root's basis codes into out_v), queued on the main stream
// behind tr.e0 (the caller records tr.e1 behind the last kernel of the query)
int tr_launch_bounds(mipx_tree *t, int cnt, const int64_t *ids, int8_t *out_v) {
    mipx_ctx *ctx = t->ctx;
    TreeRec &tr = t->tr;
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipMemcpyAsync(tr.d_ids, ids, (size_t)cnt * 8, hipMemcpyHostToDevice, st));
    mipx::TrBoundsArgs a;
    a.n = t->n; a.nv = t->n + t->m; a.nodes_count = tr.d_count; a.nodes = tr.d_nodes; a.ids = tr.d_ids;
    a.root_l = tr.d_root; a.root_u = tr.d_root + t->n; a.root_v = tr.have_root ? tr.d_root_v : nullptr;
    a.out_l = tr.d_l; a.out_u = tr.d_u; a.out_v = out_v;
    HIP_TRY(ctx, hipEventRecord(tr.e0, st));
    enqueue_treerec_bounds(a, cnt, st);
    HIP_TRY(ctx, hipGetLastError());
    tr.materialised += cnt;
    return MIPX_OK;
}

void tr_take_time(mipx_tree *t) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, t->tr.e0, t->tr.e1) == hipSuccess) t->tr.query_us += 1000.0 * ms;
}

}  // namespace

extern "C" {

int mipx_tree_set_tree_record(mipx_tree *t, int on) {
    if (!t) return MIPX_EINVAL;
    mipx_ctx *ctx = t->ctx;
    if (t->steps > 0 || t->nodes.size() != 1 || t->evaluated > 0)
        return fail(ctx, MIPX_EINVAL, "mipx_tree_set_tree_record: recording is set before the first step");
    if (t->comm) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_tree_record: not with a communicator");
    if (t->cuts) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_tree_record: not with cut rounds");
    if (t->n > 65536) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_tree_record: more than 65536 columns");
    if (on && t->pg.on) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_tree_record: not with the bound propagation (mipx_tree_set_propagation)");
    if (on && t->rc.on) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_tree_record: not with the reduced-cost tightening (mipx_tree_set_reduced_cost)");
    if (on && t->os.on) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_tree_record: not with the objective step (mipx_tree_set_objective_step)");
    TreeRec &tr = t->tr;
    if (!on) {   // (before the first step nothing has been recorded; the finish mode stays as it is)
        tr.on = false;
        return MIPX_OK;
    }
    tr.on = true;
    // every node, dive children included, gets its id and its parent in tree_finish's evaluate: every step
    // is finished on the host with the host's pseudo-cost table, the switch mipx_tree_set_dual_record uses
    t->fast_ok = false;
    tr.root();
    return MIPX_OK;
}

int64_t mipx_tree_records(mipx_tree *t, int64_t first, int64_t count, int64_t *parent, int32_t *bvar, int32_t *bdir,
                          double *bval, int32_t *depth, int32_t *lp_status, int32_t *flags, double *dual_bound,
                          double *objective) {
    if (!t) return MIPX_EINVAL;
    const TreeRec &tr = t->tr;
    if (!tr.on) return fail(t->ctx, MIPX_EINVAL, "mipx_tree_records: recording is off (mipx_tree_set_tree_record)");
    const int64_t N = (int64_t)t->nodes.size();
    if (first < 0 || count < 0) return fail(t->ctx, MIPX_EINVAL, "mipx_tree_records: bad range");
    const int64_t cnt = first >= N ? 0 : std::min(count, N - first);
    for (int64_t k = 0; k < cnt; k++) {
        const size_t id = (size_t)(first + k);
        const NodeRec &nd = t->nodes[id];
        const int st = tr.status[id];
        if (parent) parent[k] = tr.parent[id];
        if (bvar) bvar[k] = nd.b_idx;
        if (bdir) bdir[k] = nd.b_dir;
        if (bval) bval[k] = nd.b_val;
        if (depth) depth[k] = nd.depth;
        if (lp_status) lp_status[k] = st;
        if (flags) flags[k] = tr.flags[id] | (st < 0 && !(tr.flags[id] & MIPX_TR_CLOSED_AT_POP) ? MIPX_TR_OPEN : 0);
        if (dual_bound) dual_bound[k] = nd.dual_bound;
        if (objective) objective[k] = tr.obj[id];
    }
    return cnt;
}

int mipx_tree_node_bounds(mipx_tree *t, int64_t K, const int64_t *ids, double *l, double *u) {
    if (!t) return MIPX_EINVAL;
    int rc = tr_check_ids(t, "mipx_tree_node_bounds", K, ids);
    if (rc || K == 0) return rc;
    mipx_ctx *ctx = t->ctx;
    TreeRec &tr = t->tr;
    if ((rc = tr_quiesce(t))) return rc;
    if ((rc = tr_prepare(t, std::min(K, kTrChunk)))) return rc;
    const size_t n = (size_t)t->n;
    for (int64_t k0 = 0; k0 < K; k0 += kTrChunk) {
        const int cnt = (int)std::min(kTrChunk, K - k0);
        if ((rc = tr_launch_bounds(t, cnt, ids + k0, nullptr))) return rc;
        HIP_TRY(ctx, hipEventRecord(tr.e1, ctx->stream));
        if (l) HIP_TRY(ctx, hipMemcpyAsync(l + (size_t)k0 * n, tr.d_l, (size_t)cnt * n * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (u) HIP_TRY(ctx, hipMemcpyAsync(u + (size_t)k0 * n, tr.d_u, (size_t)cnt * n * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        tr_take_time(t);
    }
    return MIPX_OK;
}

int mipx_tree_node_solve(mipx_tree *t, int64_t K, const int64_t *ids, int32_t *status, double *obj, double *x,
                         int8_t *vstat) {
    if (!t) return MIPX_EINVAL;
    int rc = tr_check_ids(t, "mipx_tree_node_solve", K, ids);
    if (rc || K == 0) return rc;
    mipx_ctx *ctx = t->ctx;
    TreeRec &tr = t->tr;
    if ((rc = tr_quiesce(t))) return rc;
    const int64_t chunk = std::min(K, kTrChunk);
    if ((rc = tr_prepare(t, chunk))) return rc;
    const size_t n = (size_t)t->n, nv = n + (size_t)t->m, C = (size_t)chunk;
    // one block: vstat in | vstat out | x | obj | status | iters | pivots
    const size_t o_vo = pad8(C * nv), o_x = o_vo + pad8(C * nv), o_obj = o_x + C * n * 8, o_st = o_obj + C * 8,
                 o_it = o_st + pad8(C * 4), o_np = o_it + pad8(C * 4), total = o_np + pad8(C * 4);
    if (total > tr.solve_bytes) {
        if (tr.d_solve) (void)hipFree(tr.d_solve);
        tr.d_solve = nullptr; tr.solve_bytes = 0;
        HIP_TRY(ctx, hipMalloc((void **)&tr.d_solve, total));
        tr.solve_bytes = total;
    }
    char *blk = tr.d_solve;
    hipStream_t st = ctx->stream;
    for (int64_t k0 = 0; k0 < K; k0 += kTrChunk) {
        const int cnt = (int)std::min(kTrChunk, K - k0);
        if ((rc = tr_launch_bounds(t, cnt, ids + k0, (int8_t *)blk))) return rc;
        mipx::LpArgs a = problem_args(t->prob);
        a.l = tr.d_l; a.u = tr.d_u;
        a.vstat_in = tr.have_root ? (const int8_t *)blk : nullptr;   // (the root did not end optimal: cold)
        a.max_iter = 0;
        a.status = (int32_t *)(blk + o_st); a.obj = (double *)(blk + o_obj); a.x = (double *)(blk + o_x);
        a.vstat_out = (int8_t *)(blk + o_vo); a.iters = (int32_t *)(blk + o_it); a.npivots = (int32_t *)(blk + o_np);
        a.batch = cnt;
        if ((rc = launch_lp_any(t->prob, a, cnt))) return rc;
        HIP_TRY(ctx, hipEventRecord(tr.e1, st));
        const size_t c = (size_t)cnt, k = (size_t)k0;
        if (status) HIP_TRY(ctx, hipMemcpyAsync(status + k, blk + o_st, c * 4, hipMemcpyDeviceToHost, st));
        if (obj) HIP_TRY(ctx, hipMemcpyAsync(obj + k, blk + o_obj, c * 8, hipMemcpyDeviceToHost, st));
        if (x) HIP_TRY(ctx, hipMemcpyAsync(x + k * n, blk + o_x, c * n * 8, hipMemcpyDeviceToHost, st));
        if (vstat) HIP_TRY(ctx, hipMemcpyAsync(vstat + k * nv, blk + o_vo, c * nv, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        tr_take_time(t);
        tr.resolved += cnt;
    }
    return MIPX_OK;
}

int mipx_tree_record_stats(mipx_tree *t, int64_t out[6]) {
    if (!t || !out) return MIPX_EINVAL;
    const TreeRec &tr = t->tr;
    const int64_t N = tr.on ? (int64_t)tr.parent.size() : 0;
    out[0] = N;
    out[1] = N * 14 + (int64_t)tr.root_v.size();
    out[2] = tr.d_cap * (int64_t)sizeof(mipx::TrNode);
    out[3] = tr.materialised; out[4] = tr.resolved; out[5] = (int64_t)tr.query_us;
    return MIPX_OK;
}

}  // extern "C"
