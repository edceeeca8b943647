// cglp_api.hip.h -- host side and C entries of include/mipx_cglp.h (included at the end of tree_engine.hip.h,
// behind treerec_api.hip.h, whose mirror and bounds kernel it uses): the session's buffers, the leaf-LP
// launches with pi in the place of c, the selection.

struct mipx_support {
    mipx_tree *t = nullptr;
    int n = 0, m = 0;
    int64_t T = 0;                       // leaves now
    std::vector<int64_t> ids, dropped;   // node ids: of the leaves, of those dropped as infeasible
    bool first = true;                   // no evaluation yet: the next one starts from the root's basis and drops
    // per leaf, position k the same leaf in every buffer
    int64_t *d_ids = nullptr;
    double *d_l = nullptr, *d_u = nullptr, *d_x = nullptr, *d_obj = nullptr, *d_margin = nullptr;
    int8_t *d_v[2] = {nullptr, nullptr};   // basis codes: the last launch's output is the next one's input
    int cur = 0;                           // d_v[cur]: the input of the next launch
    int32_t *d_status = nullptr, *d_iters = nullptr, *d_np = nullptr;
    double *d_pi = nullptr;
    // selection: per segment candidates (grown with max_points), the output block
    double *d_cand_m = nullptr, *d_seg = nullptr, *d_block = nullptr;
    int32_t *d_cand_id = nullptr, *d_cand_t = nullptr;
    int capP = 0, G0 = 1;                // rows the selection buffers hold, segments of the leaves at open
    hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
    int64_t evals = 0, lps = 0, iters = 0, pivots = 0, bytes = 0;
    double kernel_us = 0.0, select_us = 0.0;
};

namespace {

void sup_free(mipx_support *s) {
    void *dp[] = {s->d_ids, s->d_l, s->d_u, s->d_x, s->d_obj, s->d_margin, s->d_v[0], s->d_v[1], s->d_status, s->d_iters,
                  s->d_np, s->d_pi, s->d_cand_m, s->d_seg, s->d_block, s->d_cand_id, s->d_cand_t};
    for (void *q : dp)
        if (q) (void)hipFree(q);
    if (s->e0) (void)hipEventDestroy(s->e0);
    if (s->e1) (void)hipEventDestroy(s->e1);
    if (s->e2) (void)hipEventDestroy(s->e2);
    delete s;
}

int sup_segments(int64_t T) { return (int)((T + mipx::kSupSeg - 1) / mipx::kSupSeg); }

// the ids go up; bounds (and the root's basis codes into d_v[cur]) of all of them, kTrChunk nodes per launch
int sup_bounds(mipx_support *s) {
    mipx_tree *t = s->t;
    mipx_ctx *ctx = t->ctx;
    TreeRec &tr = t->tr;
    int rc = tr_prepare(t, 1);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)s->n, nv = n + (size_t)s->m;
    HIP_TRY(ctx, hipMemcpyAsync(s->d_ids, s->ids.data(), (size_t)s->T * 8, hipMemcpyHostToDevice, st));
    for (int64_t k0 = 0; k0 < s->T; k0 += kTrChunk) {
        const int cnt = (int)std::min(kTrChunk, s->T - k0);
        mipx::TrBoundsArgs a;
        a.n = s->n; a.nv = (int)nv; a.count = cnt; a.nodes_count = tr.d_count; a.nodes = tr.d_nodes; a.ids = s->d_ids + k0;
        a.root_l = tr.d_root; a.root_u = tr.d_root + n; a.root_v = tr.have_root ? tr.d_root_v : nullptr;
        a.out_l = s->d_l + (size_t)k0 * n; a.out_u = s->d_u + (size_t)k0 * n; a.out_v = s->d_v[s->cur] + (size_t)k0 * nv;
        hipLaunchKernelGGL(mipx::treerec_bounds, dim3((unsigned)cnt), dim3(mipx::kTrNT), n, st, a);
        HIP_TRY(ctx, hipGetLastError());
        tr.materialised += cnt;
    }
    return MIPX_OK;
}

// h_t(pi) of every leaf: the node-LP kernel over the session's bounds with d_pi as the objective, kTrChunk
// leaves per launch, without the anchor (its tableau belongs to c)
int sup_launch_lps(mipx_support *s, bool warm) {
    mipx_tree *t = s->t;
    const size_t n = (size_t)s->n, nv = n + (size_t)s->m;
    const int8_t *vin = s->d_v[s->cur];
    int8_t *vout = s->d_v[s->cur ^ 1];
    for (int64_t k0 = 0; k0 < s->T; k0 += kTrChunk) {
        const int cnt = (int)std::min(kTrChunk, s->T - k0);
        const size_t k = (size_t)k0;
        mipx::LpArgs a = problem_args(t->prob, false);
        a.c = s->d_pi;
        a.l = s->d_l + k * n; a.u = s->d_u + k * n;
        a.vstat_in = warm ? vin + k * nv : nullptr;
        a.max_iter = 0;
        a.status = s->d_status + k; a.obj = s->d_obj + k; a.x = s->d_x + k * n;
        a.vstat_out = vout + k * nv; a.iters = s->d_iters + k; a.npivots = s->d_np + k;
        a.batch = cnt;
        const int rc = launch_lp_any(t->prob, a, cnt);
        if (rc) return rc;
    }
    s->cur ^= 1;
    s->lps += s->T;
    return MIPX_OK;
}

// a side of a column that is infinite at the root is finite at a node only if a branching of its lineage set it
bool sup_bounds_finite(mipx_tree *t, const int64_t *ids, int64_t K) {
    std::vector<int> inf_side;   // 2 j + side (0 lower, 1 upper)
    for (int j = 0; j < t->n; j++) {
        if (!std::isfinite(t->root_l[(size_t)j])) inf_side.push_back(2 * j);
        if (!std::isfinite(t->root_u[(size_t)j])) inf_side.push_back(2 * j + 1);
    }
    if (inf_side.empty()) return true;
    std::vector<uint8_t> need((size_t)2 * t->n, 0);
    for (int64_t k = 0; k < K; k++) {
        size_t left = inf_side.size();
        for (int q : inf_side) need[(size_t)q] = 1;
        for (int64_t id = ids[k]; id > 0 && left > 0; id = t->tr.parent[(size_t)id]) {
            const NodeRec &nd = t->nodes[(size_t)id];
            if (nd.b_idx < 0) continue;
            const size_t q = (size_t)2 * nd.b_idx + (nd.b_dir ? 0 : 1);   // right: the lower bound, left: the upper
            if (need[q]) { need[q] = 0; left--; }
        }
        if (left) return false;
    }
    return true;
}

}  // namespace

extern "C" {

int mipx_tree_support_open(mipx_tree *t, const int64_t *ids, int64_t K, mipx_support **out) {
    if (!t || !out) return MIPX_EINVAL;
    *out = nullptr;
    mipx_ctx *ctx = t->ctx;
    int rc = tr_check_ids(t, "mipx_tree_support_open", K, ids);
    if (rc) return rc;
    if (t->cuts) return fail(ctx, MIPX_EINVAL, "mipx_tree_support_open: not with cut rounds");
    if (K > (int64_t)1 << 30) return fail(ctx, MIPX_EINVAL, "mipx_tree_support_open: more than 2^30 leaves");
    if (!sup_bounds_finite(t, ids, K))
        return fail(ctx, MIPX_EINVAL, "mipx_tree_support_open: a leaf has an infinite bound (every leaf must be a polytope)");
    {
        std::vector<int64_t> sorted(ids, ids + K);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
            return fail(ctx, MIPX_EINVAL, "mipx_tree_support_open: a node id is given twice");
    }
    if ((rc = tr_quiesce(t))) return rc;
    mipx_support *s = new (std::nothrow) mipx_support();
    if (!s) return fail(ctx, MIPX_ENOMEM, "mipx_tree_support_open: host alloc");
    s->t = t; s->n = t->n; s->m = t->m; s->T = K;
    s->ids.assign(ids, ids + K);
    s->G0 = std::max(1, sup_segments(K));
    const size_t T = (size_t)K, n = (size_t)t->n, nv = n + (size_t)t->m, G = (size_t)s->G0;
    rc = dmalloc(ctx, &s->d_ids, T) | dmalloc(ctx, &s->d_l, T * n) | dmalloc(ctx, &s->d_u, T * n) | dmalloc(ctx, &s->d_x, T * n) |
         dmalloc(ctx, &s->d_obj, T) | dmalloc(ctx, &s->d_margin, T) | dmalloc(ctx, &s->d_v[0], T * nv) | dmalloc(ctx, &s->d_v[1], T * nv) |
         dmalloc(ctx, &s->d_status, T) | dmalloc(ctx, &s->d_iters, T) | dmalloc(ctx, &s->d_np, T) | dmalloc(ctx, &s->d_pi, n) |
         dmalloc(ctx, &s->d_seg, G * 4);
    if (!rc && (hipEventCreate(&s->e0) != hipSuccess || hipEventCreate(&s->e1) != hipSuccess || hipEventCreate(&s->e2) != hipSuccess))
        rc = fail(ctx, MIPX_EHIP, "mipx_tree_support_open: events");
    s->bytes = (int64_t)(T * 8 + 3 * T * n * 8 + 2 * T * 8 + 2 * T * nv + 3 * T * 4 + n * 8 + G * 32);
    if (!rc && K > 0) rc = sup_bounds(s);
    if (!rc && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = fail(ctx, MIPX_EHIP, "mipx_tree_support_open: sync");
    if (rc) { sup_free(s); return rc; }
    *out = s;
    return MIPX_OK;
}

int mipx_tree_support_eval(mipx_support *s, const double *pi, double pi0, double tol, int max_points,
                           double *block, double *margins) {
    if (!s || !s->t) return MIPX_EINVAL;
    mipx_tree *t = s->t;
    mipx_ctx *ctx = t->ctx;
    if (!pi || !block || max_points < 1 || max_points > mipx::kSupMaxP || !(tol >= 0.0))
        return fail(ctx, MIPX_EINVAL, "mipx_tree_support_eval: bad argument");
    int rc = tr_quiesce(t);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)s->n;
    const int P = max_points;
    const size_t block_len = (size_t)mipx::kSupHead + (size_t)P * (n + 2);
    if (P > s->capP) {   // (the segments only shrink: sized for the leaves the session opened with)
        void *old[] = {s->d_cand_m, s->d_cand_id, s->d_cand_t, s->d_block};
        for (void *q : old)
            if (q) (void)hipFree(q);
        s->d_cand_m = nullptr; s->d_cand_id = s->d_cand_t = nullptr; s->d_block = nullptr;
        s->capP = 0;
        const size_t G0 = (size_t)s->G0;
        rc = dmalloc(ctx, &s->d_cand_m, G0 * P) | dmalloc(ctx, &s->d_cand_id, G0 * P) | dmalloc(ctx, &s->d_cand_t, G0 * P) |
             dmalloc(ctx, &s->d_block, block_len);
        if (rc) return rc;
        s->capP = P;
    }
    HIP_TRY(ctx, hipMemcpyAsync(s->d_pi, pi, n * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipEventRecord(s->e0, st));
    if (s->T > 0) {
        if ((rc = sup_launch_lps(s, s->first ? t->tr.have_root : true))) return rc;
        if (s->first) {   // the empty terms leave; the others are packed and solved again from the root's basis
            std::vector<int32_t> status((size_t)s->T);
            HIP_TRY(ctx, hipMemcpyAsync(status.data(), s->d_status, (size_t)s->T * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(ctx, hipStreamSynchronize(st));
            std::vector<int64_t> keep;
            for (int64_t k = 0; k < s->T; k++) (status[(size_t)k] == 1 ? s->dropped : keep).push_back(s->ids[(size_t)k]);
            if (!s->dropped.empty()) {
                s->ids.swap(keep);
                s->T = (int64_t)s->ids.size();
                s->cur = 0;
                if (s->T > 0 && ((rc = sup_bounds(s)) || (rc = sup_launch_lps(s, t->tr.have_root)))) return rc;
            }
        }
    }
    s->first = false;
    HIP_TRY(ctx, hipEventRecord(s->e1, st));
    if (s->T > 0) {
        mipx::SupSelectArgs a;
        a.T = (int)s->T; a.n = s->n; a.P = P; a.G = sup_segments(s->T);
        a.pi0 = pi0; a.tol = tol;
        a.ids = s->d_ids; a.status = s->d_status; a.obj = s->d_obj; a.x = s->d_x; a.iters = s->d_iters; a.npivots = s->d_np;
        a.margin = s->d_margin; a.cand_m = s->d_cand_m; a.cand_id = s->d_cand_id; a.cand_t = s->d_cand_t;
        a.seg_sum = s->d_seg; a.block = s->d_block;
        hipLaunchKernelGGL(mipx::support_select, dim3((unsigned)a.G), dim3(mipx::kSupNT), 0, st, a);
        HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(mipx::support_select_merge, dim3(1), dim3(mipx::kSupNT), 0, st, a);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipEventRecord(s->e2, st));
    if (s->T > 0) {
        // the head says how many rows there are: the rows asked for come down in one copy all the same
        HIP_TRY(ctx, hipMemcpyAsync(block, s->d_block, block_len * 8, hipMemcpyDeviceToHost, st));
        if (margins) HIP_TRY(ctx, hipMemcpyAsync(margins, s->d_margin, (size_t)s->T * 8, hipMemcpyDeviceToHost, st));
    } else {
        const double head[mipx::kSupHead] = {std::numeric_limits<double>::infinity(), -1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        std::memcpy(block, head, sizeof head);
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, s->e0, s->e2) == hipSuccess) s->kernel_us += 1000.0 * ms;
    if (hipEventElapsedTime(&ms, s->e1, s->e2) == hipSuccess) s->select_us += 1000.0 * ms;
    s->evals++;
    if (s->T > 0) {
        s->iters += (int64_t)block[5];
        s->pivots += (int64_t)block[6];
        t->tr.resolved += s->T;
    }
    return MIPX_OK;
}

int64_t mipx_tree_support_leaves(mipx_support *s, int dropped, int64_t cap, int64_t *ids) {
    if (!s) return MIPX_EINVAL;
    const std::vector<int64_t> &v = dropped ? s->dropped : s->ids;
    if (ids)
        for (int64_t k = 0; k < cap && k < (int64_t)v.size(); k++) ids[k] = v[(size_t)k];
    return (int64_t)v.size();
}

int mipx_tree_support_stats(mipx_support *s, int64_t out[9]) {
    if (!s || !out) return MIPX_EINVAL;
    out[0] = s->T; out[1] = (int64_t)s->dropped.size(); out[2] = s->evals; out[3] = s->lps; out[4] = s->iters;
    out[5] = s->pivots; out[6] = s->bytes + (int64_t)s->capP * ((int64_t)s->G0 * 16 + (int64_t)(s->n + 2) * 8); out[7] = (int64_t)s->kernel_us; out[8] = (int64_t)s->select_us;
    return MIPX_OK;
}

void mipx_tree_support_close(mipx_support *s) {
    if (!s) return;
    if (s->t && s->t->ctx) {
        (void)hipSetDevice(s->t->ctx->device);
        if (s->t->ctx->stream) (void)hipStreamSynchronize(s->t->ctx->stream);
    }
    sup_free(s);
}

}  // extern "C"
