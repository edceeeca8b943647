// cglp_api.hip.h -- host side and C entries of include/mipx_cglp.h and include/mipx_cglp_screen.h (included at the
// end of tree_engine.hip.h, behind treerec_api.hip.h, whose mirror and bounds kernel it uses): the session's buffers,
// the leaf-LP launches with pi in the place of c, the selection; with kept duals the screen in front of the launch,
// the launch over the packed leaves, and the cold retry behind it.

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
    // MIPX_SUPPORT_KEEP_DUALS: the row duals of each leaf's last optimal LP, the screen's outputs, and launch buffers
    // for a packed subset of the leaves (position k of a launch is leaf d_pack[k])
    bool keep = false;
    double *d_y = nullptr, *d_bound = nullptr;
    uint8_t *d_has_y = nullptr, *d_scr = nullptr;
    int32_t *d_pack = nullptr, *d_seg_count = nullptr;
    double *d_seg_min = nullptr;
    mipx::SupPackInfo *d_info = nullptr;
    double *p_l = nullptr, *p_u = nullptr, *p_x = nullptr, *p_obj = nullptr, *p_y = nullptr;
    int8_t *p_v[2] = {nullptr, nullptr};
    int32_t *p_status = nullptr, *p_iters = nullptr, *p_np = nullptr;
    static constexpr int kPairs = 6;     // timed stretches: screen + pack, gather, scatter, and the same of the retry
    hipEvent_t ev[2 * kPairs] = {};
};

namespace {

void sup_free(mipx_support *s) {
    void *dp[] = {s->d_ids, s->d_l, s->d_u, s->d_x, s->d_obj, s->d_margin, s->d_v[0], s->d_v[1], s->d_status, s->d_iters,
                  s->d_np, s->d_pi, s->d_cand_m, s->d_seg, s->d_block, s->d_cand_id, s->d_cand_t,
                  s->d_y, s->d_bound, s->d_has_y, s->d_scr, s->d_pack, s->d_seg_count, s->d_seg_min, s->d_info,
                  s->p_l, s->p_u, s->p_x, s->p_obj, s->p_y, s->p_v[0], s->p_v[1], s->p_status, s->p_iters, s->p_np};
    for (void *q : dp)
        if (q) (void)hipFree(q);
    for (hipEvent_t e : s->ev)
        if (e) (void)hipEventDestroy(e);
    if (s->e0) (void)hipEventDestroy(s->e0);
    if (s->e1) (void)hipEventDestroy(s->e1);
    if (s->e2) (void)hipEventDestroy(s->e2);
    delete s;
}

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
        a.n = s->n; a.nv = (int)nv; a.nodes_count = tr.d_count; a.nodes = tr.d_nodes; a.ids = s->d_ids + k0;
        a.root_l = tr.d_root; a.root_u = tr.d_root + n; a.root_v = tr.have_root ? tr.d_root_v : nullptr;
        a.out_l = s->d_l + (size_t)k0 * n; a.out_u = s->d_u + (size_t)k0 * n; a.out_v = s->d_v[s->cur] + (size_t)k0 * nv;
        enqueue_treerec_bounds(a, cnt, st);
        HIP_TRY(ctx, hipGetLastError());
        tr.materialised += cnt;
    }
    return MIPX_OK;
}

// h_t(pi) of every leaf: the node-LP kernel over the session's bounds with d_pi as the objective, kTrChunk
// leaves per launch, without the anchor (its tableau belongs to c)
int sup_launch_lps(mipx_support *s, bool warm, double *y = nullptr) {
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
        if (y) a.y = y + k * (size_t)s->m;
        a.batch = cnt;
        const int rc = launch_lp_any(t->prob, a, cnt);
        if (rc) return rc;
    }
    s->cur ^= 1;
    s->lps += s->T;
    return MIPX_OK;
}

void sup_tick(mipx_support *s, int i, uint32_t &used) {
    if (hipEventRecord(s->ev[i], s->t->ctx->stream) == hipSuccess) used |= 1u << i;
}

mipx::SupPackArgs sup_pack_args(mipx_support *s, bool by_status, double pi0) {
    mipx::SupPackArgs a;
    if (by_status) a.status = s->d_status;
    else { a.skip = s->d_scr; a.bound = s->d_bound; }
    a.pi0 = pi0;
    a.seg_count = s->d_seg_count; a.seg_min = s->d_seg_min; a.packed = s->d_pack; a.info = s->d_info;
    return a;
}

// the two pack kernels, then the one small read of an evaluation: how many leaves the launch has
int sup_pack(mipx_support *s, const mipx::SupPackArgs &a, mipx::SupPackInfo *info) {
    mipx_ctx *ctx = s->t->ctx;
    hipStream_t st = ctx->stream;
    enqueue_support_pack_count(a, (int)s->T, st);
    HIP_TRY(ctx, hipGetLastError());
    enqueue_support_pack(a, (int)s->T, st);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(info, s->d_info, sizeof *info, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (info->count < 0 || info->count > s->T) return fail(ctx, MIPX_EHIP, "mipx_tree_support_eval_ex: packed count out of range");
    return MIPX_OK;
}

// gather the `count` packed leaves, solve them (warm: from their last bases; else without a basis), scatter
int sup_solve_packed(mipx_support *s, int count, bool warm, bool add, int pair, uint32_t &used) {
    mipx_tree *t = s->t;
    mipx_ctx *ctx = t->ctx;
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)s->n, m = (size_t)s->m, nv = n + m;
    mipx::SupMoveArgs g;
    g.T = (int)s->T; g.n = s->n; g.m = s->m; g.packed = s->d_pack;
    g.l = s->d_l; g.u = s->d_u; g.x = s->d_x; g.obj = s->d_obj; g.y = s->d_y; g.v = s->d_v[s->cur];
    g.status = s->d_status; g.iters = s->d_iters; g.npivots = s->d_np; g.has_y = s->d_has_y;
    g.pl = s->p_l; g.pu = s->p_u; g.px = s->p_x; g.pobj = s->p_obj; g.py = s->p_y; g.pv_in = s->p_v[0]; g.pv_out = s->p_v[1];
    g.pstatus = s->p_status; g.piters = s->p_iters; g.pnpivots = s->p_np;
    g.add = add ? 1 : 0;
    mipx::SupMoveArgs in = g;
    if (!warm) in.v = nullptr;
    sup_tick(s, 2 * pair, used);
    enqueue_support_gather(in, count, st);
    HIP_TRY(ctx, hipGetLastError());
    sup_tick(s, 2 * pair + 1, used);
    for (int64_t k0 = 0; k0 < count; k0 += kTrChunk) {
        const int cnt = (int)std::min(kTrChunk, (int64_t)count - k0);
        const size_t k = (size_t)k0;
        mipx::LpArgs a = problem_args(t->prob, false);
        a.c = s->d_pi;
        a.l = s->p_l + k * n; a.u = s->p_u + k * n;
        a.vstat_in = warm ? s->p_v[0] + k * nv : nullptr;
        a.max_iter = 0;
        a.status = s->p_status + k; a.obj = s->p_obj + k; a.x = s->p_x + k * n; a.y = s->p_y + k * m;
        a.vstat_out = s->p_v[1] + k * nv; a.iters = s->p_iters + k; a.npivots = s->p_np + k;
        a.batch = cnt;
        const int rc = launch_lp_any(t->prob, a, cnt);
        if (rc) return rc;
    }
    s->lps += count;
    sup_tick(s, 2 * pair + 2, used);
    enqueue_support_scatter(g, count, st);
    HIP_TRY(ctx, hipGetLastError());
    sup_tick(s, 2 * pair + 3, used);
    return MIPX_OK;
}

mipx::SupScreenArgs sup_screen_args(const mipx_problem *p, const double *pi, double pi0, double screen_tol,
                                    const double *l, const double *u, const double *y, const uint8_t *has_y,
                                    double *bound, uint8_t *screened) {
    mipx::SupScreenArgs a;
    a.m = p->m; a.n = p->n; a.pi0 = pi0; a.screen_tol = screen_tol;
    a.A = p->dA; a.b = p->db; a.pi = pi; a.l = l; a.u = u; a.y = y; a.has_y = has_y; a.bound = bound; a.screened = screened;
    return a;
}

int sup_launch_screen(mipx_ctx *ctx, const mipx::SupScreenArgs &a, int T) {
    enqueue_support_screen(a, T, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
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
    return mipx_tree_support_open_ex(t, ids, K, 0, out);
}

int mipx_tree_support_open_ex(mipx_tree *t, const int64_t *ids, int64_t K, int flags, mipx_support **out) {
    if (!t || !out) return MIPX_EINVAL;
    *out = nullptr;
    mipx_ctx *ctx = t->ctx;
    if (flags & ~MIPX_SUPPORT_KEEP_DUALS) return fail(ctx, MIPX_EINVAL, "mipx_tree_support_open_ex: unknown flag");
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
    if (!rc && (flags & MIPX_SUPPORT_KEEP_DUALS)) {
        const size_t m = (size_t)t->m;
        s->keep = true;
        rc = dmalloc(ctx, &s->d_y, T * m) | dmalloc(ctx, &s->d_bound, T) | dmalloc(ctx, &s->d_has_y, T) | dmalloc(ctx, &s->d_scr, T) |
             dmalloc(ctx, &s->d_pack, T) | dmalloc(ctx, &s->d_seg_count, G) | dmalloc(ctx, &s->d_seg_min, G) | dmalloc(ctx, &s->d_info, 1) |
             dmalloc(ctx, &s->p_l, T * n) | dmalloc(ctx, &s->p_u, T * n) | dmalloc(ctx, &s->p_x, T * n) | dmalloc(ctx, &s->p_obj, T) |
             dmalloc(ctx, &s->p_y, T * m) | dmalloc(ctx, &s->p_v[0], T * nv) | dmalloc(ctx, &s->p_v[1], T * nv) |
             dmalloc(ctx, &s->p_status, T) | dmalloc(ctx, &s->p_iters, T) | dmalloc(ctx, &s->p_np, T);
        for (hipEvent_t &e : s->ev)
            if (!rc && hipEventCreate(&e) != hipSuccess) rc = fail(ctx, MIPX_EHIP, "mipx_tree_support_open_ex: events");
        if (!rc && T > 0 && hipMemsetAsync(s->d_has_y, 0, T, ctx->stream) != hipSuccess)
            rc = fail(ctx, MIPX_EHIP, "mipx_tree_support_open_ex: memset");
        s->bytes += (int64_t)(2 * T * m * 8 + T * 8 + 2 * T + T * 4 + G * 12 + sizeof(mipx::SupPackInfo) + 3 * T * n * 8 + T * 8 +
                              2 * T * nv + 3 * T * 4);
    }
    if (!rc && K > 0) rc = sup_bounds(s);
    if (!rc && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = fail(ctx, MIPX_EHIP, "mipx_tree_support_open: sync");
    if (rc) { sup_free(s); return rc; }
    *out = s;
    return MIPX_OK;
}

int mipx_tree_support_eval(mipx_support *s, const double *pi, double pi0, double tol, int max_points,
                           double *block, double *margins) {
    return mipx_tree_support_eval_ex(s, pi, pi0, tol, -1.0, 0, max_points, block, margins, nullptr);
}

int mipx_tree_support_eval_ex(mipx_support *s, const double *pi, double pi0, double tol, double screen_tol, int retry_cold,
                              int max_points, double *block, double *margins, double *extra) {
    if (!s || !s->t) return MIPX_EINVAL;
    mipx_tree *t = s->t;
    mipx_ctx *ctx = t->ctx;
    if (!pi || !block || max_points < 1 || max_points > mipx::kSupMaxP || !(tol >= 0.0) || screen_tol != screen_tol)
        return fail(ctx, MIPX_EINVAL, "mipx_tree_support_eval: bad argument");
    const bool screening = screen_tol >= 0.0;
    if ((screening || retry_cold) && !s->keep)
        return fail(ctx, MIPX_EINVAL, "mipx_tree_support_eval_ex: screening and the cold retry need a session opened with MIPX_SUPPORT_KEEP_DUALS");
    if (screening && (s->m > mipx::kScrMax || s->n > mipx::kScrMax))
        return fail(ctx, MIPX_ETOOBIG, "mipx_tree_support_eval_ex: the screen takes 1024 rows and columns at most");
    uint32_t used = 0;   // the events of sup_tick recorded in this evaluation
    int64_t n_screened = 0, n_solved = 0, n_retried = 0, n_retried_ok = 0;
    double min_screened = std::numeric_limits<double>::infinity();
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
    if (s->T > 0 && screening && !s->first) {
        // the leaves whose duals on record prove h_t(pi) >= pi0 - screen_tol get no LP; the others are packed and solved
        mipx::SupScreenArgs sa = sup_screen_args(t->prob, s->d_pi, pi0, screen_tol, s->d_l, s->d_u, s->d_y,
                                                 s->d_has_y, s->d_bound, s->d_scr);
        sa.obj = s->d_obj; sa.status = s->d_status; sa.iters = s->d_iters; sa.npivots = s->d_np;
        mipx::SupPackInfo info;
        sup_tick(s, 0, used);
        if ((rc = sup_launch_screen(ctx, sa, (int)s->T))) return rc;
        rc = sup_pack(s, sup_pack_args(s, false, pi0), &info);
        sup_tick(s, 1, used);
        if (rc) return rc;
        n_solved = info.count;
        n_screened = s->T - info.count;
        min_screened = info.min_margin;
        if (info.count > 0 && (rc = sup_solve_packed(s, info.count, true, false, 1, used))) return rc;
    } else if (s->T > 0) {
        // (a first evaluation with screening on has no duals to screen with: it records them)
        double *y = screening ? s->d_y : nullptr;
        if ((rc = sup_launch_lps(s, s->first ? t->tr.have_root : true, y))) return rc;
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
                if (s->T > 0 && ((rc = sup_bounds(s)) || (rc = sup_launch_lps(s, t->tr.have_root, y)))) return rc;
            }
        }
        n_solved = s->T;
        if (y && s->T > 0) {   // whose duals are on record now
            enqueue_support_mark((int)s->T, s->d_status, s->d_has_y, st);
            HIP_TRY(ctx, hipGetLastError());
        }
    }
    if (retry_cold && s->T > 0) {   // the leaves whose LP did not end optimal, once more without a basis
        mipx::SupPackInfo info;
        sup_tick(s, 6, used);
        rc = sup_pack(s, sup_pack_args(s, true, pi0), &info);
        sup_tick(s, 7, used);
        if (rc) return rc;
        n_retried = info.count;
        if (info.count > 0) {
            if ((rc = sup_solve_packed(s, info.count, false, true, 4, used))) return rc;
            std::vector<int32_t> status((size_t)info.count);
            HIP_TRY(ctx, hipMemcpyAsync(status.data(), s->p_status, (size_t)info.count * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(ctx, hipStreamSynchronize(st));
            for (int32_t v : status) n_retried_ok += v == 0 ? 1 : 0;
        }
    }
    s->first = false;
    HIP_TRY(ctx, hipEventRecord(s->e1, st));
    if (s->T > 0) {
        mipx::SupSelectArgs a;
        a.n = s->n; a.P = P;
        a.pi0 = pi0; a.tol = tol;
        a.ids = s->d_ids; a.status = s->d_status; a.obj = s->d_obj; a.x = s->d_x; a.iters = s->d_iters; a.npivots = s->d_np;
        a.margin = s->d_margin; a.cand_m = s->d_cand_m; a.cand_id = s->d_cand_id; a.cand_t = s->d_cand_t;
        a.seg_sum = s->d_seg; a.block = s->d_block;
        enqueue_support_select(a, (int)s->T, st);
        HIP_TRY(ctx, hipGetLastError());
        enqueue_support_select_merge(a, (int)s->T, st);
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
        t->tr.resolved += n_solved + n_retried;
    }
    if (extra) {
        double us = 0.0;
        for (int k = 0; k < mipx_support::kPairs; k++)
            if ((used >> (2 * k) & 3u) == 3u && hipEventElapsedTime(&ms, s->ev[2 * k], s->ev[2 * k + 1]) == hipSuccess) us += 1000.0 * ms;
        extra[0] = (double)n_screened; extra[1] = (double)n_solved; extra[2] = min_screened;
        extra[3] = (double)n_retried; extra[4] = (double)n_retried_ok; extra[5] = us;
    }
    return MIPX_OK;
}

int mipx_support_screen_batch(mipx_problem *p, int64_t T, const double *pi, double pi0, double screen_tol, const double *l,
                              const double *u, const double *y, const uint8_t *has_y, double *bound_out,
                              uint8_t *screened_out, int32_t *packed_out, int32_t *count_out) {
    if (!p) return MIPX_EINVAL;
    mipx_ctx *ctx = p->ctx;
    if (T < 0 || T > (int64_t)1 << 30 || !pi || !count_out || !(screen_tol >= 0.0) || pi0 != pi0 ||
        (T && (!l || !u || !y || !has_y || !bound_out || !screened_out || !packed_out)))
        return fail(ctx, MIPX_EINVAL, "mipx_support_screen_batch: bad argument");
    if (p->m > mipx::kScrMax || p->n > mipx::kScrMax)
        return fail(ctx, MIPX_ETOOBIG, "mipx_support_screen_batch: more than 1024 rows or columns");
    *count_out = 0;
    if (T == 0) return MIPX_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t K = (size_t)T, n = (size_t)p->n, m = (size_t)p->m, G = (size_t)sup_segments(T);
    Staging S(ctx, "mipx_support_screen_batch");
    const size_t o_pi = S.in(pi, n * 8), o_l = S.in(l, K * n * 8), o_u = S.in(u, K * n * 8), o_y = S.in(y, K * m * 8),
                 o_h = S.in(has_y, K), o_b = S.out(bound_out, K * 8), o_s = S.out(screened_out, K), o_p = S.out(packed_out, K * 4),
                 o_sc = S.carve(G * 4), o_sm = S.carve(G * 8), o_i = S.carve(sizeof(mipx::SupPackInfo));
    int rc = S.alloc(p->scratch, p->scratch_bytes);
    if (rc == MIPX_OK) rc = S.upload();
    mipx::SupPackInfo info = {0, 0, 0.0};
    if (rc == MIPX_OK && hipMemsetAsync(S.at<char>(o_p), 0xff, K * 4, ctx->stream) != hipSuccess)   // (entries past the count read -1)
        rc = fail(ctx, MIPX_EHIP, "mipx_support_screen_batch: memset");
    if (rc == MIPX_OK)
        rc = sup_launch_screen(ctx, sup_screen_args(p, S.at<const double>(o_pi), pi0, screen_tol, S.at<const double>(o_l),
                                                    S.at<const double>(o_u), S.at<const double>(o_y), S.at<const uint8_t>(o_h),
                                                    S.at<double>(o_b), S.at<uint8_t>(o_s)), (int)T);
    if (rc == MIPX_OK) {
        mipx::SupPackArgs a;
        a.skip = S.at<const uint8_t>(o_s); a.bound = S.at<const double>(o_b); a.pi0 = pi0;
        a.seg_count = S.at<int32_t>(o_sc); a.seg_min = S.at<double>(o_sm); a.packed = S.at<int32_t>(o_p);
        a.info = S.at<mipx::SupPackInfo>(o_i);
        enqueue_support_pack_count(a, (int)T, ctx->stream);
        enqueue_support_pack(a, (int)T, ctx->stream);
        if (hipGetLastError() != hipSuccess) rc = fail(ctx, MIPX_EHIP, "mipx_support_screen_batch: launch");
        else if (hipMemcpyAsync(&info, a.info, sizeof info, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
            rc = fail(ctx, MIPX_EHIP, "mipx_support_screen_batch: copy");
    }
    rc = S.finish(rc);
    if (rc == MIPX_OK) *count_out = info.count;
    return rc;
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
