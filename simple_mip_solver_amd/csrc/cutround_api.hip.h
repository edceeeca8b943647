// cutround_api.hip.h -- the C entries of include/mipx_cutround.h (included at the end of tree_engine.hip.h, which
// holds enqueue_cut_begin and enqueue_cut_generate): the kernels of a cut round on a caller's round.  Test
// scaffolding: no product code calls them.  Every index a kernel would follow is checked here first.

namespace {

// the rows a tree with cut rounds would allot: m0 + kc must fit where m0 does (mipx_tree_create_ex lowers kc until it
// does; a caller of the scaffolding names the kc it means)
bool cut_shape_ok(int m0, int n, int kc) {
    if (n < 1 || m0 < 1 || kc < 1 || kc > mipx::kMaxNodeCuts || !shape_supported(m0, n)) return false;
    return pick_cfg(m0, n) != nullptr ? pick_cfg(m0 + kc, n) != nullptr : big_fits(m0 + kc, n);
}

}  // namespace

extern "C" {

int mipx_cut_round_begin_batch(mipx_ctx *ctx, int n, int m0, int kc, int B, int round, int max_rounds,
                               double progress_tol, double max_dual_bound, int have_dump, int gather, int pool_rows,
                               const int32_t *slot, const int32_t *pool_ncut, const int32_t *pool_ids,
                               const int32_t *status, const double *obj, const int32_t *mipf, const double *y,
                               int8_t *vstat, int32_t *ncut, int32_t *ids, int32_t *state, double *obj_before,
                               int32_t *active, int32_t *counters, int32_t *resolve, int32_t *need_tab) {
    if (!ctx) return MIPX_EINVAL;
    const char *who = "mipx_cut_round_begin_batch";
    if (B < 1 || round < 0 || max_rounds < 0 || have_dump < 0 || have_dump > 1 || gather < 0 || gather > 1 ||
        !cut_shape_ok(m0, n, kc))
        return fail(ctx, MIPX_EINVAL, "mipx_cut_round_begin_batch: B < 1, round or max_rounds < 0, have_dump or gather outside 0..1, "
                                      "kc outside 1..64 or a shape without room for m0 + kc rows");
    if (!status || !obj || !mipf || !y || !vstat || !ncut || !ids || !state || !obj_before || !active || !counters ||
        !resolve || !need_tab)
        return fail(ctx, MIPX_EINVAL, "mipx_cut_round_begin_batch: a null argument");
    const size_t Bz = (size_t)B, K = (size_t)kc, ms = (size_t)m0 + K, nv = (size_t)n + ms;
    if (gather) {
        if (pool_rows < 1 || !slot || !pool_ncut || !pool_ids)
            return fail(ctx, MIPX_EINVAL, "mipx_cut_round_begin_batch: gather needs pool_rows >= 1, slot, pool_ncut and pool_ids");
        for (size_t k = 0; k < Bz; k++)
            if (slot[k] < 0 || slot[k] >= pool_rows) return fail(ctx, MIPX_EINVAL, "mipx_cut_round_begin_batch: a slot outside the pool");
        for (size_t r = 0; r < (size_t)pool_rows; r++)
            if (pool_ncut[r] < 0 || pool_ncut[r] > kc) return fail(ctx, MIPX_EINVAL, "mipx_cut_round_begin_batch: a pool_ncut outside 0..kc");
    } else {
        for (size_t k = 0; k < Bz; k++)
            if (ncut[k] < 0 || ncut[k] > kc) return fail(ctx, MIPX_EINVAL, "mipx_cut_round_begin_batch: an ncut outside 0..kc");
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Staging S(ctx, who);
    auto inout = [&S](void *p, size_t bytes) { const size_t o = S.in(p, bytes); S.down(p, o, bytes); return o; };
    const size_t rows = gather ? (size_t)pool_rows : 1;
    const size_t o_sl = S.in(gather ? slot : nullptr, Bz * 4), o_pn = S.in(gather ? pool_ncut : nullptr, rows * 4),
                 o_pi = S.in(gather ? pool_ids : nullptr, rows * K * 4);
    const size_t o_st = S.in(status, Bz * 4), o_ob = S.in(obj, Bz * 8), o_mf = S.in(mipf, Bz * 4), o_y = S.in(y, Bz * ms * 8);
    const size_t o_vs = inout(vstat, Bz * nv), o_nc = inout(ncut, Bz * 4), o_id = inout(ids, Bz * K * 4),
                 o_state = inout(state, (size_t)mipx::CF_FIELDS * Bz * 4), o_bef = inout(obj_before, Bz * 8),
                 o_act = inout(active, Bz * 4), o_cnt = inout(counters, 16), o_res = inout(resolve, Bz * 4),
                 o_tab = inout(need_tab, Bz * 4);
    int rc = S.alloc();
    if (rc == MIPX_OK) rc = S.upload();
    if (rc == MIPX_OK) {
        CutRoundData d;
        d.n = n; d.m0 = m0; d.mstride = (int)ms; d.kc = kc; d.B = B;
        d.round = round; d.max_rounds = max_rounds; d.have_dump = have_dump;
        d.progress_tol = progress_tol; d.max_dual_bound = max_dual_bound;
        d.status = S.at<const int32_t>(o_st); d.obj = S.at<const double>(o_ob); d.mipf = S.at<const int32_t>(o_mf);
        d.y = S.at<const double>(o_y); d.vstat = S.at<int8_t>(o_vs);
        d.ncut = S.at<int32_t>(o_nc); d.ids = S.at<int32_t>(o_id); d.state = S.at<int32_t>(o_state);
        d.obj_before = S.at<double>(o_bef); d.active = S.at<int32_t>(o_act); d.resolve = S.at<int32_t>(o_res);
        d.need_tab = S.at<int32_t>(o_tab); d.counters = S.at<int32_t>(o_cnt);
        mipx::CutGatherArgs ga;
        ga.batch = B; ga.kc = kc; ga.slot = S.at<const int32_t>(o_sl);
        ga.pool_ncut = S.at<const int32_t>(o_pn); ga.pool_ids = S.at<const int32_t>(o_pi);
        ga.ncut = d.ncut; ga.ids = d.ids; ga.state = d.state; ga.counters = d.counters;
        rc = enqueue_cut_begin(ctx, d, gather ? &ga : nullptr, true, ctx->stream);
    }
    return S.finish(rc);
}

int mipx_cut_round_generate_batch(mipx_problem *p, int B, int kc, int slab_rows, int chunks, int group, int store_cap,
                                  double max_term, int max_nonzero_coefs, double min_cut_depth, double cos_parallel,
                                  double max_abs_coef, const double *T, const int32_t *idx, const double *x,
                                  const uint8_t *is_int, const int32_t *active, int8_t *vstat, int32_t *ncut,
                                  int32_t *ids, int32_t *state, int32_t *pool_list, double *slab_pi, double *slab_pi0,
                                  double *store_pi, double *store_pi0, int32_t *store_count, int32_t *resolve,
                                  int32_t *counters, int32_t *k2_ncuts, int32_t *k3_nadded, int32_t *k3_added,
                                  int32_t *k3_term, int32_t *used) {
    if (!p) return MIPX_EINVAL;
    mipx_ctx *ctx = p->ctx;
    const char *who = "mipx_cut_round_generate_batch";
    const int n = p->n, m0 = p->m;
    if (B < 1 || slab_rows < 1 || slab_rows > 2040 || !(chunks == 0 || chunks == 1 || chunks == 4 || chunks == 16) || group < 0 ||
        group > mipx::kGomoryGroup || store_cap < 1 || !cut_shape_ok(m0, n, kc))
        return fail(ctx, MIPX_EINVAL, "mipx_cut_round_generate_batch: B < 1, kc outside 1..64, slab_rows outside 1..2040, chunks not in "
                                      "{0, 1, 4, 16}, group outside 0..8, store_cap < 1 or a shape without room for m + kc rows");
    if (max_nonzero_coefs < 1 || !(min_cut_depth > 0) || !(max_term > 0))
        return fail(ctx, MIPX_EINVAL, "mipx_cut_round_generate_batch: bad cut parameter");
    if (!T || !idx || !x || !is_int || !active || !vstat || !ncut || !ids || !state || !pool_list || !slab_pi || !slab_pi0 ||
        !store_pi || !store_pi0 || !store_count || !resolve || !counters || !k2_ncuts || !k3_nadded || !k3_added || !k3_term || !used)
        return fail(ctx, MIPX_EINVAL, "mipx_cut_round_generate_batch: a null argument");
    const size_t Bz = (size_t)B, nn = (size_t)n, K = (size_t)kc, ms = (size_t)m0 + K, nv = nn + ms, SR = (size_t)slab_rows,
                 cap = (size_t)store_cap;
    CutRoundData d;
    d.n = n; d.m0 = m0; d.mstride = (int)ms; d.kc = kc; d.B = B; d.slab_rows = slab_rows;
    cut_launch_shape(d, chunks, group);
    if (mipx::gomory_lds_bytes(n, (int)ms, group) > 160 * 1024)
        return fail(ctx, MIPX_EINVAL, "mipx_cut_round_generate_batch: the group's staging does not fit the LDS");
    // (the kernels index the store by ids, the slabs by pool_list and the two state counts, LDS by idx)
    if (store_count[0] < 0 || store_count[0] > (1 << 30))
        return fail(ctx, MIPX_EINVAL, "mipx_cut_round_generate_batch: store_count negative or above 2^30");
    std::vector<uint8_t> seen;
    for (size_t k = 0; k < Bz; k++) {
        if (ncut[k] < 0 || ncut[k] > kc) return fail(ctx, MIPX_EINVAL, "mipx_cut_round_generate_batch: an ncut outside 0..kc");
        for (int i = 0; i < ncut[k]; i++)
            if (ids[k * K + (size_t)i] < 0 || ids[k * K + (size_t)i] >= store_cap)
                return fail(ctx, MIPX_EINVAL, "mipx_cut_round_generate_batch: an id outside the store");
        const int pn = state[(size_t)mipx::CF_POOL_N * Bz + k], sn = state[(size_t)mipx::CF_SLAB_N * Bz + k];
        if (sn < 0 || sn > slab_rows || pn < 0 || pn > sn)
            return fail(ctx, MIPX_EINVAL, "mipx_cut_round_generate_batch: pool or slab count outside slab_rows");
        for (int q = 0; q < pn; q++)
            if (pool_list[k * SR + (size_t)q] < 0 || pool_list[k * SR + (size_t)q] >= slab_rows)
                return fail(ctx, MIPX_EINVAL, "mipx_cut_round_generate_batch: a pool_list entry outside slab_rows");
        if (!active[k]) continue;
        const int tot = n + m0 + ncut[k];
        seen.assign((size_t)tot, 0);
        const int32_t *ix = idx + k * (2 * nn + ms);
        for (int j = 0; j < tot; j++) {
            const int v = ix[j];
            if (v < 0 || v >= tot || seen[(size_t)v])
                return fail(ctx, MIPX_EINVAL, "mipx_cut_round_generate_batch: idx is not a split of the node's variables");
            seen[(size_t)v] = 1;
        }
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Staging S(ctx, who);
    auto inout = [&S](void *q, size_t bytes) { const size_t o = S.in(q, bytes); S.down(q, o, bytes); return o; };
    const size_t o_T = S.in(T, Bz * ms * nn * 8), o_ix = S.in(idx, Bz * (2 * nn + ms) * 4), o_x = S.in(x, Bz * nn * 8),
                 o_int = S.in(is_int, nn), o_act = S.in(active, Bz * 4);
    const size_t o_vs = inout(vstat, Bz * nv), o_nc = inout(ncut, Bz * 4), o_id = inout(ids, Bz * K * 4),
                 o_state = inout(state, (size_t)mipx::CF_FIELDS * Bz * 4), o_pl = inout(pool_list, Bz * SR * 4),
                 o_sp = inout(slab_pi, Bz * SR * nn * 8), o_s0 = inout(slab_pi0, Bz * SR * 8), o_tp = inout(store_pi, cap * nn * 8),
                 o_t0 = inout(store_pi0, cap * 8), o_tc = inout(store_count, 4), o_res = inout(resolve, Bz * 4),
                 o_cnt = inout(counters, 16), o_k2 = inout(k2_ncuts, Bz * 4), o_na = inout(k3_nadded, Bz * 4),
                 o_ad = inout(k3_added, Bz * SR * 4), o_te = inout(k3_term, Bz * 4);
    int rc = S.alloc();
    if (rc == MIPX_OK) rc = S.upload();
    if (rc == MIPX_OK) {
        d.A = p->dA; d.b = p->db; d.T = S.at<const double>(o_T); d.idx = S.at<const int32_t>(o_ix); d.x = S.at<const double>(o_x);
        d.is_int = S.at<const uint8_t>(o_int); d.active = S.at<int32_t>(o_act);
        d.max_term = max_term; d.max_nonzero_coefs = max_nonzero_coefs; d.min_cut_depth = min_cut_depth;
        d.cos_parallel = cos_parallel; d.max_abs_coef = max_abs_coef;
        d.vstat = S.at<int8_t>(o_vs); d.ncut = S.at<int32_t>(o_nc); d.ids = S.at<int32_t>(o_id); d.state = S.at<int32_t>(o_state);
        d.pool_list = S.at<int32_t>(o_pl); d.slab_pi = S.at<double>(o_sp); d.slab_pi0 = S.at<double>(o_s0);
        d.store_pi = S.at<double>(o_tp); d.store_pi0 = S.at<double>(o_t0); d.store_count = S.at<int32_t>(o_tc);
        d.store_cap = store_cap; d.resolve = S.at<int32_t>(o_res); d.counters = S.at<int32_t>(o_cnt);
        d.k2_ncuts = S.at<int32_t>(o_k2); d.k3_nadded = S.at<int32_t>(o_na); d.k3_added = S.at<int32_t>(o_ad);
        d.k3_term = S.at<int32_t>(o_te);
        rc = enqueue_cut_generate(ctx, d, chunks, group, ctx->stream);
    }
    rc = S.finish(rc);
    if (rc == MIPX_OK) { used[0] = chunks; used[1] = group; }
    return rc;
}

}  // extern "C"
