// wrepair_api.hip.h -- the C entries of include/mipx_wrepair.h (included at the end of tree_engine.hip.h, which holds
// the launch and the per-step halves: wr_launch, and the option's parts of heur_step_launch and heur_step_collect).

extern "C" {

int mipx_weighted_repair_batch(mipx_problem *p, int batch, const double *x, const double *l, const double *u,
                               const int32_t *int_idx, int n_int, double tol, int max_steps, const uint8_t *skip,
                               const int32_t *gate, double *x_out, double *obj_out, int32_t *status_out,
                               int32_t *counts_out) {
    if (!p) return MIPX_EINVAL;
    mipx_ctx *ctx = p->ctx;
    if (batch < 0 || n_int < 0 || n_int > p->n || !(tol >= 0.0) || max_steps < 0 || !l || !u || (n_int && !int_idx) ||
        (batch && (!x || !x_out || !obj_out || !status_out || !counts_out)))
        return fail(ctx, MIPX_EINVAL, "mipx_weighted_repair_batch: bad argument");
    std::vector<uint8_t> seen((size_t)p->n, 0);
    for (int k = 0; k < n_int; k++) {
        if (int_idx[k] < 0 || int_idx[k] >= p->n || seen[(size_t)int_idx[k]])
            return fail(ctx, MIPX_EINVAL, "mipx_weighted_repair_batch: int_idx out of range or repeated");
        seen[(size_t)int_idx[k]] = 1;
    }
    if (p->m > mipx::kWrMax || p->n > mipx::kWrMax)
        return fail(ctx, MIPX_ETOOBIG, "mipx_weighted_repair_batch: more than 1024 rows or columns");
    const size_t B = (size_t)batch, nn = (size_t)p->n;
    for (size_t e = 0; e < nn; e++)
        if (!std::isfinite(l[e]) || u[e] != u[e] || u[e] == -std::numeric_limits<double>::infinity())
            return fail(ctx, MIPX_EINVAL, "mipx_weighted_repair_batch: a lower bound that is not finite, or an upper bound that is NaN or -inf");
    for (size_t e = 0; e < B * nn; e++)
        if (!std::isfinite(x[e])) return fail(ctx, MIPX_EINVAL, "mipx_weighted_repair_batch: a point that is not finite");
    if (batch == 0) return MIPX_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Staging S(ctx, "mipx_weighted_repair_batch");
    const size_t o_x = S.in(x, B * nn * 8), o_l = S.in(l, nn * 8), o_u = S.in(u, nn * 8),
                 o_ii = S.in(n_int ? int_idx : nullptr, (size_t)(n_int ? n_int : 1) * 4), o_sk = S.in(skip, B),
                 o_gt = S.in(gate, B * 4), o_xo = S.out(x_out, B * nn * 8), o_ob = S.out(obj_out, B * 8),
                 o_st = S.out(status_out, B * 4), o_ct = S.out(counts_out, B * 8);
    int rc = S.alloc(p->scratch, p->scratch_bytes);
    if (rc == MIPX_OK) rc = S.upload();
    if (rc == MIPX_OK)
        rc = wr_launch(p, ctx->stream, batch, S.at<const double>(o_x), S.at<const double>(o_l), S.at<const double>(o_u),
                       S.at<const int32_t>(o_ii), n_int, tol, max_steps, skip ? S.at<const uint8_t>(o_sk) : nullptr,
                       gate ? S.at<const int32_t>(o_gt) : nullptr, false, S.at<double>(o_xo), S.at<double>(o_ob),
                       S.at<int32_t>(o_st), S.at<int32_t>(o_ct));
    return S.finish(rc);
}

int mipx_tree_set_weighted_repair(mipx_tree *t, int max_steps) {
    if (!t) return MIPX_EINVAL;
    mipx_ctx *ctx = t->ctx;
    if (max_steps < 0) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_weighted_repair: max_steps is not negative");
    if (!t->hr.on)
        return fail(ctx, MIPX_EINVAL, "mipx_tree_set_weighted_repair: the repair runs on the heuristic's points (mipx_tree_set_heuristic first)");
    if (t->cuts) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_weighted_repair: not with cut rounds");
    if (t->comm) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_weighted_repair: not with a communicator");
    if (t->steps > 0 || t->evaluated > 0)
        return fail(ctx, MIPX_EINVAL, "mipx_tree_set_weighted_repair: the repair is set before the first step");
    WrState &wr = t->wr;
    if (max_steps == 0) {   // (the buffers stay)
        wr.on = false;
        return MIPX_OK;
    }
    if (t->fp.on)
        return fail(ctx, MIPX_EINVAL, "mipx_tree_set_weighted_repair: not with the fix-and-propagate dive (mipx_tree_set_fix_propagate(t, 1, 0) first)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (t->hr.cap > wr.cap) {   // (the heuristic's step buffers grew or are new: nothing is in flight before the first step)
        const size_t out_bytes = step_layout::WrOut((size_t)t->hr.cap).bytes();
        for (int k = 0; k < 3; k++) {
            if (wr.d_out[k]) (void)hipFree(wr.d_out[k]);
            if (wr.h_out[k]) (void)hipHostFree(wr.h_out[k]);
            wr.d_out[k] = nullptr; wr.h_out[k] = nullptr;
            int rc = dmalloc(ctx, &wr.d_out[k], out_bytes);
            if (rc) return rc;
            HIP_TRY(ctx, hipHostMalloc((void **)&wr.h_out[k], out_bytes));
            if (!wr.e0[k]) HIP_TRY(ctx, hipEventCreate(&wr.e0[k]));
            if (!wr.e1[k]) HIP_TRY(ctx, hipEventCreate(&wr.e1[k]));
        }
        wr.cap = t->hr.cap;   // (laid out for wr.cap points: step_layout::WrOut)
    }
    wr.max_steps = max_steps;
    wr.on = true;
    return MIPX_OK;
}

int mipx_tree_weighted_repair_stats(mipx_tree *t, int64_t out[8]) {
    if (!t || !out) return MIPX_EINVAL;
    const WrState &wr = t->wr;
    out[0] = wr.tried; out[1] = wr.feasible; out[2] = wr.capped; out[3] = wr.moves; out[4] = wr.bumps;
    out[5] = wr.installed; out[6] = 0; out[7] = (int64_t)wr.us;
    return MIPX_OK;
}

}  // extern "C"
