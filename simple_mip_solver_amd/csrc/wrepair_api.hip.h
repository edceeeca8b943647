// wrepair_api.hip.h -- the C entries of include/mipx_wrepair.h (included at the end of tree_engine.hip.h, which holds
// the launch and the per-step halves: wr_launch, and the option's parts of heur_step_launch and heur_step_collect).
// The buffers behind the option's step block are a StepRing (tree_engine.hip.h): the set entry switches the option off,
// grows the ring, and switches it on last.  The batch entry's prologue is the shared one of mipx.hip (check_int_idx, ...).

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
    if (int rc = check_int_idx(ctx, "mipx_weighted_repair_batch", int_idx, n_int, p->n)) return rc;
    if (p->m > mipx::kWrMax || p->n > mipx::kWrMax)
        return fail(ctx, MIPX_ETOOBIG, "mipx_weighted_repair_batch: more than 1024 rows or columns");
    const size_t B = (size_t)batch, nn = (size_t)p->n;
    if (int rc = check_bounds(ctx, "mipx_weighted_repair_batch", nullptr, l, u, nn)) return rc;
    if (int rc = check_points(ctx, "mipx_weighted_repair_batch", x, B * nn)) return rc;
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
        wr.on = false;   // (until every block is there: a failure below leaves the option off and nothing to launch on)
        wr.cap = 0;
        const int rc = wr.ring.grow(ctx, step_layout::WrOut((size_t)t->hr.cap).bytes(), 0);
        if (rc) return rc;
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
