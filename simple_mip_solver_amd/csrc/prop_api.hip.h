// prop_api.hip.h -- the C entries of include/mipx_prop.h (included at the end of tree_engine.hip.h, which holds
// the launch and the per-step halves: prop_launch, prop_step_launch, prop_step_collect).
// The buffers behind the option's step block are a StepRing (tree_engine.hip.h): the set entry switches the option off,
// grows the ring, and switches it on last.  The batch entry's prologue is the shared one of mipx.hip (check_int_idx, ...).

extern "C" {

int mipx_propagate_batch(mipx_problem *p, int batch, const double *l, const double *u, const int32_t *int_idx,
                         int n_int, double cutoff, double tol, int max_rounds, double *l_out, double *u_out,
                         int32_t *status_out, int32_t *changed_out, int32_t *rounds_out) {
    if (!p) return MIPX_EINVAL;
    mipx_ctx *ctx = p->ctx;
    if (batch < 0 || n_int < 0 || n_int > p->n || !(tol >= 0.0) || max_rounds < 1 || cutoff != cutoff || (n_int && !int_idx) ||
        (batch && (!l || !u || !l_out || !u_out || !status_out || !changed_out || !rounds_out)))
        return fail(ctx, MIPX_EINVAL, "mipx_propagate_batch: bad argument");
    if (int rc = check_int_idx(ctx, "mipx_propagate_batch", int_idx, n_int, p->n)) return rc;
    if (p->m > mipx::kPropMax || p->n > mipx::kPropMax)
        return fail(ctx, MIPX_ETOOBIG, "mipx_propagate_batch: more than 1024 rows or columns");
    const size_t B = (size_t)batch, nn = (size_t)p->n;
    if (int rc = check_bounds(ctx, "mipx_propagate_batch", nullptr, l, u, B * nn)) return rc;
    if (batch == 0) return MIPX_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Staging S(ctx, "mipx_propagate_batch");
    const size_t o_l = S.in(l, B * nn * 8), o_u = S.in(u, B * nn * 8),
                 o_ii = S.in(n_int ? int_idx : nullptr, (size_t)(n_int ? n_int : 1) * 4),
                 o_lo = S.out(l_out, B * nn * 8), o_uo = S.out(u_out, B * nn * 8), o_st = S.out(status_out, B * 4),
                 o_ch = S.out(changed_out, B * 4), o_rd = S.out(rounds_out, B * 4);
    int rc = S.alloc(p->scratch, p->scratch_bytes);
    if (rc == MIPX_OK) rc = S.upload();
    if (rc == MIPX_OK)
        rc = prop_launch(p, ctx->stream, batch, nullptr, S.at<const double>(o_l), S.at<const double>(o_u),
                         S.at<const int32_t>(o_ii), n_int, cutoff, tol, max_rounds, S.at<double>(o_lo), S.at<double>(o_uo),
                         S.at<int32_t>(o_st), S.at<int32_t>(o_ch), S.at<int32_t>(o_rd), nullptr);
    return S.finish(rc);
}

int mipx_tree_set_propagation(mipx_tree *t, int max_rounds, int use_cutoff) {
    if (!t) return MIPX_EINVAL;
    mipx_ctx *ctx = t->ctx;
    if (max_rounds < 1) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_propagation: max_rounds is positive");
    if (t->cuts) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_propagation: not with cut rounds");
    if (t->comm) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_propagation: not with a communicator");
    if (t->df.on) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_propagation: not with the dual function (mipx_tree_set_dual_record)");
    if (t->tr.on) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_propagation: not with the tree record (mipx_tree_set_tree_record)");
    if (t->steps > 0 || t->evaluated > 0)
        return fail(ctx, MIPX_EINVAL, "mipx_tree_set_propagation: the propagation is set before the first step");
    if (t->m > mipx::kPropMax || t->n > mipx::kPropMax)
        return fail(ctx, MIPX_ETOOBIG, "mipx_tree_set_propagation: more than 1024 rows or columns");
    PropState &pg = t->pg;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (pg.cap == 0) {
        pg.on = false;   // (until every block is there: a failure below leaves the option off and nothing to launch on)
        const int rc = pg.ring.grow(ctx, step_layout::PropOut((size_t)t->max_batch).bytes(), 0);
        if (rc) return rc;
        pg.cap = t->max_batch;   // (the step buffers are laid out for pg.cap nodes: step_layout::PropOut)
    }
    pg.max_rounds = max_rounds;
    pg.use_cutoff = use_cutoff ? 1 : 0;
    pg.on = true;
    // a node found infeasible is closed by the host before the step's nodes are evaluated: every step is finished
    // on the host, the switch mipx_tree_set_dual_record and mipx_tree_set_tree_record use
    t->fast_ok = false;
    return MIPX_OK;
}

int mipx_tree_propagation_stats(mipx_tree *t, int64_t out[8]) {
    if (!t || !out) return MIPX_EINVAL;
    const PropState &pg = t->pg;
    out[0] = pg.nodes; out[1] = pg.tightened; out[2] = pg.infeasible; out[3] = pg.changed; out[4] = pg.rounds;
    out[5] = pg.capped; out[6] = 0; out[7] = (int64_t)pg.us;
    return MIPX_OK;
}

}  // extern "C"
