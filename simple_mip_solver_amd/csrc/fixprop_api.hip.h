// fixprop_api.hip.h -- the C entries of include/mipx_fixprop.h (included at the end of tree_engine.hip.h, which holds
// the launch and the per-step halves: fp_launch, and the dive's parts of heur_step_launch and heur_step_collect).
// The buffers behind the option's step block are a StepRing (tree_engine.hip.h): the set entry switches the option off,
// grows the ring, and switches it on last.  The batch entry's prologue is the shared one of mipx.hip (check_int_idx, ...).

extern "C" {

int mipx_fix_propagate_batch(mipx_problem *p, int batch, const double *x, const double *l, const double *u,
                             const int32_t *int_idx, int n_int, double cutoff, double tol, int max_rounds,
                             int max_tries, const uint8_t *skip, double *x_out, double *obj_out, int32_t *status_out,
                             int32_t *counts_out) {
    if (!p) return MIPX_EINVAL;
    mipx_ctx *ctx = p->ctx;
    if (batch < 0 || n_int < 0 || n_int > p->n || !(tol >= 0.0) || max_rounds < 1 || max_tries < 0 || cutoff != cutoff || !l || !u ||
        (n_int && !int_idx) || (batch && (!x || !x_out || !obj_out || !status_out || !counts_out)))
        return fail(ctx, MIPX_EINVAL, "mipx_fix_propagate_batch: bad argument");
    if (int rc = check_int_idx(ctx, "mipx_fix_propagate_batch", int_idx, n_int, p->n)) return rc;
    if (p->m > mipx::kFpMax || p->n > mipx::kFpMax)
        return fail(ctx, MIPX_ETOOBIG, "mipx_fix_propagate_batch: more than 1024 rows or columns");
    const size_t B = (size_t)batch, nn = (size_t)p->n;
    if (int rc = check_bounds(ctx, "mipx_fix_propagate_batch", nullptr, l, u, nn)) return rc;
    if (int rc = check_points(ctx, "mipx_fix_propagate_batch", x, B * nn)) return rc;
    if (batch == 0) return MIPX_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Staging S(ctx, "mipx_fix_propagate_batch");
    const size_t o_x = S.in(x, B * nn * 8), o_l = S.in(l, nn * 8), o_u = S.in(u, nn * 8),
                 o_ii = S.in(n_int ? int_idx : nullptr, (size_t)(n_int ? n_int : 1) * 4), o_sk = S.in(skip, B),
                 o_xo = S.out(x_out, B * nn * 8), o_ob = S.out(obj_out, B * 8), o_st = S.out(status_out, B * 4),
                 o_ct = S.out(counts_out, B * 8);
    int rc = S.alloc(p->scratch, p->scratch_bytes);
    if (rc == MIPX_OK) rc = S.upload();
    if (rc == MIPX_OK)
        rc = fp_launch(p, ctx->stream, batch, S.at<const double>(o_x), S.at<const double>(o_l), S.at<const double>(o_u),
                       S.at<const int32_t>(o_ii), n_int, cutoff, tol, max_rounds, max_tries, skip ? S.at<const uint8_t>(o_sk) : nullptr,
                       nullptr, S.at<double>(o_xo), S.at<double>(o_ob), S.at<int32_t>(o_st), S.at<int32_t>(o_ct));
    return S.finish(rc);
}

int mipx_tree_set_fix_propagate(mipx_tree *t, int max_rounds, int max_tries) {
    if (!t) return MIPX_EINVAL;
    mipx_ctx *ctx = t->ctx;
    if (max_rounds < 1 || max_tries < 0)
        return fail(ctx, MIPX_EINVAL, "mipx_tree_set_fix_propagate: max_rounds is positive and max_tries is not negative");
    if (!t->hr.on)
        return fail(ctx, MIPX_EINVAL, "mipx_tree_set_fix_propagate: the dive runs on the heuristic's points (mipx_tree_set_heuristic first)");
    if (t->cuts) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_fix_propagate: not with cut rounds");
    if (t->comm) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_fix_propagate: not with a communicator");
    if (t->steps > 0 || t->evaluated > 0)
        return fail(ctx, MIPX_EINVAL, "mipx_tree_set_fix_propagate: the dive is set before the first step");
    FpState &fp = t->fp;
    if (max_tries == 0) {   // (the buffers stay)
        fp.on = false;
        return MIPX_OK;
    }
    if (t->wr.on)
        return fail(ctx, MIPX_EINVAL, "mipx_tree_set_fix_propagate: not with the weighted row repair (mipx_tree_set_weighted_repair(t, 0) first)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (t->hr.cap > fp.cap) {   // (the heuristic's step buffers grew or are new: nothing is in flight before the first step)
        fp.on = false;   // (until every block is there: a failure below leaves the option off and nothing to launch on)
        fp.cap = 0;
        const int rc = fp.ring.grow(ctx, step_layout::FpOut((size_t)t->hr.cap).bytes(), 0);
        if (rc) return rc;
        fp.cap = t->hr.cap;   // (laid out for fp.cap points: step_layout::FpOut)
    }
    fp.max_rounds = max_rounds;
    fp.max_tries = max_tries;
    fp.on = true;
    return MIPX_OK;
}

int mipx_tree_fix_propagate_stats(mipx_tree *t, int64_t out[8]) {
    if (!t || !out) return MIPX_EINVAL;
    const FpState &fp = t->fp;
    out[0] = fp.tried; out[1] = fp.feasible; out[2] = fp.stuck; out[3] = fp.capped; out[4] = fp.fixings; out[5] = fp.tries;
    out[6] = fp.installed; out[7] = (int64_t)fp.us;
    return MIPX_OK;
}

}  // extern "C"
