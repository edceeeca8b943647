// complete_api.hip.h -- the C entries of include/mipx_complete.h (included at the end of tree_engine.hip.h, which holds
// the launch and the per-step halves: comp_launch, and the option's parts of heur_step_launch and heur_step_collect).
// The buffers behind the option's step block are a StepRing (tree_engine.hip.h): the set entry switches the option off,
// grows the ring, and switches it on last.  The batch entry's prologue is the shared one of mipx.hip (check_int_idx, ...).

extern "C" {

int mipx_complete_batch(mipx_problem *p, int batch, const double *x, const double *l, const double *u,
                        const int32_t *int_idx, int n_int, const int8_t *vstat, double ctol, const uint8_t *skip,
                        double *x_out, double *obj_out, int32_t *status_out, int32_t *pivots_out) {
    if (!p) return MIPX_EINVAL;
    mipx_ctx *ctx = p->ctx;
    if (batch < 0 || n_int < 0 || n_int > p->n || !(ctol >= 0.0) || !l || !u || (n_int && !int_idx) ||
        (batch && (!x || !x_out || !obj_out || !status_out || !pivots_out)))
        return fail(ctx, MIPX_EINVAL, "mipx_complete_batch: bad argument");
    std::vector<uint8_t> is_int;
    if (int rc = check_int_idx(ctx, "mipx_complete_batch", int_idx, n_int, p->n, "int_idx out of range or repeated", &is_int)) return rc;
    if (p->m > mipx::kCompMax || p->n > mipx::kCompMax)
        return fail(ctx, MIPX_ETOOBIG, "mipx_complete_batch: more than 1024 rows or columns");
    const size_t B = (size_t)batch, nn = (size_t)p->n, nv = nn + (size_t)p->m;
    // (its own pass, not check_bounds: the two refusals alternate column by column, and the first bad column decides)
    for (size_t e = 0; e < nn; e++) {
        if (!std::isfinite(l[e]) || u[e] != u[e] || u[e] == -std::numeric_limits<double>::infinity())
            return fail(ctx, MIPX_EINVAL, "mipx_complete_batch: a lower bound that is not finite, or an upper bound that is NaN or -inf");
        if (is_int[e] && !std::isfinite(u[e]))
            return fail(ctx, MIPX_EINVAL, "mipx_complete_batch: an integer column whose upper bound is not finite");
    }
    if (int rc = check_points(ctx, "mipx_complete_batch", x, B * nn)) return rc;
    if (batch == 0) return MIPX_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Staging S(ctx, "mipx_complete_batch");
    const size_t o_x = S.in(x, B * nn * 8), o_l = S.in(l, nn * 8), o_u = S.in(u, nn * 8),
                 o_ii = S.in(n_int ? int_idx : nullptr, (size_t)(n_int ? n_int : 1) * 4), o_sk = S.in(skip, B),
                 o_vs = S.in(vstat, B * nv), o_ws = S.carve(mipx::CompWs(B, (size_t)p->m, nn).bytes()),
                 o_xo = S.out(x_out, B * nn * 8), o_ob = S.out(obj_out, B * 8), o_st = S.out(status_out, B * 4),
                 o_pv = S.out(pivots_out, B * 4);
    int rc = S.alloc(p->scratch, p->scratch_bytes);
    if (rc == MIPX_OK) rc = S.upload();
    if (rc == MIPX_OK) {
        const CompSrc src = {S.at<const double>(o_x), skip ? S.at<const uint8_t>(o_sk) : nullptr, nullptr, false,
                             vstat ? S.at<const int8_t>(o_vs) : nullptr, batch};
        rc = comp_launch(p, ctx->stream, &src, 1, S.at<const double>(o_l), S.at<const double>(o_u), S.at<const int32_t>(o_ii),
                         n_int, ctol, S.at<char>(o_ws), S.at<double>(o_xo), S.at<double>(o_ob), S.at<int32_t>(o_st),
                         S.at<int32_t>(o_pv));
    }
    return S.finish(rc);
}

int mipx_tree_set_completion(mipx_tree *t, int on) {
    if (!t) return MIPX_EINVAL;
    mipx_ctx *ctx = t->ctx;
    if (!t->hr.on)
        return fail(ctx, MIPX_EINVAL, "mipx_tree_set_completion: the completion runs on the heuristics' points (mipx_tree_set_heuristic first)");
    if (t->cuts) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_completion: not with cut rounds");
    if (t->comm) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_completion: not with a communicator");
    if (t->steps > 0 || t->evaluated > 0)
        return fail(ctx, MIPX_EINVAL, "mipx_tree_set_completion: the completion is set before the first step");
    CompState &cc = t->cc;
    if (!on) {   // (the buffers stay)
        cc.on = false;
        return MIPX_OK;
    }
    if (t->prob->m > mipx::kCompMax || t->prob->n > mipx::kCompMax)
        return fail(ctx, MIPX_ETOOBIG, "mipx_tree_set_completion: more than 1024 rows or columns");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (t->n_int < t->n && t->hr.cap > cc.cap) {   // (the heuristic's step buffers grew or are new: nothing is in flight before the first step)
        const size_t cap = (size_t)t->hr.cap, out_bytes = step_layout::CompOut(cap).bytes();
        cc.on = false;   // (until every block is there: a failure below leaves the option off and nothing to launch on)
        cc.cap = 0;
        if (cc.d_ws) (void)hipFree(cc.d_ws);
        cc.d_ws = nullptr;
        int rc = dmalloc(ctx, &cc.d_ws, mipx::CompWs(2 * cap, (size_t)t->prob->m, (size_t)t->n).bytes());
        if (rc) return rc;
        if ((rc = cc.ring.grow(ctx, out_bytes, 2 * cap * (size_t)t->n))) return rc;
        cc.cap = t->hr.cap;   // (laid out for cc.cap points per block: step_layout::CompOut)
    }
    if (t->n_int == t->n) cc.cap = std::max(cc.cap, t->hr.cap);   // (no continuous column: nothing is ever launched, no buffer is needed)
    cc.on = true;
    return MIPX_OK;
}

int mipx_tree_completion_stats(mipx_tree *t, int64_t out[8]) {
    if (!t || !out) return MIPX_EINVAL;
    const CompState &cc = t->cc;
    out[0] = cc.tried; out[1] = cc.completed; out[2] = cc.infeasible; out[3] = cc.failed; out[4] = cc.rescued;
    out[5] = cc.installed; out[6] = cc.pivots; out[7] = (int64_t)cc.us;
    return MIPX_OK;
}

}  // extern "C"
