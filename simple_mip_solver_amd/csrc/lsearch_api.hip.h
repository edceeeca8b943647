// lsearch_api.hip.h -- the C entries of include/mipx_lsearch.h (included at the end of tree_engine.hip.h, which
// holds the launch and the per-step halves: ls_launch, and the local-search parts of heur_step_launch and
// heur_step_collect).
// The buffers behind the option's step block are a StepRing (tree_engine.hip.h): the set entry switches the option off,
// grows the ring, and switches it on last.  The batch entry's prologue is the shared one of mipx.hip (check_int_idx, ...).

extern "C" {

int mipx_pair_search_batch(mipx_problem *p, int batch, const double *x, const double *l, const double *u,
                           const int32_t *int_idx, int n_int, double tol, int max_moves, const uint8_t *skip,
                           double *x_out, double *obj_out, int32_t *status_out, int32_t *moves_out) {
    if (!p) return MIPX_EINVAL;
    mipx_ctx *ctx = p->ctx;
    if (batch < 0 || n_int < 0 || n_int > p->n || !(tol >= 0.0) || max_moves < 0 || !l || !u || (n_int && !int_idx) ||
        (batch && (!x || !x_out || !obj_out || !status_out || !moves_out)))
        return fail(ctx, MIPX_EINVAL, "mipx_pair_search_batch: bad argument");
    if (int rc = check_int_idx(ctx, "mipx_pair_search_batch", int_idx, n_int, p->n)) return rc;
    if (p->m > mipx::kLsMax || p->n > mipx::kLsMax)
        return fail(ctx, MIPX_ETOOBIG, "mipx_pair_search_batch: more than 1024 rows or columns");
    if (batch == 0) return MIPX_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t B = (size_t)batch, nn = (size_t)p->n;
    Staging S(ctx, "mipx_pair_search_batch");
    // (an output that is the input on the host is the input on the device too: the kernel then works in place)
    const bool alias = x_out == x;
    const size_t o_x = S.in(x, B * nn * 8), o_l = S.in(l, nn * 8), o_u = S.in(u, nn * 8),
                 o_ii = S.in(n_int ? int_idx : nullptr, (size_t)(n_int ? n_int : 1) * 4), o_sk = S.in(skip, B),
                 o_xo = alias ? o_x : S.out(x_out, B * nn * 8), o_ob = S.out(obj_out, B * 8), o_st = S.out(status_out, B * 4),
                 o_mv = S.out(moves_out, B * 8);
    if (alias) S.down(x_out, o_x, B * nn * 8);
    int rc = S.alloc(p->scratch, p->scratch_bytes);
    if (rc == MIPX_OK) rc = S.upload();
    if (rc == MIPX_OK)
        rc = ls_launch(p, ctx->stream, batch, S.at<const double>(o_x), S.at<const double>(o_l), S.at<const double>(o_u),
                       S.at<const int32_t>(o_ii), n_int, tol, max_moves, skip ? S.at<const uint8_t>(o_sk) : nullptr, nullptr,
                       S.at<double>(o_xo), S.at<double>(o_ob), S.at<int32_t>(o_st), S.at<int32_t>(o_mv));
    return S.finish(rc);
}

int mipx_tree_set_local_search(mipx_tree *t, int max_moves) {
    if (!t) return MIPX_EINVAL;
    mipx_ctx *ctx = t->ctx;
    if (max_moves < 0) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_local_search: max_moves is not negative");
    if (!t->hr.on)
        return fail(ctx, MIPX_EINVAL, "mipx_tree_set_local_search: the search runs on the heuristic's points (mipx_tree_set_heuristic first)");
    if (t->steps > 0 || t->evaluated > 0)
        return fail(ctx, MIPX_EINVAL, "mipx_tree_set_local_search: the search is set before the first step");
    LsState &ls = t->ls;
    if (max_moves == 0) {   // (the buffers stay)
        ls.on = false;
        return MIPX_OK;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (t->hr.cap > ls.cap) {   // (the heuristic's step buffers grew or are new: nothing is in flight before the first step)
        ls.on = false;   // (until every block is there: a failure below leaves the option off and nothing to launch on)
        ls.cap = 0;
        const int rc = ls.ring.grow(ctx, step_layout::LsOut((size_t)t->hr.cap).bytes(), 0);
        if (rc) return rc;
        ls.cap = t->hr.cap;   // (laid out for ls.cap points: step_layout::LsOut)
    }
    ls.max_moves = max_moves;
    ls.on = true;
    return MIPX_OK;
}

int mipx_tree_local_search_stats(mipx_tree *t, int64_t out[8]) {
    if (!t || !out) return MIPX_EINVAL;
    const LsState &ls = t->ls;
    out[0] = ls.run; out[1] = ls.improved; out[2] = ls.singles; out[3] = ls.pairs; out[4] = ls.capped;
    out[5] = ls.installed; out[6] = 0; out[7] = (int64_t)ls.us;
    return MIPX_OK;
}

}  // extern "C"
