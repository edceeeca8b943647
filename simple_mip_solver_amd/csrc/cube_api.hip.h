// cube_api.hip.h -- the C entries of include/mipx_cube.h (included at the end of tree_engine.hip.h, which holds the
// launch and the per-step halves: cube_launch, and the option's parts of heur_step_launch and heur_step_collect).
// The buffers behind the option's step block are a StepRing (tree_engine.hip.h): the set entry switches the option off,
// grows the ring, and switches it on last.  The batch entry's prologue is the shared one of mipx.hip (check_int_idx, ...).

extern "C" {

int mipx_cube_search_batch(mipx_problem *p, int batch, const double *x, const double *l, const double *u,
                           const int32_t *int_idx, int n_int, double cutoff, double tol, double ftol, int max_columns,
                           const uint8_t *skip, double *x_out, double *obj_out, int32_t *status_out,
                           int32_t *counts_out) {
    if (!p) return MIPX_EINVAL;
    mipx_ctx *ctx = p->ctx;
    if (batch < 0 || n_int < 0 || n_int > p->n || !(tol >= 0.0) || !(ftol >= 0.0) || cutoff != cutoff || max_columns < 1 ||
        max_columns > MIPX_CUBE_MAX_COLUMNS || !l || !u || (n_int && !int_idx) ||
        (batch && (!x || !x_out || !obj_out || !status_out || !counts_out)))
        return fail(ctx, MIPX_EINVAL, "mipx_cube_search_batch: bad argument");
    if (int rc = check_int_idx(ctx, "mipx_cube_search_batch", int_idx, n_int, p->n)) return rc;
    if (p->m > mipx::kCubeMax || p->n > mipx::kCubeMax)
        return fail(ctx, MIPX_ETOOBIG, "mipx_cube_search_batch: more than 1024 rows or columns");
    const size_t B = (size_t)batch, nn = (size_t)p->n;
    if (int rc = check_bounds(ctx, "mipx_cube_search_batch", nullptr, l, u, nn)) return rc;
    if (int rc = check_points(ctx, "mipx_cube_search_batch", x, B * nn)) return rc;
    if (batch == 0) return MIPX_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Staging S(ctx, "mipx_cube_search_batch");
    const size_t o_x = S.in(x, B * nn * 8), o_l = S.in(l, nn * 8), o_u = S.in(u, nn * 8),
                 o_ii = S.in(n_int ? int_idx : nullptr, (size_t)(n_int ? n_int : 1) * 4), o_sk = S.in(skip, B),
                 o_ws = S.carve(mipx::CubeWs(B, (size_t)p->m, max_columns).bytes()), o_xo = S.out(x_out, B * nn * 8),
                 o_ob = S.out(obj_out, B * 8), o_st = S.out(status_out, B * 4), o_ct = S.out(counts_out, B * 8);
    int rc = S.alloc(p->scratch, p->scratch_bytes);
    if (rc == MIPX_OK) rc = S.upload();
    if (rc == MIPX_OK)
        rc = cube_launch(p, ctx->stream, batch, S.at<const double>(o_x), S.at<const double>(o_l), S.at<const double>(o_u),
                         S.at<const int32_t>(o_ii), n_int, cutoff, tol, ftol, max_columns,
                         skip ? S.at<const uint8_t>(o_sk) : nullptr, nullptr, S.at<char>(o_ws), S.at<double>(o_xo),
                         S.at<double>(o_ob), S.at<int32_t>(o_st), S.at<int32_t>(o_ct));
    return S.finish(rc);
}

int mipx_tree_set_cube_search(mipx_tree *t, int max_columns) {
    if (!t) return MIPX_EINVAL;
    mipx_ctx *ctx = t->ctx;
    if (max_columns < 0 || max_columns > MIPX_CUBE_MAX_COLUMNS)
        return fail(ctx, MIPX_EINVAL, "mipx_tree_set_cube_search: max_columns is 0 (off) or 1..20");
    if (!t->hr.on)
        return fail(ctx, MIPX_EINVAL, "mipx_tree_set_cube_search: the cube search runs on the heuristic's points (mipx_tree_set_heuristic first)");
    if (t->cuts) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_cube_search: not with cut rounds");
    if (t->comm) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_cube_search: not with a communicator");
    if (t->steps > 0 || t->evaluated > 0)
        return fail(ctx, MIPX_EINVAL, "mipx_tree_set_cube_search: the cube search is set before the first step");
    CubeState &cu = t->cu;
    if (max_columns == 0) {   // (the buffers stay)
        cu.on = false;
        return MIPX_OK;
    }
    if (t->prob->m > mipx::kCubeMax || t->prob->n > mipx::kCubeMax)
        return fail(ctx, MIPX_ETOOBIG, "mipx_tree_set_cube_search: more than 1024 rows or columns");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (t->hr.cap > cu.cap) {   // (the heuristic's step buffers grew or are new: nothing is in flight before the first step)
        cu.on = false;   // (until every block is there: a failure below leaves the option off and nothing to launch on)
        cu.cap = 0;
        const int rc = cu.ring.grow(ctx, step_layout::CubeOut((size_t)t->hr.cap).bytes(), (size_t)t->hr.cap * (size_t)t->n);
        if (rc) return rc;
        cu.cap = t->hr.cap;   // (laid out for cu.cap points: step_layout::CubeOut)
        cu.ws_columns = 0;    // (and the workspace with them)
    }
    if (max_columns > cu.ws_columns) {   // (the workspace grows with the points and with K: mipx::CubeWs)
        if (cu.d_ws) (void)hipFree(cu.d_ws);
        cu.d_ws = nullptr;
        cu.ws_columns = 0;
        cu.on = false;   // (as above)
        const int rc = dmalloc(ctx, &cu.d_ws, mipx::CubeWs((size_t)cu.cap, (size_t)t->prob->m, max_columns).bytes());
        if (rc) return rc;
        cu.ws_columns = max_columns;
    }
    cu.max_columns = max_columns;
    cu.on = true;
    return MIPX_OK;
}

int mipx_tree_cube_search_stats(mipx_tree *t, int64_t out[8]) {
    if (!t || !out) return MIPX_EINVAL;
    const CubeState &cu = t->cu;
    out[0] = cu.tried; out[1] = cu.found; out[2] = cu.none; out[3] = cu.columns; out[4] = cu.at_cap;
    out[5] = cu.installed; out[6] = 0; out[7] = (int64_t)cu.us;
    return MIPX_OK;
}

}  // extern "C"
