// heur_api.hip.h -- the C entries of include/mipx_heur.h (included at the end of tree_engine.hip.h, which holds
// the launch and the per-step halves: heur_launch, heur_step_launch, heur_step_collect).
// The buffers behind the option's step block are a StepRing (tree_engine.hip.h): the set entry switches the option off,
// grows the ring, and switches it on last.  The batch entry's prologue is the shared one of mipx.hip (check_int_idx, ...).

extern "C" {

int mipx_round_repair_batch(mipx_problem *p, int batch, const double *x, const double *l, const double *u,
                            const int32_t *int_idx, int n_int, double tol, int max_moves, const uint8_t *skip,
                            double *x_out, double *obj_out, int32_t *status_out, int32_t *moves_out) {
    if (!p) return MIPX_EINVAL;
    mipx_ctx *ctx = p->ctx;
    if (batch < 0 || n_int < 0 || n_int > p->n || !(tol >= 0.0) || max_moves < 0 || !l || !u || (n_int && !int_idx) ||
        (batch && (!x || !x_out || !obj_out || !status_out || !moves_out)))
        return fail(ctx, MIPX_EINVAL, "mipx_round_repair_batch: bad argument");
    if (int rc = check_int_idx(ctx, "mipx_round_repair_batch", int_idx, n_int, p->n)) return rc;
    if (p->m > mipx::kHeurMax || p->n > mipx::kHeurMax)
        return fail(ctx, MIPX_ETOOBIG, "mipx_round_repair_batch: more than 1024 rows or columns");
    if (batch == 0) return MIPX_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t B = (size_t)batch, nn = (size_t)p->n;
    Staging S(ctx, "mipx_round_repair_batch");
    const size_t o_x = S.in(x, B * nn * 8), o_l = S.in(l, nn * 8), o_u = S.in(u, nn * 8),
                 o_ii = S.in(n_int ? int_idx : nullptr, (size_t)(n_int ? n_int : 1) * 4), o_sk = S.in(skip, B),
                 o_xo = S.out(x_out, B * nn * 8), o_ob = S.out(obj_out, B * 8), o_st = S.out(status_out, B * 4),
                 o_mv = S.out(moves_out, B * 8);
    int rc = S.alloc(p->scratch, p->scratch_bytes);
    if (rc == MIPX_OK) rc = S.upload();
    if (rc == MIPX_OK)
        rc = heur_launch(p, ctx->stream, batch, S.at<const double>(o_x), S.at<const double>(o_l), S.at<const double>(o_u),
                         S.at<const int32_t>(o_ii), n_int, tol, max_moves, skip ? S.at<const uint8_t>(o_sk) : nullptr, nullptr,
                         S.at<double>(o_xo), S.at<double>(o_ob), S.at<int32_t>(o_st), S.at<int32_t>(o_mv));
    return S.finish(rc);
}

int mipx_tree_set_heuristic(mipx_tree *t, int points_per_step, int every_steps, int max_moves) {
    if (!t) return MIPX_EINVAL;
    mipx_ctx *ctx = t->ctx;
    if (points_per_step < 1 || every_steps < 1 || max_moves < 1)
        return fail(ctx, MIPX_EINVAL, "mipx_tree_set_heuristic: points_per_step, every_steps and max_moves are positive");
    if (t->cuts) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_heuristic: not with cut rounds");
    if (t->comm) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_heuristic: not with a communicator");
    if (t->steps > 0 || t->evaluated > 0)
        return fail(ctx, MIPX_EINVAL, "mipx_tree_set_heuristic: the heuristic is set before the first step");
    if (t->m > mipx::kHeurMax || t->n > mipx::kHeurMax)
        return fail(ctx, MIPX_ETOOBIG, "mipx_tree_set_heuristic: more than 1024 rows or columns");
    HeurState &hr = t->hr;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int P = std::min(points_per_step, t->max_batch);
    const size_t n = (size_t)t->n;
    if (!hr.d_lu) {
        int rc = dmalloc(ctx, &hr.d_lu, 2 * n);
        if (rc) return rc;
        HIP_TRY(ctx, hipMemcpy(hr.d_lu, t->root_l.data(), n * 8, hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(hr.d_lu + n, t->root_u.data(), n * 8, hipMemcpyHostToDevice));
    }
    if (t->ls.on && P > t->ls.cap)
        return fail(ctx, MIPX_EINVAL, "mipx_tree_set_heuristic: more points than the local search was set for (mipx_tree_set_local_search(t, 0) first)");
    if (t->fp.on && P > t->fp.cap)
        return fail(ctx, MIPX_EINVAL, "mipx_tree_set_heuristic: more points than the fix-and-propagate dive was set for (mipx_tree_set_fix_propagate(t, 1, 0) first)");
    if (t->wr.on && P > t->wr.cap)
        return fail(ctx, MIPX_EINVAL, "mipx_tree_set_heuristic: more points than the weighted row repair was set for (mipx_tree_set_weighted_repair(t, 0) first)");
    if (t->cu.on && P > t->cu.cap)
        return fail(ctx, MIPX_EINVAL, "mipx_tree_set_heuristic: more points than the cube search was set for (mipx_tree_set_cube_search(t, 0) first)");
    if (t->cc.on && P > t->cc.cap)
        return fail(ctx, MIPX_EINVAL, "mipx_tree_set_heuristic: more points than the completion was set for (mipx_tree_set_completion(t, 0) first)");
    if (t->ld.on && P > t->ld.cap)
        return fail(ctx, MIPX_EINVAL, "mipx_tree_set_heuristic: more points than the LP dive was set for (mipx_tree_set_lpdive(t, 0, 0, 0) first)");
    if (P > hr.cap) {   // (set again with more points: the step buffers grow; nothing is in flight before the first step)
        hr.on = false;   // (until every block is there: a failure below leaves the option off and nothing to launch on)
        hr.cap = 0;
        const int rc = hr.ring.grow(ctx, step_layout::HeurOut((size_t)P).bytes(), (size_t)P * n);
        if (rc) return rc;
        hr.cap = P;   // (the step buffers are laid out for hr.cap points: step_layout::HeurOut)
    }
    hr.points = P;
    hr.every = every_steps;
    hr.max_moves = max_moves;
    hr.on = true;
    // the incumbent is installed by the host before it evaluates the step's nodes: every step is finished on the
    // host, the switch mipx_tree_set_dual_record and mipx_tree_set_tree_record use
    t->fast_ok = false;
    return MIPX_OK;
}

int mipx_tree_heuristic_stats(mipx_tree *t, int64_t out[8]) {
    if (!t || !out) return MIPX_EINVAL;
    const HeurState &hr = t->hr;
    out[0] = hr.tried; out[1] = hr.feasible; out[2] = hr.stuck; out[3] = hr.capped; out[4] = hr.repair; out[5] = hr.lift;
    out[6] = hr.installed; out[7] = (int64_t)hr.us;
    return MIPX_OK;
}

}  // extern "C"
