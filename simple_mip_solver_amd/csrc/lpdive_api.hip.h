// lpdive_api.hip.h -- the C entries of include/mipx_lpdive.h (included at the end of tree_engine.hip.h, which holds the
// launch and the per-step halves: lpdive_launch, and the option's parts of heur_step_launch and heur_step_collect).
// The buffers behind the option's step block are a StepRing (tree_engine.hip.h): the set entry switches the option off,
// grows the ring, and switches it on last.  The batch entry's prologue is the shared one of mipx.hip (check_int_idx, ...).

extern "C" {

int mipx_lpdive_batch(mipx_problem *p, int batch, const double *x, const double *l, const double *u,
                      const int32_t *int_idx, int n_int, const int8_t *vstat, const uint8_t *skip,
                      double cutoff, int max_rounds, int rule,
                      double *x_out, double *obj_out, int32_t *status_out,
                      int32_t *rounds_out, int32_t *fixings_out, int32_t *flips_out, int32_t *pivots_out) {
    if (!p) return MIPX_EINVAL;
    mipx_ctx *ctx = p->ctx;
    if (batch < 0 || n_int < 0 || n_int > p->n || (n_int && !int_idx) ||
        (batch && (!x || !l || !u || !x_out || !obj_out || !status_out || !rounds_out || !fixings_out || !flips_out || !pivots_out)))
        return fail(ctx, MIPX_EINVAL, "mipx_lpdive_batch: bad argument");
    if (max_rounds < 1 || max_rounds > MIPX_LPDIVE_MAX_ROUNDS)
        return fail(ctx, MIPX_EINVAL, "mipx_lpdive_batch: max_rounds outside 1..1024");
    if (rule != MIPX_LPDIVE_RULE_FRACTIONAL && rule != MIPX_LPDIVE_RULE_COEFFICIENT)
        return fail(ctx, MIPX_EINVAL, "mipx_lpdive_batch: the rule is 0 (fractional) or 1 (coefficient)");
    if (cutoff != cutoff) return fail(ctx, MIPX_EINVAL, "mipx_lpdive_batch: the cutoff is NaN");
    if (int rc = check_int_idx(ctx, "mipx_lpdive_batch", int_idx, n_int, p->n)) return rc;
    if (p->m > mipx::kLpdiveMax || p->n > mipx::kLpdiveMax)
        return fail(ctx, MIPX_ETOOBIG, "mipx_lpdive_batch: more than 1024 rows or columns");
    const size_t B = (size_t)batch, nn = (size_t)p->n, nv = nn + (size_t)p->m;
    if (int rc = check_bounds(ctx, "mipx_lpdive_batch", nullptr, l, u, B * nn)) return rc;
    if (batch == 0) return MIPX_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Staging S(ctx, "mipx_lpdive_batch");
    const size_t ni = (size_t)(n_int ? n_int : 1);
    const size_t o_x = S.in(x, B * nn * 8), o_l = S.in(l, B * nn * 8), o_u = S.in(u, B * nn * 8),
                 o_ii = S.in(n_int ? int_idx : nullptr, ni * 4), o_sk = S.in(skip, B), o_vs = S.in(vstat, B * nv),
                 o_lk = S.carve(2 * ni * 4), o_ws = S.carve(mipx::LpdiveWs(B, (size_t)p->m, nn).bytes()),
                 o_xo = S.out(x_out, B * nn * 8), o_ob = S.out(obj_out, B * 8), o_st = S.out(status_out, B * 4),
                 o_rd = S.out(rounds_out, B * 4), o_fx = S.out(fixings_out, B * 4), o_fl = S.out(flips_out, B * 4),
                 o_pv = S.out(pivots_out, B * 4);
    int rc = S.alloc(p->scratch, p->scratch_bytes);
    if (rc == MIPX_OK) rc = S.upload();
    if (rc == MIPX_OK && n_int > 0) {
        hipLaunchKernelGGL(mipx::lpdive_locks, dim3((unsigned)((n_int + 255) / 256)), dim3(256), 0, ctx->stream, p->m, p->n, n_int,
                           (const double *)p->dA, S.at<const int32_t>(o_ii), S.at<int32_t>(o_lk));
        if (hipGetLastError() != hipSuccess) rc = fail(ctx, MIPX_EHIP, "mipx_lpdive_batch: lpdive_locks");
    }
    if (rc == MIPX_OK)
        rc = lpdive_launch(p, ctx->stream, batch, S.at<const double>(o_x), S.at<const double>(o_l), S.at<const double>(o_u), nullptr,
                           skip ? S.at<const uint8_t>(o_sk) : nullptr, nullptr, vstat ? S.at<const int8_t>(o_vs) : nullptr,
                           S.at<const int32_t>(o_ii), n_int, S.at<const int32_t>(o_lk), cutoff, max_rounds, rule, true,
                           S.at<char>(o_ws), S.at<double>(o_xo), S.at<double>(o_ob), S.at<int32_t>(o_st), S.at<int32_t>(o_rd),
                           S.at<int32_t>(o_fx), S.at<int32_t>(o_fl), S.at<int32_t>(o_pv));
    return S.finish(rc);
}

int mipx_tree_set_lpdive(mipx_tree *t, int max_rounds, int every, int rule) {
    if (!t) return MIPX_EINVAL;
    mipx_ctx *ctx = t->ctx;
    if (max_rounds < 0 || max_rounds > MIPX_LPDIVE_MAX_ROUNDS)
        return fail(ctx, MIPX_EINVAL, "mipx_tree_set_lpdive: max_rounds outside 0..1024");
    if (every < 0) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_lpdive: every is not negative");
    if (rule != MIPX_LPDIVE_RULE_FRACTIONAL && rule != MIPX_LPDIVE_RULE_COEFFICIENT)
        return fail(ctx, MIPX_EINVAL, "mipx_tree_set_lpdive: the rule is 0 (fractional) or 1 (coefficient)");
    if (!t->hr.on)
        return fail(ctx, MIPX_EINVAL, "mipx_tree_set_lpdive: the dive runs on the heuristic's points (mipx_tree_set_heuristic first)");
    if (t->cuts) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_lpdive: not with cut rounds");
    if (t->comm) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_lpdive: not with a communicator");
    if (t->steps > 0 || t->evaluated > 0)
        return fail(ctx, MIPX_EINVAL, "mipx_tree_set_lpdive: the dive is set before the first step");
    LpdiveState &ld = t->ld;
    if (max_rounds == 0) {   // (the buffers stay)
        ld.on = false;
        return MIPX_OK;
    }
    if (t->prob->m > mipx::kLpdiveMax || t->prob->n > mipx::kLpdiveMax)
        return fail(ctx, MIPX_ETOOBIG, "mipx_tree_set_lpdive: more than 1024 rows or columns");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!ld.d_locks) {   // (rule 1's lock counts: once per problem)
        int rc = dmalloc(ctx, &ld.d_locks, 2 * (size_t)(t->n_int ? t->n_int : 1));
        if (rc) return rc;
        if (t->n_int > 0) {
            hipLaunchKernelGGL(mipx::lpdive_locks, dim3((unsigned)((t->n_int + 255) / 256)), dim3(256), 0, ctx->stream, t->prob->m,
                               t->n, t->n_int, (const double *)t->prob->dA, (const int32_t *)t->d_int_idx, ld.d_locks);
            HIP_TRY(ctx, hipGetLastError());
        }
    }
    if (t->hr.cap > ld.cap) {   // (the heuristic's step buffers grew or are new: nothing is in flight before the first step)
        const size_t cap = (size_t)t->hr.cap, out_bytes = mipx::LpdiveOut(cap).bytes();
        ld.on = false;   // (until every block is there: a failure below leaves the option off and nothing to launch on)
        ld.cap = 0;
        if (ld.d_ws) (void)hipFree(ld.d_ws);
        ld.d_ws = nullptr;
        int rc = dmalloc(ctx, &ld.d_ws, mipx::LpdiveWs(cap, (size_t)t->prob->m, (size_t)t->n).bytes());
        if (rc) return rc;
        if ((rc = ld.ring.grow(ctx, out_bytes, cap * (size_t)t->n))) return rc;
        ld.cap = t->hr.cap;
    }
    ld.max_rounds = max_rounds; ld.every = every; ld.rule = rule;
    ld.on = true;
    return MIPX_OK;
}

int mipx_tree_lpdive_stats(mipx_tree *t, int64_t out[8]) {
    if (!t || !out) return MIPX_EINVAL;
    const LpdiveState &ld = t->ld;
    out[0] = ld.tried; out[1] = ld.feasible; out[2] = ld.infeasible; out[3] = ld.failed; out[4] = ld.moves;
    out[5] = ld.installed; out[6] = ld.pivots; out[7] = (int64_t)ld.us;
    return MIPX_OK;
}

}  // extern "C"
