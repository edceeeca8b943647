// rcfix_api.hip.h -- the C entries of include/mipx_rcfix.h (included at the end of tree_engine.hip.h, which holds
// the launch and the per-step parts: rc_launch, rc_step_stage, rc_level_launch, rc_step_collect).
// The prologue is the shared one of mipx.hip (check_int_idx, check_bounds).

extern "C" {

int mipx_reduced_cost_tighten_batch(mipx_problem *p, int batch, const double *l, const double *u, const double *y,
                                    const int32_t *int_idx, int n_int, double cutoff, double tol, double dtol,
                                    double *l_out, double *u_out, double *z_out, int32_t *status_out,
                                    int32_t *changed_out) {
    if (!p) return MIPX_EINVAL;
    mipx_ctx *ctx = p->ctx;
    if (batch < 0 || n_int < 0 || n_int > p->n || !(tol >= 0.0) || !(dtol >= 0.0) || cutoff != cutoff || (n_int && !int_idx) ||
        (batch && (!l || !u || (p->m > 0 && !y) || !l_out || !u_out || !z_out || !status_out || !changed_out)))
        return fail(ctx, MIPX_EINVAL, "mipx_reduced_cost_tighten_batch: bad argument");
    if (int rc = check_int_idx(ctx, "mipx_reduced_cost_tighten_batch", int_idx, n_int, p->n)) return rc;
    if (p->m > mipx::kRcMax || p->n > mipx::kRcMax)
        return fail(ctx, MIPX_ETOOBIG, "mipx_reduced_cost_tighten_batch: more than 1024 rows or columns");
    const size_t B = (size_t)batch, nn = (size_t)p->n, mm = (size_t)p->m;
    if (int rc = check_bounds(ctx, "mipx_reduced_cost_tighten_batch", nullptr, l, u, B * nn)) return rc;
    if (batch == 0) return MIPX_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Staging S(ctx, "mipx_reduced_cost_tighten_batch");
    // (outputs that are the inputs on the host are the inputs on the device too: the kernel then works in place)
    const bool alias = l_out == l && u_out == u;
    const size_t o_l = S.in(l, B * nn * 8), o_u = S.in(u, B * nn * 8), o_y = S.in(mm ? y : nullptr, B * (mm ? mm : 1) * 8),
                 o_ii = S.in(n_int ? int_idx : nullptr, (size_t)(n_int ? n_int : 1) * 4),
                 o_lo = alias ? o_l : S.out(l_out, B * nn * 8), o_uo = alias ? o_u : S.out(u_out, B * nn * 8),
                 o_z = S.out(z_out, B * 8), o_st = S.out(status_out, B * 4), o_ch = S.out(changed_out, B * 4);
    if (alias) { S.down(l_out, o_l, B * nn * 8); S.down(u_out, o_u, B * nn * 8); }
    int rc = S.alloc(p->scratch, p->scratch_bytes);
    if (rc == MIPX_OK) rc = S.upload();
    if (rc == MIPX_OK)
        rc = rc_launch(p, ctx->stream, batch, nullptr, nullptr, S.at<const double>(o_l), S.at<const double>(o_u),
                       S.at<const double>(o_y), S.at<const int32_t>(o_ii), n_int, cutoff, tol, dtol, S.at<double>(o_lo),
                       S.at<double>(o_uo), S.at<double>(o_z), S.at<int32_t>(o_st), S.at<int32_t>(o_ch));
    return S.finish(rc);
}

int mipx_tree_set_reduced_cost(mipx_tree *t, int on) {
    if (!t) return MIPX_EINVAL;
    mipx_ctx *ctx = t->ctx;
    if (t->cuts) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_reduced_cost: not with cut rounds");
    if (t->comm) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_reduced_cost: not with a communicator");
    if (t->df.on) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_reduced_cost: not with the dual function (mipx_tree_set_dual_record)");
    if (t->tr.on) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_reduced_cost: not with the tree record (mipx_tree_set_tree_record)");
    if (t->steps > 0 || t->evaluated > 0)
        return fail(ctx, MIPX_EINVAL, "mipx_tree_set_reduced_cost: the tightening is set before the first step");
    if (t->m > mipx::kRcMax || t->n > mipx::kRcMax)
        return fail(ctx, MIPX_ETOOBIG, "mipx_tree_set_reduced_cost: more than 1024 rows or columns");
    RcState &rs = t->rc;
    if (!on) {   // (the buffers stay; the finish mode stays as it is, as with the other options)
        rs.on = false;
        return MIPX_OK;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (rs.cap == 0) {
        rs.cap = t->max_batch;   // (the step buffers are laid out for rs.cap nodes per level: step_layout::RcOut)
        const size_t io_bytes = rc_layout(t).bytes(), y_count = (size_t)kRcLevels * (size_t)t->max_batch * (size_t)t->m;
        for (int k = 0; k < 3; k++) {
            int rc = dmalloc(ctx, &rs.d_y[k], y_count);
            if (!rc) rc = dmalloc(ctx, &rs.d_io[k], io_bytes / 4);
            if (rc) return rc;
            HIP_TRY(ctx, hipMemset(rs.d_y[k], 0, (y_count ? y_count : 1) * 8));
            HIP_TRY(ctx, hipHostMalloc((void **)&rs.h_io[k], io_bytes));
            for (int q = 0; q < kRcLevels; q++) {
                HIP_TRY(ctx, hipEventCreate(&rs.e0[k][q]));
                HIP_TRY(ctx, hipEventCreate(&rs.e1[k][q]));
            }
        }
    }
    rs.on = true;
    // the tightening runs where the host writes the children of a step: every step is finished on the host, the
    // switch mipx_tree_set_propagation uses
    t->fast_ok = false;
    return MIPX_OK;
}

int mipx_tree_reduced_cost_stats(mipx_tree *t, int64_t out[8]) {
    if (!t || !out) return MIPX_EINVAL;
    for (StepBuf &S : t->buf) {   // (a pipelined solve leaves its last launches uncollected)
        const int rc = rc_step_collect(t, S);
        if (rc) return rc;
    }
    const RcState &rs = t->rc;
    out[0] = rs.nodes; out[1] = rs.tightened; out[2] = rs.cut_off; out[3] = rs.no_bound; out[4] = rs.changed;
    out[5] = rs.launches; out[6] = 0; out[7] = (int64_t)rs.us;
    return MIPX_OK;
}

}  // extern "C"
