// dualfn_api.hip.h -- the C entries of include/mipx_dualfn.h (included at the end of tree_engine.hip.h).

extern "C" {

int mipx_tree_set_dual_record(mipx_tree *t, int64_t max_bytes, int rows, const int32_t *pos, const double *sign) {
    if (!t) return MIPX_EINVAL;
    mipx_ctx *ctx = t->ctx;
    if (max_bytes == -1) {   // half of the device memory free now
        size_t free_b = 0, total_b = 0;
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HIP_TRY(ctx, hipMemGetInfo(&free_b, &total_b));
        max_bytes = (int64_t)(free_b / 2);
    }
    if (max_bytes <= 0) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_dual_record: the byte cap must be positive (or -1)");
    if (t->rs.on) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_dual_record: not on a restarted tree (mipx_tree_create_restart)");
    if (t->steps > 0 || t->nodes.size() != 1 || t->evaluated > 0)
        return fail(ctx, MIPX_EINVAL, "mipx_tree_set_dual_record: recording must be turned on before the first step");
    if (t->comm) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_dual_record: not with a communicator");
    if (t->cuts) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_dual_record: not with cut rounds");
    if (t->pg.on) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_dual_record: not with the bound propagation (mipx_tree_set_propagation)");
    if (t->rc.on) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_dual_record: not with the reduced-cost tightening (mipx_tree_set_reduced_cost)");
    if (t->os.on) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_dual_record: not with the objective step (mipx_tree_set_objective_step)");
    if (rows < 0 || (t->m > 0 && (!pos || !sign)))
        return fail(ctx, MIPX_EINVAL, "mipx_tree_set_dual_record: bad row map");
    for (int e = 0; e < t->m; e++)
        if (pos[e] < 0 || pos[e] >= rows || (sign[e] != 1.0 && sign[e] != -1.0))
            return fail(ctx, MIPX_EINVAL, "mipx_tree_set_dual_record: bad row map");
    DualFn &df = t->df;
    df.on = true;
    // Every step is finished on the host, which knows each child's parent, with the host's pseudo-cost table
    // (the mode of MIPX_HOST_FINISH=1): steps finished on the host while the device holds the table would
    // update a version that launches already in flight read.
    t->fast_ok = false;
    df.cap = max_bytes;
    df.rows = rows;
    df.pos.assign(pos, pos + t->m);
    df.sign.assign(sign, sign + t->m);
    df.parent.assign(1, -1);
    df.rec.assign(1, -1);
    df.haschild.assign(1, 0);
    df.dirty = true;
    return MIPX_OK;
}

int mipx_tree_dual_function(mipx_tree *t, int K, const double *w, double M, double *out) {
    if (!t) return MIPX_EINVAL;
    mipx_ctx *ctx = t->ctx;
    if (!t->df.on) return fail(ctx, MIPX_EINVAL, "mipx_tree_dual_function: recording is off (mipx_tree_set_dual_record)");
    if (K < 0 || (K > 0 && (!w || !out))) return fail(ctx, MIPX_EINVAL, "mipx_tree_dual_function: bad argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(ctx, hipStreamSynchronize(t->st3));
    HIP_TRY(ctx, hipStreamSynchronize(t->st2));
    HIP_TRY(ctx, hipStreamSynchronize(t->stf));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (StepBuf &S : t->buf) df_take_time(t, S);
    int rc = df_penalised(t, M);
    if (!rc) rc = df_lineage(t);
    if (!rc && K > 0) rc = df_evaluate(t, K, w, out);
    t->df.eval_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

int mipx_tree_dual_function_stats(mipx_tree *t, int64_t out[8]) {
    if (!t || !out) return MIPX_EINVAL;
    const DualFn &df = t->df;
    for (const StepBuf &S : t->buf)
        if (S.df_timed && hipEventQuery(S.df_e1) == hipSuccess) df_take_time(t, const_cast<StepBuf &>(S));
    out[0] = (int64_t)df.rec_node.size(); out[1] = df.bytes; out[2] = df.dropped; out[3] = (int64_t)df.inf_node.size();
    out[4] = df.resolves; out[5] = df.noterm; out[6] = (int64_t)df.record_us; out[7] = (int64_t)df.eval_us;
    return MIPX_OK;
}

int64_t mipx_tree_dual_records(mipx_tree *t, int64_t max_records, int64_t *node, int64_t *parent, int32_t *status,
                               double *tval, double *y) {
    if (!t) return MIPX_EINVAL;
    mipx_ctx *ctx = t->ctx;
    const DualFn &df = t->df;
    if (!df.on) return fail(ctx, MIPX_EINVAL, "mipx_tree_dual_records: recording is off");
    const int64_t R = std::min<int64_t>(max_records < 0 ? 0 : max_records, (int64_t)df.rec_node.size());
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(t->st3));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int64_t r = 0; r < R; r++) {
        const int64_t id = df.rec_node[(size_t)r];
        if (node) node[r] = id;
        if (parent) parent[r] = df.parent[(size_t)id];
        if (status) status[r] = df.rec_status[(size_t)r];
    }
    if (R > 0 && tval) HIP_TRY(ctx, hipMemcpy(tval, df.d_t, (size_t)R * 8, hipMemcpyDeviceToHost));
    if (R > 0 && y) HIP_TRY(ctx, hipMemcpy(y, df.d_y, (size_t)R * t->m * 8, hipMemcpyDeviceToHost));
    return R;
}

}  // extern "C"
