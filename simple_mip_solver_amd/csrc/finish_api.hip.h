// finish_api.hip.h -- the C entries of include/mipx_finish.h (included at the end of tree_engine.hip.h, which holds
// enqueue_finish): the device finish on a caller's step.  Test scaffolding: no product code calls them.

extern "C" {

int mipx_finish_step_batch(mipx_ctx *ctx, int n, int m, int B, int dive, int rule, int ask_count, int ask_cap,
                           const int32_t *out_i, const double *out_d, const int8_t *vout, const int32_t *slot,
                           const int32_t *par_i, const double *par_d, const int32_t *budget, int pool_rows,
                           double *pool_l, double *pool_u, int8_t *pool_v, double *primal, double *cost_l,
                           double *cost_r, uint8_t *has, int32_t *times, double *own, void *summary, void *open,
                           int32_t *dead, void *samples, int32_t *sample_keys) {
    if (!ctx) return MIPX_EINVAL;
    const char *who = "mipx_finish_step_batch";
    if (B < 1 || dive < 0 || dive > 8 || n < 1 || n > 1024 || m < 0 || rule < 0 || rule > 1 || pool_rows < 1)
        return fail(ctx, MIPX_EINVAL, "mipx_finish_step_batch: B < 1, dive outside 0..8, n outside 1..1024, m < 0, rule outside 0..1 or pool_rows < 1");
    if (!out_i || !out_d || !vout || !slot || !par_i || !par_d || !budget || !pool_l || !pool_u || !pool_v || !primal ||
        !summary || !open || !dead)
        return fail(ctx, MIPX_EINVAL, "mipx_finish_step_batch: a null argument");
    if (rule == 1 && (!cost_l || !cost_r || !has || !times || !own || !samples || !sample_keys))
        return fail(ctx, MIPX_EINVAL, "mipx_finish_step_batch: rule 1 needs the table, samples and sample_keys");
    const size_t Bz = (size_t)B, nn = (size_t)n, nv = (size_t)n + (size_t)m, per = 2 * (1 + (size_t)dive), P = (1 + (size_t)dive) * Bz,
                 rows = (size_t)pool_rows;
    // (the kernels index the pool by these rows and by nothing else a caller sends)
    for (size_t k = 0; k < Bz; k++)
        if (slot[k] < 0 || slot[k] >= pool_rows) return fail(ctx, MIPX_EINVAL, "mipx_finish_step_batch: a slot outside the pool");
    for (size_t e = 0; e < Bz * per; e++)
        if (budget[e] < 0 || budget[e] >= pool_rows) return fail(ctx, MIPX_EINVAL, "mipx_finish_step_batch: a budget row outside the pool");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Staging S(ctx, who);
    auto inout = [&S](void *p, size_t bytes) { const size_t o = S.in(p, bytes); S.down(p, o, bytes); return o; };
    const int32_t ask[4] = {ask_count, 0, 0, 0};
    const size_t o_oi = S.in(out_i, 7 * P * 4), o_od = S.in(out_d, 3 * P * 8), o_vo = S.in(vout, P * nv), o_sl = S.in(slot, Bz * 4),
                 o_pi = S.in(par_i, 4 * Bz * 4), o_pd = S.in(par_d, 2 * Bz * 8), o_bu = S.in(budget, Bz * per * 4),
                 o_ask = S.in(ask, sizeof ask);
    const size_t o_pl = inout(pool_l, rows * nn * 8), o_pu = inout(pool_u, rows * nn * 8), o_pv = inout(pool_v, rows * nv),
                 o_pr = inout(primal, 8);
    const bool tab = rule == 1;
    const size_t o_cl = inout(tab ? cost_l : nullptr, nn * 8), o_cr = inout(tab ? cost_r : nullptr, nn * 8),
                 o_ha = inout(tab ? has : nullptr, nn), o_ti = inout(tab ? times : nullptr, 2 * nn * 4),
                 o_ow = inout(tab ? own : nullptr, 4 * nn * 8);
    const size_t o_su = inout(summary, sizeof(mipx::FinishSummary)), o_op = inout(open, per * Bz * sizeof(mipx::OpenEntry)),
                 o_de = inout(dead, per * Bz * 4), o_sa = inout(tab ? samples : nullptr, P * sizeof(mipx::PcSample)),
                 o_sk = inout(tab ? sample_keys : nullptr, P * 4);
    // the per-chain scratch (FinishArgs)
    const size_t o_info = S.carve(Bz * 4), o_cnt = S.carve(3 * Bz * 4), o_eval = S.carve(2 * Bz * 4), o_val = S.carve(2 * Bz * 8),
                 o_flag = S.carve(Bz * 4), o_run = S.carve(Bz * 8);
    int rc = S.alloc();
    if (rc == MIPX_OK) rc = S.upload();
    if (rc == MIPX_OK) {
        mipx::FinishArgs g;
        g.n = n; g.m = m; g.B = B; g.dive = dive; g.rule = rule;
        const int32_t *oi = S.at<const int32_t>(o_oi);
        const double *od = S.at<const double>(o_od);
        g.status = oi; g.bidx = oi + P; g.mipf = oi + 2 * P; g.nprobe = oi + 3 * P; g.npiv = oi + 4 * P;
        g.dvar = oi + 5 * P; g.ddir = oi + 6 * P;
        g.obj = od; g.bval = od + P; g.dval = od + 2 * P;
        g.ask_count = S.at<const int32_t>(o_ask); g.ask_cap = ask_cap; g.vout = S.at<const int8_t>(o_vo);
        g.slot = S.at<const int32_t>(o_sl); g.par_i = S.at<const int32_t>(o_pi); g.par_d = S.at<const double>(o_pd);
        g.budget = S.at<const int32_t>(o_bu);
        g.pool_l = S.at<double>(o_pl); g.pool_u = S.at<double>(o_pu); g.pool_v = S.at<int8_t>(o_pv); g.primal = S.at<double>(o_pr);
        g.c_info = S.at<int32_t>(o_info); g.c_cnt = S.at<int32_t>(o_cnt); g.c_eval = S.at<int32_t>(o_eval);
        g.c_val = S.at<double>(o_val); g.c_flag = S.at<int32_t>(o_flag); g.c_run = S.at<double>(o_run);
        g.sum = S.at<mipx::FinishSummary>(o_su); g.open = S.at<mipx::OpenEntry>(o_op); g.dead = S.at<int32_t>(o_de);
        g.samples = S.at<mipx::PcSample>(o_sa); g.sample_keys = S.at<int32_t>(o_sk);
        mipx::PcApplyArgs a{};
        if (tab) {
            a.n = n; a.sum = g.sum; a.count = -1; a.samples = g.samples; a.keys = g.sample_keys;
            a.cost_l = S.at<double>(o_cl); a.cost_r = S.at<double>(o_cr); a.has = S.at<uint8_t>(o_ha);
            a.times = S.at<int32_t>(o_ti); a.own = S.at<double>(o_ow);
        }
        enqueue_finish(g, tab ? &a : nullptr, ctx->stream);
        if (hipError_t e = hipGetLastError()) rc = S.err("launch", e);
    }
    return S.finish(rc);
}

int mipx_pc_apply_batch(mipx_ctx *ctx, int n, int count, const void *samples, const int32_t *keys, double *cost_l,
                        double *cost_r, uint8_t *has, int32_t *times, double *own) {
    if (!ctx) return MIPX_EINVAL;
    if (n < 1 || n > 1024 || count < 0 || !cost_l || !cost_r || !has || !times || !own || (count > 0 && (!samples || !keys)))
        return fail(ctx, MIPX_EINVAL, "mipx_pc_apply_batch: bad argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)n, cnt = (size_t)(count ? count : 1);
    Staging S(ctx, "mipx_pc_apply_batch");
    auto inout = [&S](void *p, size_t bytes) { const size_t o = S.in(p, bytes); S.down(p, o, bytes); return o; };
    const size_t o_sa = S.in(count ? samples : nullptr, cnt * sizeof(mipx::PcSample)), o_sk = S.in(count ? keys : nullptr, cnt * 4),
                 o_cl = inout(cost_l, nn * 8), o_cr = inout(cost_r, nn * 8), o_ha = inout(has, nn), o_ti = inout(times, 2 * nn * 4),
                 o_ow = inout(own, 4 * nn * 8);
    int rc = S.alloc();
    if (rc == MIPX_OK) rc = S.upload();
    if (rc == MIPX_OK) {
        mipx::PcApplyArgs a{};
        a.n = n; a.sum = nullptr; a.count = count; a.samples = S.at<const mipx::PcSample>(o_sa); a.keys = S.at<const int32_t>(o_sk);
        a.cost_l = S.at<double>(o_cl); a.cost_r = S.at<double>(o_cr); a.has = S.at<uint8_t>(o_ha);
        a.times = S.at<int32_t>(o_ti); a.own = S.at<double>(o_ow);
        hipLaunchKernelGGL(mipx::pc_apply, dim3(2 * n), dim3(64), 0, ctx->stream, a);
        if (hipError_t e = hipGetLastError()) rc = S.err("launch", e);
    }
    return S.finish(rc);
}

}  // extern "C"
