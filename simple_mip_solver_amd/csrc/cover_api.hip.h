// cover_api.hip.h -- the C entry of include/mipx_cover.h (included by mipx.hip behind mir_api.hip.h, with cover_kernels.hip.h).

extern "C" {

int mipx_cover_separate_batch(mipx_problem *p, int batch, const double *x, const double *l, const double *u,
                              const int32_t *int_idx, int n_int, const int32_t *rows, int n_rows, double min_efficacy,
                              double *pi_out, double *pi0_out, double *efficacy_out, int32_t *cover_size_out,
                              int32_t *status_out) {
    if (!p) return MIPX_EINVAL;
    mipx_ctx *ctx = p->ctx;
    const int R = rows ? n_rows : p->m;
    if (batch < 0 || n_int < 0 || n_int > p->n || n_rows < 0 || n_rows > p->m || (n_int && !int_idx) ||
        min_efficacy != min_efficacy || (batch && R < 1) ||
        (batch && (!x || !l || !u || !pi_out || !pi0_out || !efficacy_out || !cover_size_out || !status_out)))
        return fail(ctx, MIPX_EINVAL, "mipx_cover_separate_batch: bad argument");
    std::vector<uint8_t> seen((size_t)p->n, 0);
    for (int k = 0; k < n_int; k++) {
        if (int_idx[k] < 0 || int_idx[k] >= p->n || seen[(size_t)int_idx[k]])
            return fail(ctx, MIPX_EINVAL, "mipx_cover_separate_batch: int_idx out of range or repeated");
        seen[(size_t)int_idx[k]] = 1;
    }
    std::vector<uint8_t> seen_row((size_t)p->m, 0);
    for (int k = 0; rows && k < n_rows; k++) {
        if (rows[k] < 0 || rows[k] >= p->m || seen_row[(size_t)rows[k]])
            return fail(ctx, MIPX_EINVAL, "mipx_cover_separate_batch: rows out of range or repeated");
        seen_row[(size_t)rows[k]] = 1;
    }
    if (p->m > mipx::kCovMax || p->n > mipx::kCovMax)
        return fail(ctx, MIPX_ETOOBIG, "mipx_cover_separate_batch: more than 1024 rows or columns");
    const size_t B = (size_t)batch, nn = (size_t)p->n, RR = (size_t)R;
    for (size_t e = 0; e < B * nn; e++)
        if (!std::isfinite(x[e]) || !std::isfinite(l[e]) || u[e] != u[e] || u[e] == -std::numeric_limits<double>::infinity())
            return fail(ctx, MIPX_EINVAL, "mipx_cover_separate_batch: a point or a lower bound that is not finite, or an upper bound that is NaN or -inf");
    if (batch == 0) return MIPX_OK;
    if (B * RR > (size_t)0x7fffffff) return fail(ctx, MIPX_ETOOBIG, "mipx_cover_separate_batch: more than 2^31 - 1 rows in one launch");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!ctx->k0 && (hipEventCreate(&ctx->k0) != hipSuccess || hipEventCreate(&ctx->k1) != hipSuccess))
        return fail(ctx, MIPX_EHIP, "mipx_cover_separate_batch: events");
    Staging S(ctx, "mipx_cover_separate_batch");
    const size_t o_x = S.in(x, B * nn * 8), o_l = S.in(l, B * nn * 8), o_u = S.in(u, B * nn * 8),
                 o_ii = S.in(n_int ? int_idx : nullptr, (size_t)(n_int ? n_int : 1) * 4),
                 o_ro = S.in(rows, (rows ? RR : 1) * 4),
                 o_pi = S.out(pi_out, B * RR * nn * 8), o_p0 = S.out(pi0_out, B * RR * 8),
                 o_ef = S.out(efficacy_out, B * RR * 8), o_sz = S.out(cover_size_out, B * RR * 4),
                 o_st = S.out(status_out, B * RR * 4);
    int rc = S.alloc(p->scratch, p->scratch_bytes);
    if (rc == MIPX_OK) rc = S.upload();
    if (rc == MIPX_OK) {
        mipx::CoverArgs a;
        a.m = p->m; a.n = p->n; a.n_int = n_int; a.R = R; a.min_eff = min_efficacy;
        a.A = p->dA; a.b = p->db;
        a.x = S.at<const double>(o_x); a.l = S.at<const double>(o_l); a.u = S.at<const double>(o_u);
        a.int_idx = S.at<const int32_t>(o_ii);
        a.rows = rows ? S.at<const int32_t>(o_ro) : nullptr;
        a.pi = S.at<double>(o_pi); a.pi0 = S.at<double>(o_p0); a.eff = S.at<double>(o_ef);
        a.size = S.at<int32_t>(o_sz); a.status = S.at<int32_t>(o_st);
        (void)hipEventRecord(ctx->k0, ctx->stream);
        hipLaunchKernelGGL(mipx::cover_separate, dim3((unsigned)(B * RR)), dim3(mipx::kCovNT), 0, ctx->stream, a);
        if (hipError_t e = hipGetLastError()) rc = fail(ctx, MIPX_EHIP, "mipx_cover_separate_batch: launch", e);
        else (void)hipEventRecord(ctx->k1, ctx->stream);
    }
    rc = S.finish(rc);
    ctx->last_kernel_ms = -1.f;
    if (rc == MIPX_OK && hipEventElapsedTime(&ctx->last_kernel_ms, ctx->k0, ctx->k1) != hipSuccess) ctx->last_kernel_ms = -1.f;
    return rc;
}

}  // extern "C"
