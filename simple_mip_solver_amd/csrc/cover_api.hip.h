// cover_api.hip.h -- the C entry of include/mipx_cover.h (included by mipx.hip behind mir_api.hip.h, with cover_kernels.hip.h).
// The prologue is the shared one of mipx.hip (check_int_idx, check_bounds), the timed launch and the finish are timed_launch_finish's.

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
    if (int rc = check_int_idx(ctx, "mipx_cover_separate_batch", int_idx, n_int, p->n)) return rc;
    if (int rc = check_int_idx(ctx, "mipx_cover_separate_batch", rows, rows ? n_rows : 0, p->m, "rows out of range or repeated")) return rc;
    if (p->m > mipx::kCovMax || p->n > mipx::kCovMax)
        return fail(ctx, MIPX_ETOOBIG, "mipx_cover_separate_batch: more than 1024 rows or columns");
    const size_t B = (size_t)batch, nn = (size_t)p->n, RR = (size_t)R;
    if (int rc = check_bounds(ctx, "mipx_cover_separate_batch", x, l, u, B * nn)) return rc;
    if (batch == 0) return MIPX_OK;
    if (B * RR > (size_t)0x7fffffff) return fail(ctx, MIPX_ETOOBIG, "mipx_cover_separate_batch: more than 2^31 - 1 rows in one launch");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Staging S(ctx, "mipx_cover_separate_batch");
    const size_t o_x = S.in(x, B * nn * 8), o_l = S.in(l, B * nn * 8), o_u = S.in(u, B * nn * 8),
                 o_ii = S.in(n_int ? int_idx : nullptr, (size_t)(n_int ? n_int : 1) * 4),
                 o_ro = S.in(rows, (rows ? RR : 1) * 4),
                 o_pi = S.out(pi_out, B * RR * nn * 8), o_p0 = S.out(pi0_out, B * RR * 8),
                 o_ef = S.out(efficacy_out, B * RR * 8), o_sz = S.out(cover_size_out, B * RR * 4),
                 o_st = S.out(status_out, B * RR * 4);
    int rc = S.alloc(p->scratch, p->scratch_bytes);
    if (rc == MIPX_OK) rc = S.upload();
    return timed_launch_finish(S, rc, [&] {
        mipx::CoverArgs a;
        a.m = p->m; a.n = p->n; a.n_int = n_int; a.R = R; a.min_eff = min_efficacy;
        a.A = p->dA; a.b = p->db;
        a.x = S.at<const double>(o_x); a.l = S.at<const double>(o_l); a.u = S.at<const double>(o_u);
        a.int_idx = S.at<const int32_t>(o_ii);
        a.rows = rows ? S.at<const int32_t>(o_ro) : nullptr;
        a.pi = S.at<double>(o_pi); a.pi0 = S.at<double>(o_p0); a.eff = S.at<double>(o_ef);
        a.size = S.at<int32_t>(o_sz); a.status = S.at<int32_t>(o_st);
        hipLaunchKernelGGL(mipx::cover_separate, dim3((unsigned)(B * RR)), dim3(mipx::kCovNT), 0, ctx->stream, a);
    });
}

}  // extern "C"
