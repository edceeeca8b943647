// mir_api.hip.h -- the C entry of include/mipx_mir.h (included by mipx.hip behind tree_engine.hip.h, with mir_kernels.hip.h).
// The prologue is the shared one of mipx.hip (check_int_idx, check_bounds), the timed launch and the finish are timed_launch_finish's.

extern "C" {

int mipx_mir_separate_batch(mipx_problem *p, int batch, const double *x, const double *l, const double *u,
                            const int32_t *int_idx, int n_int, const uint8_t *row_integral, int n_mult,
                            const double *mult, int max_divisors, double f0_min, double min_efficacy,
                            double max_dynamism, double *pi_out, double *pi0_out, double *efficacy_out,
                            double *delta_out, int32_t *sign_out, int32_t *status_out) {
    if (!p) return MIPX_EINVAL;
    mipx_ctx *ctx = p->ctx;
    const int R = mult ? n_mult : p->m;
    if (batch < 0 || n_int < 0 || n_int > p->n || n_mult < 0 || (n_int && !int_idx) ||
        max_divisors < 1 || max_divisors > mipx::kMirMaxDiv || !(f0_min > 0.0 && f0_min < 0.5) ||
        min_efficacy != min_efficacy || !(max_dynamism >= 1.0) || (batch && R < 1) ||
        (batch && (!x || !l || !u || !pi_out || !pi0_out || !efficacy_out || !delta_out || !sign_out || !status_out)))
        return fail(ctx, MIPX_EINVAL, "mipx_mir_separate_batch: bad argument");
    if (int rc = check_int_idx(ctx, "mipx_mir_separate_batch", int_idx, n_int, p->n)) return rc;
    if (p->m > mipx::kMirMax || p->n > mipx::kMirMax)
        return fail(ctx, MIPX_ETOOBIG, "mipx_mir_separate_batch: more than 1024 rows or columns");
    const size_t B = (size_t)batch, nn = (size_t)p->n, mm = (size_t)p->m, RR = (size_t)R;
    if (int rc = check_bounds(ctx, "mipx_mir_separate_batch", x, l, u, B * nn)) return rc;
    for (size_t e = 0; mult && e < RR * mm; e++)
        if (!std::isfinite(mult[e])) return fail(ctx, MIPX_EINVAL, "mipx_mir_separate_batch: a multiplier that is not finite");
    if (batch == 0) return MIPX_OK;
    if (B * RR > (size_t)0x7fffffff) return fail(ctx, MIPX_ETOOBIG, "mipx_mir_separate_batch: more than 2^31 - 1 base rows in one launch");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Staging S(ctx, "mipx_mir_separate_batch");
    const size_t o_x = S.in(x, B * nn * 8), o_l = S.in(l, B * nn * 8), o_u = S.in(u, B * nn * 8),
                 o_ii = S.in(n_int ? int_idx : nullptr, (size_t)(n_int ? n_int : 1) * 4),
                 o_ri = S.in(row_integral, mm ? mm : 1), o_mu = S.in(mult, (mult ? RR * mm : 1) * 8),
                 o_pi = S.out(pi_out, B * RR * nn * 8), o_p0 = S.out(pi0_out, B * RR * 8),
                 o_ef = S.out(efficacy_out, B * RR * 8), o_de = S.out(delta_out, B * RR * 8),
                 o_sg = S.out(sign_out, B * RR * 4), o_st = S.out(status_out, B * RR * 4);
    int rc = S.alloc(p->scratch, p->scratch_bytes);
    if (rc == MIPX_OK) rc = S.upload();
    return timed_launch_finish(S, rc, [&] {
        mipx::MirArgs a;
        a.m = p->m; a.n = p->n; a.n_int = n_int; a.R = R; a.max_div = max_divisors;
        a.f0_min = f0_min; a.min_eff = min_efficacy; a.max_dyn = max_dynamism;
        a.A = p->dA; a.b = p->db;
        a.x = S.at<const double>(o_x); a.l = S.at<const double>(o_l); a.u = S.at<const double>(o_u);
        a.int_idx = S.at<const int32_t>(o_ii);
        a.row_int = row_integral ? S.at<const uint8_t>(o_ri) : nullptr;
        a.mult = mult ? S.at<const double>(o_mu) : nullptr;
        a.pi = S.at<double>(o_pi); a.pi0 = S.at<double>(o_p0); a.eff = S.at<double>(o_ef); a.delta = S.at<double>(o_de);
        a.sign = S.at<int32_t>(o_sg); a.status = S.at<int32_t>(o_st);
        hipLaunchKernelGGL(mipx::mir_separate, dim3((unsigned)(B * RR)), dim3(mipx::kMirNT), 0, ctx->stream, a);
    });
}

}  // extern "C"
