// clique_api.hip.h -- the C entries of include/mipx_clique.h (included by mipx.hip behind cover_api.hip.h, with clique_kernels.hip.h).
// The prologue is the shared one of mipx.hip (check_int_idx, check_bounds), the timed launch and the finish are timed_launch_finish's.

namespace {

// The live literals of a box as Wd words: both bits of every column that is BINARY (mipx_cover.h).
std::vector<uint32_t> clique_live_words(const std::vector<uint8_t> &isint, const double *l, const double *u, int n, int Wd) {
    std::vector<uint32_t> live((size_t)Wd, 0u);
    for (int j = 0; j < n; j++)
        if (isint[(size_t)j] && std::isfinite(u[j]) && std::floor(l[j]) == l[j] && std::floor(u[j]) == u[j] && u[j] - l[j] == 1.0)
            live[(size_t)(2 * j) >> 5] |= 3u << ((2 * j) & 31);
    return live;
}

// The form of an adjacency among the live literals: no diagonal bit, no bit between the two literals of one column, symmetric.
bool clique_adj_well_formed(const uint32_t *adj, const std::vector<uint32_t> &live, int n, int Wd) {
    for (int k = 0; k < 2 * n; k++) {
        if (!(live[(size_t)k >> 5] >> (k & 31) & 1u)) continue;
        const uint32_t *row = adj + (size_t)k * Wd;
        if (row[k >> 5] & live[(size_t)k >> 5] & (3u << ((k & 31) & ~1))) return false;   // (k itself and its complement)
        for (int w = 0; w < Wd; w++) {
            uint32_t bits = row[w] & live[(size_t)w];
            while (bits) {
                const int h = 32 * w + __builtin_ctz(bits);
                bits &= bits - 1;
                if (!(adj[(size_t)h * Wd + (k >> 5)] >> (k & 31) & 1u)) return false;
            }
        }
    }
    return true;
}

}  // namespace

extern "C" {

int mipx_clique_graph(mipx_problem *p, const double *l, const double *u, const int32_t *int_idx, int n_int,
                      uint32_t *adj_out, int32_t *row_status_out) {
    if (!p) return MIPX_EINVAL;
    mipx_ctx *ctx = p->ctx;
    if (n_int < 0 || n_int > p->n || (n_int && !int_idx) || !l || !u || !adj_out || p->m < 1)
        return fail(ctx, MIPX_EINVAL, "mipx_clique_graph: bad argument");
    if (int rc = check_int_idx(ctx, "mipx_clique_graph", int_idx, n_int, p->n)) return rc;
    if (p->m > mipx::kCovMax || p->n > mipx::kCovMax)
        return fail(ctx, MIPX_ETOOBIG, "mipx_clique_graph: more than 1024 rows or columns");
    const size_t nn = (size_t)p->n, mm = (size_t)p->m;
    const int Wd = (2 * p->n + 31) / 32;
    const size_t adj_bytes = 2 * nn * (size_t)Wd * 4;
    if (int rc = check_bounds(ctx, "mipx_clique_graph", nullptr, l, u, nn)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Staging S(ctx, "mipx_clique_graph");
    const size_t o_l = S.in(l, nn * 8), o_u = S.in(u, nn * 8),
                 o_ii = S.in(n_int ? int_idx : nullptr, (size_t)(n_int ? n_int : 1) * 4),
                 o_adj = S.out(adj_out, adj_bytes), o_rs = S.out(row_status_out, mm * 4);
    int rc = S.alloc(p->scratch, p->scratch_bytes);
    if (rc == MIPX_OK) rc = S.upload();
    if (rc == MIPX_OK)
        if (hipError_t e = hipMemsetAsync(S.at<char>(o_adj), 0, adj_bytes, ctx->stream)) rc = S.err("memset", e);
    return timed_launch_finish(S, rc, [&] {
        mipx::CliqueGraphArgs a;
        a.m = p->m; a.n = p->n; a.n_int = n_int; a.Wd = Wd;
        a.A = p->dA; a.b = p->db;
        a.l = S.at<const double>(o_l); a.u = S.at<const double>(o_u);
        a.int_idx = S.at<const int32_t>(o_ii);
        a.adj = S.at<uint32_t>(o_adj); a.row_status = S.at<int32_t>(o_rs);
        hipLaunchKernelGGL(mipx::clique_graph, dim3((unsigned)mm), dim3(mipx::kCovNT), 0, ctx->stream, a);
    });
}

int mipx_clique_separate_batch(mipx_problem *p, int batch, const double *x, const double *l, const double *u,
                               const int32_t *int_idx, int n_int, const uint32_t *adj, const int32_t *seeds,
                               int n_seeds, double min_efficacy, double *pi_out, double *pi0_out,
                               double *efficacy_out, int32_t *size_out, int32_t *status_out) {
    if (!p) return MIPX_EINVAL;
    mipx_ctx *ctx = p->ctx;
    const int R = seeds ? n_seeds : 2 * p->n;
    if (batch < 0 || n_int < 0 || n_int > p->n || n_seeds < 0 || n_seeds > 2 * p->n || (n_int && !int_idx) ||
        min_efficacy != min_efficacy || (batch && R < 1) || !l || !u || !adj ||
        (batch && (!x || !pi_out || !pi0_out || !efficacy_out || !size_out || !status_out)))
        return fail(ctx, MIPX_EINVAL, "mipx_clique_separate_batch: bad argument");
    std::vector<uint8_t> isint;
    if (int rc = check_int_idx(ctx, "mipx_clique_separate_batch", int_idx, n_int, p->n, "int_idx out of range or repeated", &isint)) return rc;
    if (int rc = check_int_idx(ctx, "mipx_clique_separate_batch", seeds, seeds ? n_seeds : 0, 2 * p->n, "seeds out of range or repeated")) return rc;
    if (p->m > mipx::kCovMax || p->n > mipx::kCovMax)
        return fail(ctx, MIPX_ETOOBIG, "mipx_clique_separate_batch: more than 1024 rows or columns");
    const size_t B = (size_t)batch, nn = (size_t)p->n, RR = (size_t)R;
    const int Wd = (2 * p->n + 31) / 32;
    const size_t adj_bytes = 2 * nn * (size_t)Wd * 4;
    if (int rc = check_bounds(ctx, "mipx_clique_separate_batch", nullptr, l, u, nn)) return rc;
    if (int rc = check_points(ctx, "mipx_clique_separate_batch", x, B * nn)) return rc;
    if (!clique_adj_well_formed(adj, clique_live_words(isint, l, u, p->n, Wd), p->n, Wd))
        return refuse(ctx, "mipx_clique_separate_batch", "adj is not symmetric, has a diagonal bit or joins the two literals of a column");
    if (batch == 0) return MIPX_OK;
    if (B * RR > (size_t)0x7fffffff) return fail(ctx, MIPX_ETOOBIG, "mipx_clique_separate_batch: more than 2^31 - 1 seeds in one launch");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Staging S(ctx, "mipx_clique_separate_batch");
    const size_t o_x = S.in(x, B * nn * 8), o_l = S.in(l, nn * 8), o_u = S.in(u, nn * 8),
                 o_ii = S.in(n_int ? int_idx : nullptr, (size_t)(n_int ? n_int : 1) * 4),
                 o_adj = S.in(adj, adj_bytes), o_sd = S.in(seeds, (seeds ? RR : 1) * 4),
                 o_pi = S.out(pi_out, B * RR * nn * 8), o_p0 = S.out(pi0_out, B * RR * 8),
                 o_ef = S.out(efficacy_out, B * RR * 8), o_sz = S.out(size_out, B * RR * 4),
                 o_st = S.out(status_out, B * RR * 4);
    int rc = S.alloc(p->scratch, p->scratch_bytes);
    if (rc == MIPX_OK) rc = S.upload();
    return timed_launch_finish(S, rc, [&] {
        mipx::CliqueArgs a;
        a.n = p->n; a.n_int = n_int; a.R = R; a.Wd = Wd; a.min_eff = min_efficacy;
        a.x = S.at<const double>(o_x); a.l = S.at<const double>(o_l); a.u = S.at<const double>(o_u);
        a.int_idx = S.at<const int32_t>(o_ii);
        a.adj = S.at<const uint32_t>(o_adj);
        a.seeds = seeds ? S.at<const int32_t>(o_sd) : nullptr;
        a.pi = S.at<double>(o_pi); a.pi0 = S.at<double>(o_p0); a.eff = S.at<double>(o_ef);
        a.size = S.at<int32_t>(o_sz); a.status = S.at<int32_t>(o_st);
        hipLaunchKernelGGL(mipx::clique_separate, dim3((unsigned)(B * RR)), dim3(mipx::kCovNT), 0, ctx->stream, a);
    });
}

}  // extern "C"
