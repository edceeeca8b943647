// supportkernels_api.hip.h -- the C entries of include/mipx_supportkernels.h (included at the end of tree_engine.hip.h,
// whose enqueue_support_* functions are the one launch site of each kernel): the kernels behind a support evaluation
// on a caller's leaves.  Test scaffolding: no product code calls them.

namespace {

constexpr int64_t kSkMaxT = (int64_t)1 << 30;

// in and out: uploaded whole, copied back whole (an empty array is neither)
size_t sk_in(Staging &S, const void *p, size_t bytes) { return S.in(bytes ? p : nullptr, bytes); }
size_t sk_inout(Staging &S, void *p, size_t bytes) {
    const size_t o = sk_in(S, p, bytes);
    if (bytes) S.down(p, o, bytes);
    return o;
}

int sk_launched(Staging &S, int rc) {
    if (rc != MIPX_OK) return rc;
    if (hipError_t e = hipGetLastError()) return S.err("launch", e);
    return MIPX_OK;
}

// what the gather and the scatter share: the sizes and the packed positions
int sk_move_check(mipx_ctx *ctx, const char *who, int64_t count, int64_t T, int n, int m, const int32_t *packed) {
    if (count < 0 || T < 0 || count > kSkMaxT || T > kSkMaxT) return refuse(ctx, who, "count or T negative or above 2^30");
    if (count > T) return refuse(ctx, who, "count > T");
    if (n < 1 || m < 0) return refuse(ctx, who, "n < 1 or m < 0");
    if (!packed) return refuse(ctx, who, "a null argument");
    for (int64_t k = 0; k < count; k++)
        if (packed[k] < 0 || packed[k] >= T) return refuse(ctx, who, "a packed position outside 0 .. T-1");
    return MIPX_OK;
}

}  // namespace

extern "C" {

int mipx_support_select_batch(mipx_ctx *ctx, int64_t T, int n, int P, double pi0, double tol, const int64_t *ids,
                              const int32_t *status, const double *obj, const double *x, const int32_t *iters,
                              const int32_t *npivots, double *margin, double *cand_m, int32_t *cand_id, int32_t *cand_t,
                              double *seg_sum, double *block) {
    if (!ctx) return MIPX_EINVAL;
    const char *who = "mipx_support_select_batch";
    if (T < 0 || T > kSkMaxT) return refuse(ctx, who, "T negative or above 2^30");
    if (P < 1 || P > mipx::kSupMaxP) return refuse(ctx, who, "P outside 1 .. 1024");
    if (n < 1) return refuse(ctx, who, "n < 1");
    if (!(tol >= 0.0) || pi0 != pi0) return refuse(ctx, who, "tol negative or NaN, or pi0 NaN");
    if (!ids || !status || !obj || !x || !iters || !npivots || !margin || !cand_m || !cand_id || !cand_t || !seg_sum || !block)
        return refuse(ctx, who, "a null argument");
    for (int64_t t = 0; t < T; t++)
        if (ids[t] < 0 || ids[t] >= (int64_t)mipx::kSupNone) return refuse(ctx, who, "an id outside 0 .. 2^31 - 2");
    if (T == 0) return MIPX_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t K = (size_t)T, nn = (size_t)n, G = (size_t)sup_segments(T), C = G * (size_t)P;
    Staging S(ctx, who);
    const size_t o_ids = sk_in(S, ids, K * 8), o_st = sk_in(S, status, K * 4), o_obj = sk_in(S, obj, K * 8), o_x = sk_in(S, x, K * nn * 8),
                 o_it = sk_in(S, iters, K * 4), o_np = sk_in(S, npivots, K * 4);
    const size_t o_mg = sk_inout(S, margin, K * 8), o_cm = sk_inout(S, cand_m, C * 8), o_ci = sk_inout(S, cand_id, C * 4),
                 o_ct = sk_inout(S, cand_t, C * 4), o_ss = sk_inout(S, seg_sum, G * 4 * 8),
                 o_b = sk_inout(S, block, ((size_t)mipx::kSupHead + (size_t)P * (nn + 2)) * 8);
    int rc = S.alloc();
    if (rc == MIPX_OK) rc = S.upload();
    if (rc == MIPX_OK) {
        mipx::SupSelectArgs a;
        a.n = n; a.P = P; a.pi0 = pi0; a.tol = tol;
        a.ids = S.at<const int64_t>(o_ids); a.status = S.at<const int32_t>(o_st); a.obj = S.at<const double>(o_obj);
        a.x = S.at<const double>(o_x); a.iters = S.at<const int32_t>(o_it); a.npivots = S.at<const int32_t>(o_np);
        a.margin = S.at<double>(o_mg); a.cand_m = S.at<double>(o_cm); a.cand_id = S.at<int32_t>(o_ci); a.cand_t = S.at<int32_t>(o_ct);
        a.seg_sum = S.at<double>(o_ss); a.block = S.at<double>(o_b);
        enqueue_support_select(a, (int)T, ctx->stream);
        enqueue_support_select_merge(a, (int)T, ctx->stream);
        rc = sk_launched(S, rc);
    }
    return S.finish(rc);
}

int mipx_support_pack_batch(mipx_ctx *ctx, int64_t T, int mode, double pi0, const uint8_t *skip, const int32_t *status,
                            const double *bound, int32_t *seg_count, double *seg_min, int32_t *packed,
                            int32_t *count_out, double *min_margin_out) {
    if (!ctx) return MIPX_EINVAL;
    const char *who = "mipx_support_pack_batch";
    if (T < 0 || T > kSkMaxT) return refuse(ctx, who, "T negative or above 2^30");
    if (mode != 0 && mode != 1) return refuse(ctx, who, "mode not 0 or 1");
    if (pi0 != pi0) return refuse(ctx, who, "pi0 NaN");
    if ((mode == 0 ? !skip : !status) || !seg_count || !seg_min || !packed || !count_out || !min_margin_out)
        return refuse(ctx, who, "a null argument");
    if (T == 0) return MIPX_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t K = (size_t)T, G = (size_t)sup_segments(T);
    mipx::SupPackInfo info = {*count_out, 0, *min_margin_out};   // the caller's two words go up like every other output
    Staging S(ctx, who);
    const size_t o_sk = sk_in(S, skip, K), o_st = sk_in(S, status, K * 4), o_bd = sk_in(S, bound, K * 8);
    const size_t o_sc = sk_inout(S, seg_count, G * 4), o_sm = sk_inout(S, seg_min, G * 8), o_p = sk_inout(S, packed, K * 4),
                 o_i = sk_inout(S, &info, sizeof info);
    int rc = S.alloc();
    if (rc == MIPX_OK) rc = S.upload();
    if (rc == MIPX_OK) {
        mipx::SupPackArgs a;
        a.skip = skip ? S.at<const uint8_t>(o_sk) : nullptr;
        a.status = mode == 1 ? S.at<const int32_t>(o_st) : nullptr;
        a.bound = bound ? S.at<const double>(o_bd) : nullptr;
        a.pi0 = pi0;
        a.seg_count = S.at<int32_t>(o_sc); a.seg_min = S.at<double>(o_sm); a.packed = S.at<int32_t>(o_p);
        a.info = S.at<mipx::SupPackInfo>(o_i);
        enqueue_support_pack_count(a, (int)T, ctx->stream);
        enqueue_support_pack(a, (int)T, ctx->stream);
        rc = sk_launched(S, rc);
    }
    rc = S.finish(rc);
    if (rc == MIPX_OK) { *count_out = info.count; *min_margin_out = info.min_margin; }
    return rc;
}

int mipx_support_gather_batch(mipx_ctx *ctx, int64_t count, int64_t T, int n, int m, const int32_t *packed,
                              const double *l, const double *u, const int8_t *v, double *pl, double *pu, int8_t *pv_in) {
    if (!ctx) return MIPX_EINVAL;
    const char *who = "mipx_support_gather_batch";
    if (int rc = sk_move_check(ctx, who, count, T, n, m, packed)) return rc;
    if (!l || !u || !pl || !pu || (v && !pv_in)) return refuse(ctx, who, "a null argument");
    if (count == 0) return MIPX_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t K = (size_t)T, cnt = (size_t)count, nn = (size_t)n, nv = nn + (size_t)m;
    Staging S(ctx, who);
    const size_t o_pk = sk_in(S, packed, cnt * 4), o_l = sk_in(S, l, K * nn * 8), o_u = sk_in(S, u, K * nn * 8), o_v = sk_in(S, v, K * nv);
    const size_t o_pl = sk_inout(S, pl, cnt * nn * 8), o_pu = sk_inout(S, pu, cnt * nn * 8), o_pv = sk_inout(S, pv_in, cnt * nv);
    int rc = S.alloc();
    if (rc == MIPX_OK) rc = S.upload();
    if (rc == MIPX_OK) {
        mipx::SupMoveArgs a;
        a.T = (int)T; a.n = n; a.m = m; a.packed = S.at<const int32_t>(o_pk);
        a.l = S.at<double>(o_l); a.u = S.at<double>(o_u); a.v = v ? S.at<int8_t>(o_v) : nullptr;
        a.pl = S.at<double>(o_pl); a.pu = S.at<double>(o_pu); a.pv_in = S.at<int8_t>(o_pv);
        enqueue_support_gather(a, (int)count, ctx->stream);
        rc = sk_launched(S, rc);
    }
    return S.finish(rc);
}

int mipx_support_scatter_batch(mipx_ctx *ctx, int64_t count, int64_t T, int n, int m, const int32_t *packed, int add,
                               const double *px, const double *pobj, const double *py, const int8_t *pv_out,
                               const int32_t *pstatus, const int32_t *piters, const int32_t *pnpivots, double *x,
                               double *obj, double *y, int8_t *v, int32_t *status, int32_t *iters, int32_t *npivots,
                               uint8_t *has_y) {
    if (!ctx) return MIPX_EINVAL;
    const char *who = "mipx_support_scatter_batch";
    if (int rc = sk_move_check(ctx, who, count, T, n, m, packed)) return rc;
    if (!px || !pobj || !py || !pv_out || !pstatus || !piters || !pnpivots || !x || !obj || !y || !v || !status || !iters ||
        !npivots || !has_y)
        return refuse(ctx, who, "a null argument");
    {
        std::vector<int32_t> s(packed, packed + count);
        std::sort(s.begin(), s.end());
        if (std::adjacent_find(s.begin(), s.end()) != s.end()) return refuse(ctx, who, "a position named twice in packed");
    }
    if (count == 0) return MIPX_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t K = (size_t)T, cnt = (size_t)count, nn = (size_t)n, mm = (size_t)m, nv = nn + mm;
    Staging S(ctx, who);
    const size_t o_pk = sk_in(S, packed, cnt * 4), o_px = sk_in(S, px, cnt * nn * 8), o_po = sk_in(S, pobj, cnt * 8),
                 o_py = sk_in(S, py, cnt * mm * 8), o_pv = sk_in(S, pv_out, cnt * nv), o_ps = sk_in(S, pstatus, cnt * 4),
                 o_pi = sk_in(S, piters, cnt * 4), o_pn = sk_in(S, pnpivots, cnt * 4);
    const size_t o_x = sk_inout(S, x, K * nn * 8), o_obj = sk_inout(S, obj, K * 8), o_y = sk_inout(S, y, K * mm * 8),
                 o_v = sk_inout(S, v, K * nv), o_st = sk_inout(S, status, K * 4), o_it = sk_inout(S, iters, K * 4),
                 o_np = sk_inout(S, npivots, K * 4), o_h = sk_inout(S, has_y, K);
    int rc = S.alloc();
    if (rc == MIPX_OK) rc = S.upload();
    if (rc == MIPX_OK) {
        mipx::SupMoveArgs a;
        a.T = (int)T; a.n = n; a.m = m; a.packed = S.at<const int32_t>(o_pk); a.add = add ? 1 : 0;
        a.px = S.at<double>(o_px); a.pobj = S.at<double>(o_po); a.py = S.at<double>(o_py); a.pv_out = S.at<int8_t>(o_pv);
        a.pstatus = S.at<int32_t>(o_ps); a.piters = S.at<int32_t>(o_pi); a.pnpivots = S.at<int32_t>(o_pn);
        a.x = S.at<double>(o_x); a.obj = S.at<double>(o_obj); a.y = S.at<double>(o_y); a.v = S.at<int8_t>(o_v);
        a.status = S.at<int32_t>(o_st); a.iters = S.at<int32_t>(o_it); a.npivots = S.at<int32_t>(o_np); a.has_y = S.at<uint8_t>(o_h);
        enqueue_support_scatter(a, (int)count, ctx->stream);
        rc = sk_launched(S, rc);
    }
    return S.finish(rc);
}

int mipx_support_mark_batch(mipx_ctx *ctx, int64_t T, const int32_t *status, uint8_t *has_y) {
    if (!ctx) return MIPX_EINVAL;
    const char *who = "mipx_support_mark_batch";
    if (T < 0 || T > kSkMaxT) return refuse(ctx, who, "T negative or above 2^30");
    if (!status || !has_y) return refuse(ctx, who, "a null argument");
    if (T == 0) return MIPX_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t K = (size_t)T;
    Staging S(ctx, who);
    const size_t o_st = sk_in(S, status, K * 4), o_h = sk_inout(S, has_y, K);
    int rc = S.alloc();
    if (rc == MIPX_OK) rc = S.upload();
    if (rc == MIPX_OK) {
        enqueue_support_mark((int)T, S.at<const int32_t>(o_st), S.at<uint8_t>(o_h), ctx->stream);
        rc = sk_launched(S, rc);
    }
    return S.finish(rc);
}

}  // extern "C"
