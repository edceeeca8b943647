// dualfn_batch_api.hip.h -- the C entries of include/mipx_dualfn_batch.h (included at the end of tree_engine.hip.h,
// which holds enqueue_df_record, enqueue_df_save and df_eval_tiles through dualfn.hip.h): the kernels of the dual
// function on a caller's records.  Test scaffolding: no product code calls them.

namespace {

// every row index of a list inside [0, rows)
template <typename T>
bool df_rows_ok(const T *idx, int count, int rows) {
    for (int e = 0; e < count; e++)
        if (idx[e] < 0 || idx[e] >= rows) return false;
    return true;
}

// no record of the store written twice in one call (the kernels' blocks would race for it)
bool df_dst_distinct(const int64_t *dst, int count) {
    std::vector<int64_t> s(dst, dst + count);
    std::sort(s.begin(), s.end());
    return std::adjacent_find(s.begin(), s.end()) == s.end();
}

}  // namespace

extern "C" {

int mipx_dualfn_record_batch(mipx_ctx *ctx, int m, int n, const double *A, const double *c, int count, const int32_t *src,
                             const int32_t *lrow, const int64_t *dst, int y_rows, const double *y_src, int b_rows,
                             const double *l, const double *u, int store_rows, double *store_y, double *store_t) {
    if (!ctx) return MIPX_EINVAL;
    if (m < 1 || n < 1 || count < 0 || y_rows < 1 || b_rows < 1 || store_rows < 1)
        return fail(ctx, MIPX_EINVAL, "mipx_dualfn_record_batch: m, n, y_rows, b_rows or store_rows < 1, or count < 0");
    if (!A || !c || !y_src || !l || !u || !store_y || !store_t || (count > 0 && (!src || !lrow || !dst)))
        return fail(ctx, MIPX_EINVAL, "mipx_dualfn_record_batch: a null argument");
    // (the kernel indexes y_src, l, u and the store by these lists and by nothing else a caller sends)
    if (!df_rows_ok(src, count, y_rows)) return fail(ctx, MIPX_EINVAL, "mipx_dualfn_record_batch: a src outside y_src");
    if (!df_rows_ok(lrow, count, b_rows)) return fail(ctx, MIPX_EINVAL, "mipx_dualfn_record_batch: an lrow outside the bounds");
    if (!df_rows_ok(dst, count, store_rows)) return fail(ctx, MIPX_EINVAL, "mipx_dualfn_record_batch: a dst outside the store");
    if (!df_dst_distinct(dst, count)) return fail(ctx, MIPX_EINVAL, "mipx_dualfn_record_batch: two equal dst");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t mm = (size_t)m, nn = (size_t)n, cnt = (size_t)count;
    Staging S(ctx, "mipx_dualfn_record_batch");
    auto inout = [&S](void *p, size_t bytes) { const size_t o = S.in(p, bytes); S.down(p, o, bytes); return o; };
    const size_t o_A = S.in(A, mm * nn * 8), o_c = S.in(c, nn * 8), o_src = S.in(src, cnt * 4), o_lr = S.in(lrow, cnt * 4),
                 o_dst = S.in(dst, cnt * 8), o_y = S.in(y_src, (size_t)y_rows * mm * 8), o_l = S.in(l, (size_t)b_rows * nn * 8),
                 o_u = S.in(u, (size_t)b_rows * nn * 8);
    const size_t o_sy = inout(store_y, (size_t)store_rows * mm * 8), o_st = inout(store_t, (size_t)store_rows * 8);
    int rc = S.alloc();
    if (rc == MIPX_OK) rc = S.upload();
    if (rc == MIPX_OK && count > 0) {
        mipx::DfRecordArgs a;
        a.m = m; a.n = n; a.A = S.at<const double>(o_A); a.c = S.at<const double>(o_c); a.count = count;
        a.src = S.at<const int32_t>(o_src); a.lrow = S.at<const int32_t>(o_lr); a.dst = S.at<const int64_t>(o_dst);
        a.y_src = S.at<const double>(o_y); a.l = S.at<const double>(o_l); a.u = S.at<const double>(o_u);
        a.store_y = S.at<double>(o_sy); a.store_t = S.at<double>(o_st);
        enqueue_df_record(a, ctx->stream);
        if (hipError_t e = hipGetLastError()) rc = S.err("launch", e);
    }
    return S.finish(rc);
}

int mipx_dualfn_save_batch(mipx_ctx *ctx, int n, int nv, int count, const int32_t *lrow, const int32_t *vpos,
                           const int64_t *dst, int b_rows, const double *l, const double *u, int v_rows,
                           const int8_t *vstat, int out_rows, double *out_l, double *out_u, int8_t *out_v) {
    if (!ctx) return MIPX_EINVAL;
    if (n < 1 || nv < 1 || count < 0 || b_rows < 1 || v_rows < 1 || out_rows < 1)
        return fail(ctx, MIPX_EINVAL, "mipx_dualfn_save_batch: n, nv, b_rows, v_rows or out_rows < 1, or count < 0");
    if (!l || !u || !vstat || !out_l || !out_u || !out_v || (count > 0 && (!lrow || !vpos || !dst)))
        return fail(ctx, MIPX_EINVAL, "mipx_dualfn_save_batch: a null argument");
    if (!df_rows_ok(lrow, count, b_rows)) return fail(ctx, MIPX_EINVAL, "mipx_dualfn_save_batch: an lrow outside the bounds");
    if (!df_rows_ok(vpos, count, v_rows)) return fail(ctx, MIPX_EINVAL, "mipx_dualfn_save_batch: a vpos outside vstat");
    if (!df_rows_ok(dst, count, out_rows)) return fail(ctx, MIPX_EINVAL, "mipx_dualfn_save_batch: a dst outside the store");
    if (!df_dst_distinct(dst, count)) return fail(ctx, MIPX_EINVAL, "mipx_dualfn_save_batch: two equal dst");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)n, vv = (size_t)nv, cnt = (size_t)count;
    Staging S(ctx, "mipx_dualfn_save_batch");
    auto inout = [&S](void *p, size_t bytes) { const size_t o = S.in(p, bytes); S.down(p, o, bytes); return o; };
    const size_t o_lr = S.in(lrow, cnt * 4), o_vp = S.in(vpos, cnt * 4), o_dst = S.in(dst, cnt * 8),
                 o_l = S.in(l, (size_t)b_rows * nn * 8), o_u = S.in(u, (size_t)b_rows * nn * 8), o_vs = S.in(vstat, (size_t)v_rows * vv);
    const size_t o_ol = inout(out_l, (size_t)out_rows * nn * 8), o_ou = inout(out_u, (size_t)out_rows * nn * 8),
                 o_ov = inout(out_v, (size_t)out_rows * vv);
    int rc = S.alloc();
    if (rc == MIPX_OK) rc = S.upload();
    if (rc == MIPX_OK && count > 0) {
        mipx::DfSaveArgs a;
        a.n = n; a.nv = nv; a.count = count;
        a.lrow = S.at<const int32_t>(o_lr); a.vpos = S.at<const int32_t>(o_vp); a.dst = S.at<const int64_t>(o_dst);
        a.l = S.at<const double>(o_l); a.u = S.at<const double>(o_u); a.vstat = S.at<const int8_t>(o_vs);
        a.out_l = S.at<double>(o_ol); a.out_u = S.at<double>(o_ou); a.out_v = S.at<int8_t>(o_ov);
        enqueue_df_save(a, ctx->stream);
        if (hipError_t e = hipGetLastError()) rc = S.err("launch", e);
    }
    return S.finish(rc);
}

int mipx_dualfn_eval_batch(mipx_ctx *ctx, int R, int m, int K, int k_tile, const double *Y, const double *T,
                           const double *W, const int32_t *prec, const int32_t *order, const int32_t *lvl_off, int nlvl,
                           const int32_t *leaf, int nleaf, int bare, double *V_gemm, double *V_max, double *out) {
    if (!ctx) return MIPX_EINVAL;
    const char *who = "mipx_dualfn_eval_batch";
    if (R < 1 || m < 1 || K < 1 || k_tile < 0 || nlvl < 1 || nleaf < 0)
        return fail(ctx, MIPX_EINVAL, "mipx_dualfn_eval_batch: R, m, K or nlvl < 1, or k_tile or nleaf < 0");
    if (nleaf == 0 && !bare)
        return fail(ctx, MIPX_EINVAL, "mipx_dualfn_eval_batch: no leaf and none bare (the engine answers +inf on the host)");
    if (!Y || !T || !W || !prec || !order || !lvl_off || !out || (nleaf > 0 && !leaf))
        return fail(ctx, MIPX_EINVAL, "mipx_dualfn_eval_batch: a null argument");
    // (the lineage kernel indexes V by order, prec and leaf, and order by lvl_off)
    if (lvl_off[0] != 0 || lvl_off[nlvl] != R) return fail(ctx, MIPX_EINVAL, "mipx_dualfn_eval_batch: lvl_off does not run from 0 to R");
    for (int L = 0; L < nlvl; L++)
        if (lvl_off[L] >= lvl_off[L + 1]) return fail(ctx, MIPX_EINVAL, "mipx_dualfn_eval_batch: lvl_off is not ascending");
    std::vector<int32_t> lvl((size_t)R, -1);
    for (int L = 0; L < nlvl; L++)
        for (int q = lvl_off[L]; q < lvl_off[L + 1]; q++) {
            const int32_t r = order[q];
            if (r < 0 || r >= R || lvl[(size_t)r] >= 0) return fail(ctx, MIPX_EINVAL, "mipx_dualfn_eval_batch: order is no permutation of the records");
            lvl[(size_t)r] = L;
        }
    for (int r = 0; r < R; r++) {
        const int32_t p = prec[r];
        if (lvl[(size_t)r] == 0) {
            if (p != -1) return fail(ctx, MIPX_EINVAL, "mipx_dualfn_eval_batch: a record of level 0 with an ancestor");
        } else if (p < 0 || p >= R || lvl[(size_t)p] >= lvl[(size_t)r]) {
            return fail(ctx, MIPX_EINVAL, "mipx_dualfn_eval_batch: an ancestor that is no record of a lower level");
        }
    }
    if (!df_rows_ok(leaf, nleaf, R)) return fail(ctx, MIPX_EINVAL, "mipx_dualfn_eval_batch: a leaf outside the records");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t RR = (size_t)R, mm = (size_t)m, Kt = (size_t)df_tile(R, K, k_tile);
    Staging S(ctx, who);
    const size_t o_Y = S.in(Y, RR * mm * 8), o_T = S.in(T, RR * 8), o_pr = S.in(prec, RR * 4), o_or = S.in(order, RR * 4),
                 o_lv = S.in(lvl_off, ((size_t)nlvl + 1) * 4), o_lf = S.in(leaf, (size_t)nleaf * 4);
    const size_t o_W = S.carve(Kt * mm * 8), o_V = S.carve(Kt * RR * 8), o_out = S.carve(Kt * 8);
    int rc = S.alloc();
    if (rc == MIPX_OK) rc = S.upload();
    if (rc == MIPX_OK) {
        DfEvalDev d;
        d.R = R; d.m = m; d.Y = S.at<const double>(o_Y); d.T = S.at<const double>(o_T); d.prec = S.at<const int32_t>(o_pr);
        d.order = S.at<const int32_t>(o_or); d.lvl_off = S.at<const int32_t>(o_lv); d.leaf = S.at<const int32_t>(o_lf);
        d.nlvl = nlvl; d.nleaf = nleaf; d.bare = bare ? 1 : 0; d.W = S.at<double>(o_W); d.V = S.at<double>(o_V); d.out = S.at<double>(o_out);
        rc = df_eval_tiles(ctx, d, K, k_tile, W, out, V_gemm, V_max);
    }
    return S.finish(rc);
}

}  // extern "C"
