// dualfn.hip.h -- host side of the dual function (include/mipx_dualfn.h): the per-step record launch, the
// store's growth, the penalised re-solve of infeasible leaves and the evaluation.  Included by
// tree_engine.hip.h inside its anonymous namespace (needs mipx_tree, launch_lp_any, problem_args, fail).

constexpr size_t kDfEntry = 16;   // bytes per entry of a step's lists: src, lrow (i32), dst (i64)

int64_t df_record_bytes(const mipx_tree *t) { return 8 * ((int64_t)t->m + 1); }
int64_t df_inf_bytes(const mipx_tree *t) { return 16 * (int64_t)t->n + t->n + t->m; }

// the step buffers' y and entry staging, for the dive depth of this solve
int df_prepare(mipx_tree *t) {
    mipx_ctx *ctx = t->ctx;
    const size_t rows = (size_t)(1 + t->dive) * (size_t)t->max_batch;
    if (rows <= t->df.ystep_rows) return MIPX_OK;
    HIP_TRY(ctx, hipDeviceSynchronize());
    for (StepBuf &S : t->buf) {
        if (S.df_y) (void)hipFree(S.df_y);
        if (S.df_d) (void)hipFree(S.df_d);
        if (S.df_h) (void)hipHostFree(S.df_h);
        S.df_y = nullptr; S.df_d = nullptr; S.df_h = nullptr;
        int rc = dmalloc(ctx, &S.df_y, rows * (size_t)t->m);
        rc |= dmalloc(ctx, &S.df_d, 2 * rows * kDfEntry);
        if (rc) return rc;
        HIP_TRY(ctx, hipHostMalloc((void **)&S.df_h, 2 * rows * kDfEntry, hipHostMallocDefault));
        if (!S.df_e0) {
            HIP_TRY(ctx, hipEventCreate(&S.df_e0));
            HIP_TRY(ctx, hipEventCreate(&S.df_e1));
        }
    }
    t->df.ystep_rows = rows;
    return MIPX_OK;
}

// device time of the last record launch of S (complete by now)
void df_take_time(mipx_tree *t, StepBuf &S) {
    if (!S.df_timed) return;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, S.df_e0, S.df_e1) == hipSuccess) t->df.record_us += 1000.0 * ms;
    S.df_timed = false;
}

// grow a device array by doubling (its contents kept); the streams that may write it are synchronised first
template <typename T>
int df_grow(mipx_tree *t, T **p, int64_t &have, int64_t need, size_t row, int64_t *cap_rows = nullptr) {
    if (need <= have) return MIPX_OK;
    mipx_ctx *ctx = t->ctx;
    int64_t want = std::max<int64_t>(need, std::max<int64_t>(1024, 2 * have));
    if (cap_rows && want > *cap_rows) want = std::max(need, *cap_rows);
    HIP_TRY(ctx, hipStreamSynchronize(t->st3));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    T *q = nullptr;
    int rc = dmalloc(ctx, &q, (size_t)want * row);
    if (rc) return rc;
    if (*p && have > 0) HIP_TRY(ctx, hipMemcpy(q, *p, (size_t)have * row * sizeof(T), hipMemcpyDeviceToDevice));
    if (*p) (void)hipFree(*p);
    *p = q;
    have = want;
    return MIPX_OK;
}

// The launches of dualfn_record and dualfn_save, the grid from the count (count > 0): df_step, the end of
// df_penalised and the entries of dualfn_batch_api.hip.h go through these two and through df_eval_tiles below.
void enqueue_df_record(const mipx::DfRecordArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(mipx::dualfn_record, dim3((unsigned)((a.count + mipx::kDfRecRB - 1) / mipx::kDfRecRB)), dim3(mipx::kDfNT), 0, st, a);
}
void enqueue_df_save(const mipx::DfSaveArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(mipx::dualfn_save, dim3((unsigned)a.count), dim3(mipx::kDfNT), 0, st, a);
}

// The records of one host-finished step: recs = (output position, pool row, node id) of the nodes whose LP
// ended optimal, infs = the same of those whose LP was infeasible, both in evaluation order.  Queued on cs
// behind the step's children records (the dive children's rows hold their bounds by then).
struct DfEntry { int32_t pos, slot; int64_t id; };
int df_step(mipx_tree *t, StepBuf &S, hipStream_t cs, const std::vector<DfEntry> &recs, const std::vector<DfEntry> &infs) {
    mipx_ctx *ctx = t->ctx;
    DualFn &df = t->df;
    df_take_time(t, S);
    if (recs.empty() && infs.empty()) return MIPX_OK;
    const size_t rows = df.ystep_rows;
    int32_t *src = (int32_t *)S.df_h, *lrow = src + rows;
    int64_t *dst = (int64_t *)(S.df_h + 8 * rows);
    int32_t *isrc = (int32_t *)(S.df_h + 16 * rows), *ilrow = isrc + rows;
    int64_t *idst = (int64_t *)(S.df_h + 24 * rows);
    const int64_t rb = df_record_bytes(t), ib = df_inf_bytes(t);
    int nr = 0, ni = 0;
    for (const DfEntry &e : recs) {
        if (df.bytes + rb > df.cap) { df.dropped++; continue; }
        df.bytes += rb;
        const int64_t r = (int64_t)df.rec_node.size();
        df.rec_node.push_back(e.id);
        df.rec_status.push_back(0);
        df.rec[(size_t)e.id] = (int32_t)r;
        src[nr] = e.pos; lrow[nr] = e.slot; dst[nr] = r; nr++;
    }
    for (const DfEntry &e : infs) {
        if (df.bytes + ib > df.cap) { df.dropped++; continue; }
        df.bytes += ib;
        const int64_t r = (int64_t)df.inf_node.size();
        df.inf_node.push_back(e.id);
        isrc[ni] = e.pos; ilrow[ni] = e.slot; idst[ni] = r; ni++;
    }
    df.dirty = true;
    if (nr == 0 && ni == 0) return MIPX_OK;
    int64_t rcap = df.cap / rb, icap = df.cap / ib;
    int rc = MIPX_OK;
    const size_t ncol = (size_t)t->n, nv = (size_t)t->n + t->m;
    if ((int64_t)df.rec_node.size() > df.rcap) {   // (y and t grow together)
        int64_t hy = df.rcap, ht = df.rcap;
        if ((rc = df_grow(t, &df.d_y, hy, (int64_t)df.rec_node.size(), (size_t)t->m, &rcap))) return rc;
        if ((rc = df_grow(t, &df.d_t, ht, (int64_t)df.rec_node.size(), 1, &rcap))) return rc;
        df.rcap = hy;
    }
    if ((int64_t)df.inf_node.size() > df.icap) {
        int64_t h1 = df.icap, h2 = df.icap, h3 = df.icap;
        if ((rc = df_grow(t, &df.d_il, h1, (int64_t)df.inf_node.size(), ncol, &icap))) return rc;
        if ((rc = df_grow(t, &df.d_iu, h2, (int64_t)df.inf_node.size(), ncol, &icap))) return rc;
        if ((rc = df_grow(t, &df.d_iv, h3, (int64_t)df.inf_node.size(), nv, &icap))) return rc;
        df.icap = h1;
    }
    HIP_TRY(ctx, hipEventRecord(S.df_e0, cs));
    HIP_TRY(ctx, hipMemcpyAsync(S.df_d, S.df_h, 2 * rows * kDfEntry, hipMemcpyHostToDevice, cs));
    if (nr > 0) {
        mipx::DfRecordArgs a;
        a.m = t->m; a.n = t->n; a.A = t->prob->dA; a.c = t->prob->dc; a.count = nr;
        a.src = (const int32_t *)S.df_d; a.lrow = a.src + rows; a.dst = (const int64_t *)(S.df_d + 8 * rows);
        a.y_src = S.df_y; a.l = t->pool_l; a.u = t->pool_u; a.store_y = df.d_y; a.store_t = df.d_t;
        enqueue_df_record(a, cs);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (ni > 0) {
        mipx::DfSaveArgs a;
        a.n = t->n; a.nv = (int)nv; a.count = ni;
        a.vpos = (const int32_t *)(S.df_d + 16 * rows); a.lrow = a.vpos + rows; a.dst = (const int64_t *)(S.df_d + 24 * rows);
        a.l = t->pool_l; a.u = t->pool_u; a.vstat = S.d_vout;
        a.out_l = df.d_il; a.out_u = df.d_iu; a.out_v = df.d_iv;
        enqueue_df_save(a, cs);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipEventRecord(S.df_e1, cs));
    S.df_timed = true;
    return MIPX_OK;
}

// The first evaluation after new infeasible leaves: all of them in one launch of the penalised LP
// [A | S] (x, s) >= b, costs (c, M), 0 <= s (mipx_dualfn.h), warm-started from the leaf's codes with the
// slacks at their lower bound, row codes as the LP's own row status maps them back (lp.py _store /
// _warm_start); each optimal result becomes the leaf's record.
int df_penalised(mipx_tree *t, double M) {
    mipx_ctx *ctx = t->ctx;
    DualFn &df = t->df;
    const int64_t first = df.inf_done, P = (int64_t)df.inf_node.size() - first;
    if (P <= 0) return MIPX_OK;
    df.inf_done = (int64_t)df.inf_node.size();
    const int n = t->n, m = t->m, nr = df.rows, np = n + nr, nv = n + m, npv = np + m;
    if (m < 1 || np > mipx::kBigMaxN || !shape_supported(m, np)) { df.noterm += P; return MIPX_OK; }
    if (df.hostA.empty()) {
        df.hostA.resize((size_t)m * n + m + n);
        HIP_TRY(ctx, hipMemcpy(df.hostA.data(), t->prob->dA, (size_t)m * n * 8, hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(df.hostA.data() + (size_t)m * n, t->prob->db, (size_t)m * 8, hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(df.hostA.data() + (size_t)m * n + m, t->prob->dc, (size_t)n * 8, hipMemcpyDeviceToHost));
    }
    const double *A = df.hostA.data(), *b = A + (size_t)m * n, *c = b + m;
    std::vector<double> Ap((size_t)m * np, 0.0), cp((size_t)np, M);
    for (int e = 0; e < m; e++) {
        std::memcpy(&Ap[(size_t)e * np], A + (size_t)e * n, (size_t)n * 8);
        Ap[(size_t)e * np + n + df.pos[(size_t)e]] = df.sign[(size_t)e];
    }
    std::memcpy(cp.data(), c, (size_t)n * 8);
    mipx_problem *pp = nullptr;
    int rc = mipx_problem_create(ctx, m, np, Ap.data(), b, cp.data(), &pp);
    if (rc) return rc;
    // the leaves' saved rows, widened by the slack block
    std::vector<double> il((size_t)P * n), iu((size_t)P * n);
    std::vector<int8_t> iv((size_t)P * nv);
    rc = MIPX_OK;
    if (hipMemcpy(il.data(), df.d_il + (size_t)first * n, il.size() * 8, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(iu.data(), df.d_iu + (size_t)first * n, iu.size() * 8, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(iv.data(), df.d_iv + (size_t)first * nv, iv.size(), hipMemcpyDeviceToHost) != hipSuccess)
        rc = fail(ctx, MIPX_EHIP, "mipx_tree_dual_function: reading the infeasible leaves");
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<double> lp((size_t)P * np), up((size_t)P * np);
    std::vector<int8_t> vp((size_t)P * npv);
    std::vector<int8_t> rstat((size_t)nr);
    for (int64_t k = 0; k < P && !rc; k++) {
        std::memcpy(&lp[(size_t)k * np], &il[(size_t)k * n], (size_t)n * 8);
        std::memcpy(&up[(size_t)k * np], &iu[(size_t)k * n], (size_t)n * 8);
        for (int j = n; j < np; j++) { lp[(size_t)k * np + j] = 0.0; up[(size_t)k * np + j] = inf; }
        const int8_t *v = &iv[(size_t)k * nv];
        int8_t *w = &vp[(size_t)k * npv];
        std::memcpy(w, v, (size_t)n);
        for (int j = n; j < np; j++) w[j] = 3;
        // row status of the LP's rows: 3 where a >= side is tight, then 2 where a <= side is (written second)
        std::fill(rstat.begin(), rstat.end(), (int8_t)1);
        for (int e = 0; e < m; e++)
            if (df.sign[(size_t)e] > 0 && v[n + e] != 1) rstat[(size_t)df.pos[(size_t)e]] = 3;
        for (int e = 0; e < m; e++)
            if (df.sign[(size_t)e] < 0 && v[n + e] != 1) rstat[(size_t)df.pos[(size_t)e]] = 2;
        for (int e = 0; e < m; e++) {
            const int8_t code = rstat[(size_t)df.pos[(size_t)e]];
            const bool tight = df.sign[(size_t)e] > 0 ? code == 3 : code == 2;
            w[np + e] = tight ? 3 : 1;
        }
    }
    // one block: l, u (P x np), y (P x m), x (P x np), status, obj, iters, npiv, entries, vstat in / out
    char *blk = nullptr;
    const size_t PP = (size_t)P;
    const size_t o_u = PP * np * 8, o_y = 2 * o_u, o_x = o_y + PP * m * 8, o_st = o_x + PP * np * 8,
                 o_obj = o_st + PP * 4, o_it = o_obj + PP * 8, o_np = o_it + PP * 4, o_src = o_np + PP * 4,
                 o_dst = o_src + PP * 4, o_vi = o_dst + PP * 8, o_vo = o_vi + PP * npv, total = o_vo + PP * npv;
    if (!rc && hipMalloc((void **)&blk, total) != hipSuccess) rc = fail(ctx, MIPX_EHIP, "mipx_tree_dual_function: hipMalloc");
    std::vector<int32_t> st((size_t)P);
    if (!rc) {
        if (hipMemcpy(blk, lp.data(), o_u, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(blk + o_u, up.data(), o_u, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(blk + o_vi, vp.data(), PP * npv, hipMemcpyHostToDevice) != hipSuccess)
            rc = fail(ctx, MIPX_EHIP, "mipx_tree_dual_function: staging the penalised LPs");
    }
    if (!rc) {
        mipx::LpArgs a = problem_args(pp, false);
        a.l = (const double *)blk; a.u = (const double *)(blk + o_u); a.vstat_in = (const int8_t *)(blk + o_vi);
        a.status = (int32_t *)(blk + o_st); a.obj = (double *)(blk + o_obj); a.x = (double *)(blk + o_x);
        a.y = (double *)(blk + o_y); a.vstat_out = (int8_t *)(blk + o_vo);
        a.iters = (int32_t *)(blk + o_it); a.npivots = (int32_t *)(blk + o_np); a.batch = (int)P;
        rc = launch_lp_any(pp, a, (int)P);
        if (!rc && (hipStreamSynchronize(ctx->stream) != hipSuccess ||
                    hipMemcpy(st.data(), blk + o_st, PP * 4, hipMemcpyDeviceToHost) != hipSuccess))
            rc = fail(ctx, MIPX_EHIP, "mipx_tree_dual_function: the penalised re-solve");
    }
    if (!rc) {
        df.resolves += P;
        std::vector<int32_t> src;
        std::vector<int64_t> dst;
        const int64_t rb = df_record_bytes(t);
        for (int64_t k = 0; k < P; k++) {
            const int64_t id = df.inf_node[(size_t)(first + k)];
            if (st[(size_t)k] != 0) { df.noterm++; continue; }
            if (df.bytes + rb > df.cap) { df.dropped++; df.noterm++; continue; }
            df.bytes += rb;
            const int64_t r = (int64_t)df.rec_node.size();
            df.rec_node.push_back(id);
            df.rec_status.push_back(1);
            df.rec[(size_t)id] = (int32_t)r;
            src.push_back((int32_t)k);
            dst.push_back(r);
        }
        df.dirty = true;
        const int cnt = (int)src.size();
        if (cnt > 0) {
            int64_t rcap = df.cap / rb;
            if ((int64_t)df.rec_node.size() > df.rcap) {
                int64_t hy = df.rcap, ht = df.rcap;
                rc = df_grow(t, &df.d_y, hy, (int64_t)df.rec_node.size(), (size_t)m, &rcap);
                if (!rc) rc = df_grow(t, &df.d_t, ht, (int64_t)df.rec_node.size(), 1, &rcap);
                if (!rc) df.rcap = hy;
            }
            if (!rc && (hipMemcpy(blk + o_src, src.data(), (size_t)cnt * 4, hipMemcpyHostToDevice) != hipSuccess ||
                        hipMemcpy(blk + o_dst, dst.data(), (size_t)cnt * 8, hipMemcpyHostToDevice) != hipSuccess))
                rc = fail(ctx, MIPX_EHIP, "mipx_tree_dual_function: staging the records");
            if (!rc) {
                mipx::DfRecordArgs a;
                a.m = m; a.n = np; a.A = pp->dA; a.c = pp->dc; a.count = cnt;
                a.src = (const int32_t *)(blk + o_src); a.lrow = a.src; a.dst = (const int64_t *)(blk + o_dst);
                a.y_src = (const double *)(blk + o_y); a.l = (const double *)blk; a.u = (const double *)(blk + o_u);
                a.store_y = df.d_y; a.store_t = df.d_t;
                enqueue_df_record(a, ctx->stream);
                if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess)
                    rc = fail(ctx, MIPX_EHIP, "mipx_tree_dual_function: recording the penalised duals");
            }
        }
    }
    if (blk) (void)hipFree(blk);
    mipx_problem_destroy(pp);
    return rc;
}

// the lineage arrays: per record its nearest recorded ancestor and level, records by level, the leaves
int df_lineage(mipx_tree *t) {
    mipx_ctx *ctx = t->ctx;
    DualFn &df = t->df;
    if (!df.dirty) return MIPX_OK;
    const size_t N = t->nodes.size(), R = df.rec_node.size();
    std::vector<int32_t> eff(N), prec(R, -1), lvl(R, 0), leaf;
    int bare = 0;
    for (size_t id = 0; id < N; id++) {   // (a parent's id is below its children's)
        const int64_t p = df.parent[id];
        const int32_t pe = p >= 0 ? eff[(size_t)p] : -1;
        const int32_t r = df.rec[id];
        if (r >= 0) { prec[(size_t)r] = pe; eff[id] = r; } else eff[id] = pe;
    }
    int nlvl = R ? 1 : 0;
    for (size_t r = 0; r < R; r++) {
        lvl[r] = prec[r] < 0 ? 0 : lvl[(size_t)prec[r]] + 1;
        nlvl = std::max(nlvl, lvl[r] + 1);
    }
    std::vector<int32_t> off((size_t)nlvl + 1, 0), order(R);
    for (size_t r = 0; r < R; r++) off[(size_t)lvl[r] + 1]++;
    for (int L = 0; L < nlvl; L++) off[(size_t)L + 1] += off[(size_t)L];
    {
        std::vector<int32_t> fill(off.begin(), off.end() - 1);
        for (size_t r = 0; r < R; r++) order[(size_t)fill[(size_t)lvl[r]]++] = (int32_t)r;
    }
    for (size_t id = 0; id < N; id++)
        if (!df.haschild[id]) {
            if (eff[id] < 0) bare = 1;
            else leaf.push_back(eff[id]);
        }
    int32_t *ptrs[4] = {df.d_prec, df.d_order, df.d_lvl, df.d_leaf};
    for (int32_t *q : ptrs)
        if (q) (void)hipFree(q);
    df.d_prec = df.d_order = df.d_lvl = df.d_leaf = nullptr;
    int rc = dmalloc(ctx, &df.d_prec, R) | dmalloc(ctx, &df.d_order, R) | dmalloc(ctx, &df.d_lvl, off.size()) |
             dmalloc(ctx, &df.d_leaf, leaf.size());
    if (rc) return rc;
    if (R) {
        HIP_TRY(ctx, hipMemcpy(df.d_prec, prec.data(), R * 4, hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(df.d_order, order.data(), R * 4, hipMemcpyHostToDevice));
    }
    HIP_TRY(ctx, hipMemcpy(df.d_lvl, off.data(), off.size() * 4, hipMemcpyHostToDevice));
    if (!leaf.empty()) HIP_TRY(ctx, hipMemcpy(df.d_leaf, leaf.data(), leaf.size() * 4, hipMemcpyHostToDevice));
    df.nlvl = nlvl; df.nleaf = (int)leaf.size(); df.bare = bare;
    df.dirty = false;
    return MIPX_OK;
}

// right-hand sides per tile: V of a tile is R x Kt f64, at most 256 MB; k_tile > 0 caps it further (the test entry)
int df_tile(int64_t R, int K, int k_tile) {
    const int64_t budget = ((int64_t)256 << 20) / 8;
    int64_t Kt = std::max<int64_t>(1, std::min<int64_t>({(int64_t)K, (int64_t)1024, budget / R}));
    if (k_tile > 0) Kt = std::min<int64_t>(Kt, k_tile);
    return (int)Kt;
}

// The device arrays of an evaluation: R records (Y, T), their lineage, and room for one tile (W: Kt x m, V: Kt x R,
// out: Kt, with Kt = df_tile(R, K, k_tile)).
struct DfEvalDev {
    int R = 0, m = 0;
    const double *Y = nullptr, *T = nullptr;
    const int32_t *prec = nullptr, *order = nullptr, *lvl_off = nullptr, *leaf = nullptr;
    int nlvl = 0, nleaf = 0, bare = 0;
    double *W = nullptr, *V = nullptr, *out = nullptr;
};

// The tile loop of an evaluation, queued on ctx->stream (the caller syncs): per tile the upload of its right-hand sides
// from w (host, K x m), dualfn_gemm, dualfn_lineage and the download of its values into out (host, K).  v_gemm and v_max
// (host, K x R, or null) take V as it is between the two kernels and after them: the test entry's, null in the engine.
int df_eval_tiles(mipx_ctx *ctx, const DfEvalDev &d, int K, int k_tile, const double *w, double *out, double *v_gemm,
                  double *v_max) {
    const int Kt = df_tile(d.R, K, k_tile), m = d.m;
    const size_t R = (size_t)d.R;
    hipStream_t st = ctx->stream;
    for (int k0 = 0; k0 < K; k0 += Kt) {
        const int kt = std::min(Kt, K - k0);
        HIP_TRY(ctx, hipMemcpyAsync(d.W, w + (size_t)k0 * m, (size_t)kt * m * 8, hipMemcpyHostToDevice, st));
        mipx::DfGemmArgs g;
        g.R = d.R; g.m = m; g.K = kt; g.Y = d.Y; g.T = d.T; g.W = d.W; g.V = d.V;
        hipLaunchKernelGGL(mipx::dualfn_gemm, dim3((unsigned)((R + mipx::kDfTR - 1) / mipx::kDfTR), (unsigned)((kt + mipx::kDfTK - 1) / mipx::kDfTK)),
                           dim3(mipx::kDfNT), 0, st, g);
        HIP_TRY(ctx, hipGetLastError());
        if (v_gemm) HIP_TRY(ctx, hipMemcpyAsync(v_gemm + (size_t)k0 * R, d.V, (size_t)kt * R * 8, hipMemcpyDeviceToHost, st));
        mipx::DfLineageArgs a;
        a.R = d.R; a.K = kt; a.V = d.V; a.prec = d.prec; a.order = d.order; a.lvl_off = d.lvl_off;
        a.nlvl = d.nlvl; a.leaf = d.leaf; a.nleaf = d.nleaf; a.bare = d.bare; a.out = d.out;
        hipLaunchKernelGGL(mipx::dualfn_lineage, dim3((unsigned)kt), dim3(mipx::kDfNT), 0, st, a);
        HIP_TRY(ctx, hipGetLastError());
        if (v_max) HIP_TRY(ctx, hipMemcpyAsync(v_max + (size_t)k0 * R, d.V, (size_t)kt * R * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(out + k0, d.out, (size_t)kt * 8, hipMemcpyDeviceToHost, st));
    }
    return MIPX_OK;
}

// f(w_k) for K right-hand sides, in tiles of the right-hand sides (df_tile)
int df_evaluate(mipx_tree *t, int K, const double *w, double *out) {
    mipx_ctx *ctx = t->ctx;
    DualFn &df = t->df;
    const int m = t->m;
    const int64_t R = (int64_t)df.rec_node.size();
    if (R == 0 || df.nleaf == 0) {   // no term anywhere: nothing bounds the leaves
        for (int k = 0; k < K; k++) out[k] = df.nleaf == 0 && !df.bare ? std::numeric_limits<double>::infinity()
                                                                        : -std::numeric_limits<double>::infinity();
        return MIPX_OK;
    }
    const int Kt = df_tile(R, K, 0);
    int64_t hv = (int64_t)df.vcap, hw = (int64_t)df.wcap, ho = (int64_t)df.ocap;
    if ((size_t)(R * Kt) > df.vcap) { if (df.d_V) (void)hipFree(df.d_V); df.d_V = nullptr; int rc = dmalloc(ctx, &df.d_V, (size_t)(R * Kt)); if (rc) return rc; hv = R * Kt; }
    if ((size_t)Kt * m > df.wcap) { if (df.d_W) (void)hipFree(df.d_W); df.d_W = nullptr; int rc = dmalloc(ctx, &df.d_W, (size_t)Kt * m); if (rc) return rc; hw = (int64_t)Kt * m; }
    if ((size_t)Kt > df.ocap) { if (df.d_out) (void)hipFree(df.d_out); df.d_out = nullptr; int rc = dmalloc(ctx, &df.d_out, (size_t)Kt); if (rc) return rc; ho = Kt; }
    df.vcap = (size_t)hv; df.wcap = (size_t)hw; df.ocap = (size_t)ho;
    DfEvalDev d;
    d.R = (int)R; d.m = m; d.Y = df.d_y; d.T = df.d_t; d.prec = df.d_prec; d.order = df.d_order; d.lvl_off = df.d_lvl;
    d.nlvl = df.nlvl; d.leaf = df.d_leaf; d.nleaf = df.nleaf; d.bare = df.bare; d.W = df.d_W; d.V = df.d_V; d.out = df.d_out;
    int rc = df_eval_tiles(ctx, d, K, 0, w, out, nullptr, nullptr);
    if (rc) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return MIPX_OK;
}
