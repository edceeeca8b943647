// restart_api.hip.h -- host side and C entries of include/mipx_restart.h (included at the end of
// tree_engine.hip.h, behind treerec_api.hip.h, whose mirror upload it uses): the skeleton copy, the seeds'
// pool rows (restart_seed) and their queue entries.

namespace {

// rows a restarted search must find free beside its seeds: what mipx_tree_create keeps as the least pool
int64_t restart_reserve(const mipx_tree *t) { return 2 * (int64_t)t->max_batch + 2; }

// the seeds' pool rows, written on the device in chunks of kTrChunk (ids and rows are all that goes up)
int restart_seed_rows(mipx_tree *t, const std::vector<int32_t> &slots) {
    mipx_ctx *ctx = t->ctx;
    TreeRec &tr = t->tr;
    RestartRec &rs = t->rs;
    const int64_t S = (int64_t)rs.seeds.size();
    const int64_t chunk = std::min(S, kTrChunk);
    int64_t *d_ids = nullptr;
    int32_t *d_slots = nullptr;
    int rc = dmalloc(ctx, &d_ids, (size_t)chunk) | dmalloc(ctx, &d_slots, (size_t)chunk);
    hipStream_t st = ctx->stream;
    for (int64_t k0 = 0; !rc && k0 < S; k0 += kTrChunk) {
        const int cnt = (int)std::min(kTrChunk, S - k0);
        hipError_t e = hipMemcpyAsync(d_ids, rs.seeds.data() + k0, (size_t)cnt * 8, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(d_slots, slots.data() + k0, (size_t)cnt * 4, hipMemcpyHostToDevice, st);
        mipx::RestartSeedArgs a;
        a.n = t->n; a.nv = t->n + t->mrows; a.nodes_count = tr.d_count; a.capacity = t->capacity;
        a.nodes = tr.d_nodes; a.ids = d_ids; a.slots = d_slots;
        a.root_l = tr.d_root; a.root_u = tr.d_root + t->n; a.root_v = tr.have_root ? tr.d_root_v : nullptr;
        a.pool_l = t->pool_l; a.pool_u = t->pool_u; a.pool_v = t->pool_v;
        if (e == hipSuccess) e = hipEventRecord(tr.e0, st);
        if (e == hipSuccess) {
            enqueue_restart_seed(a, cnt, st);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipEventRecord(tr.e1, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);   // (the staging is reused by the next chunk)
        if (e != hipSuccess) { rc = fail(ctx, MIPX_EHIP, "mipx_tree_create_restart: seeding", e); break; }
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, tr.e0, tr.e1) == hipSuccess) rs.seed_us += 1000.0 * ms;
        rs.bytes += (int64_t)cnt * (2 * (int64_t)t->n * 8 + a.nv);
    }
    if (d_ids) (void)hipFree(d_ids);
    if (d_slots) (void)hipFree(d_slots);
    return rc ? (rc < 0 ? rc : MIPX_EHIP) : MIPX_OK;
}

}  // namespace

extern "C" {

int mipx_tree_create_restart(mipx_tree *src, mipx_problem *p, mipx_tree **out) {
    if (!src || !p || !out) return fail(src ? src->ctx : (p ? p->ctx : nullptr), MIPX_EINVAL, "mipx_tree_create_restart: bad argument");
    mipx_ctx *ctx = src->ctx;
    *out = nullptr;
    if (!src->tr.on) return fail(ctx, MIPX_EINVAL, "mipx_tree_create_restart: the source keeps no record (mipx_tree_set_tree_record)");
    if (src->cuts) return fail(ctx, MIPX_EINVAL, "mipx_tree_create_restart: not from a search with cut rounds");
    if (src->comm) return fail(ctx, MIPX_EINVAL, "mipx_tree_create_restart: not from a search with a communicator");
    if (p->ctx != ctx) return fail(ctx, MIPX_EINVAL, "mipx_tree_create_restart: problem of another context");
    if (p->m != src->m || p->n != src->n)
        return fail(ctx, MIPX_EINVAL, "mipx_tree_create_restart: the problem's shape differs from the source's");
    for (const StepBuf &S : src->buf)
        if (S.in_flight) return fail(ctx, MIPX_EINVAL, "mipx_tree_create_restart: a step of the source is in flight");
    const int64_t N = (int64_t)src->nodes.size();
    const TreeRec &sr = src->tr;
    std::vector<int64_t> seeds;
    for (int64_t id = 0; id < N; id++)
        if (!(sr.flags[(size_t)id] & MIPX_TR_HAS_CHILDREN)) seeds.push_back(id);
    const int64_t S = (int64_t)seeds.size();
    if (S + restart_reserve(src) > src->capacity) {
        char msg[200];
        std::snprintf(msg, sizeof msg, "mipx_tree_create_restart: %lld seeds and the %lld rows a step reserves do not fit "
                      "the pool of %lld rows (raise pool_capacity)", (long long)S, (long long)restart_reserve(src),
                      (long long)src->capacity);
        return fail(ctx, MIPX_ENOMEM, msg);
    }
    mipx_tree *t = nullptr;
    int rc = mipx_tree_create_ex(p, src->int_idx.data(), src->n_int, src->root_l.data(), src->root_u.data(), src->rule,
                                 src->search, src->sb_iters, src->max_batch, src->capacity, nullptr, &t);
    if (rc) return rc;
    // recording on, as mipx_tree_set_tree_record turns it on: every step is finished on the host
    TreeRec &tr = t->tr;
    tr.on = true;
    t->fast_ok = false;
    RestartRec &rs = t->rs;
    rs.on = true;
    rs.skeleton = N;
    rs.seeds = seeds;
    // the skeleton: who every node is; what its LP said is reset
    const double inf = std::numeric_limits<double>::infinity();
    for (int64_t id = 0; id < N; id++) {
        NodeRec r = src->nodes[(size_t)id];
        r.dual_bound = -inf;
        r.key = t->search == 0 ? -inf : -(double)r.depth;
        r.slot = -1; r.anchor = -1; r.born = 0; r.ncut = 0;
        if (id == 0) t->nodes[0] = r;
        else t->nodes.push_back(r);
    }
    tr.parent = sr.parent;
    tr.status.assign((size_t)N, -1);
    tr.obj.assign((size_t)N, 0.0);
    tr.flags.resize((size_t)N);
    for (int64_t id = 0; id < N; id++) tr.flags[(size_t)id] = sr.flags[(size_t)id] & MIPX_TR_HAS_CHILDREN;
    tr.root_v = sr.root_v;
    tr.have_root = sr.have_root;
    rc = mipx_tree_set_pseudo_costs(t, src->cost_l.data(), src->cost_r.data(), src->times_l.data(), src->times_r.data());
    // the seeds: rows 0 .. S - 1 of the pool in id order, the free list behind them
    std::vector<int32_t> slots((size_t)S);
    for (int64_t k = 0; k < S; k++) {
        slots[(size_t)k] = (int32_t)k;
        t->nodes[(size_t)seeds[(size_t)k]].slot = (int32_t)k;
    }
    t->free_slots.clear();
    for (int64_t s = t->capacity - 1; s >= S; s--) t->free_slots.push_back((int32_t)s);
    if (!rc) rc = tr_prepare(t, 0);   // the device mirror (TrNode) of the skeleton, the root's rows and basis codes
    if (!rc) rc = restart_seed_rows(t, slots);
    if (rc) { mipx_tree_destroy(t); return rc; }
    t->started = true;   // (the queue starts with the seeds, not with the root)
    t->bq.hold = t->use_bq;
    for (int64_t id : seeds) tree_push(t, id);
    *out = t;
    return MIPX_OK;
}

int mipx_tree_restart_stats(mipx_tree *t, int64_t out[8]) {
    if (!t || !out) return MIPX_EINVAL;
    const RestartRec &rs = t->rs;
    for (int k = 0; k < 8; k++) out[k] = 0;
    if (!rs.on) return MIPX_OK;
    out[0] = rs.skeleton; out[1] = (int64_t)rs.seeds.size(); out[2] = rs.bytes; out[3] = (int64_t)rs.seed_us;
    for (int64_t id : rs.seeds) {
        const int st = t->tr.status[(size_t)id];
        if (st < 0) continue;
        out[4]++;
        if (st == 1) out[5]++;
        if (t->tr.flags[(size_t)id] & MIPX_TR_MIP_FEASIBLE) out[6]++;
    }
    return MIPX_OK;
}

int64_t mipx_tree_restart_seeds(mipx_tree *t, int64_t cap, int64_t *ids) {
    if (!t || cap < 0 || (cap > 0 && !ids)) return MIPX_EINVAL;
    const RestartRec &rs = t->rs;
    const int64_t S = (int64_t)rs.seeds.size();
    for (int64_t k = 0; k < std::min(cap, S); k++) ids[k] = rs.seeds[(size_t)k];
    return S;
}

}  // extern "C"
