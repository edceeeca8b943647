// objstep_api.hip.h -- the C entries of include/mipx_objstep.h (included at the end of tree_engine.hip.h, which
// holds the cutoff itself: tree_cutoff, and its uses in tree_launch, finish_table and evaluate_node).

extern "C" {

int mipx_tree_set_objective_step(mipx_tree *t, double step) {
    if (!t) return MIPX_EINVAL;
    mipx_ctx *ctx = t->ctx;
    if (!(step > 0.0) || !std::isfinite(step))
        return fail(ctx, MIPX_EINVAL, "mipx_tree_set_objective_step: the step is positive and finite");
    if (t->cuts) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_objective_step: not with cut rounds");
    if (t->comm) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_objective_step: not with a communicator");
    if (t->df.on) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_objective_step: not with the dual function (mipx_tree_set_dual_record)");
    if (t->tr.on) return fail(ctx, MIPX_EINVAL, "mipx_tree_set_objective_step: not with the tree record (mipx_tree_set_tree_record)");
    if (t->steps > 0 || t->evaluated > 0)
        return fail(ctx, MIPX_EINVAL, "mipx_tree_set_objective_step: the step is set before the first step");
    t->os.step = step;
    t->os.on = true;
    // the cutoff is applied where the host evaluates a step's nodes: every step is finished on the host, the switch
    // mipx_tree_set_heuristic uses
    t->fast_ok = false;
    return MIPX_OK;
}

int mipx_tree_objective_step_stats(mipx_tree *t, int64_t out[8]) {
    if (!t || !out) return MIPX_EINVAL;
    const ObjStepState &os = t->os;
    out[0] = os.popped; out[1] = os.unbranched; out[2] = os.launches;
    for (int k = 3; k < 8; k++) out[k] = 0;
    return MIPX_OK;
}

}  // extern "C"
