/*
 * mipx_objstep.h -- the objective-step cutoff of the frontier engine (included by mipx.h).
 *
 * Where the objective values of any two integer-feasible points differ by a multiple of a known step (a pure-integer
 * model with integer costs: the gcd of the costs), a node whose LP bound z is above U - step holds no point better
 * than an incumbent of value U.  The engine prunes at z >= U; with the step set it prunes at the cutoff
 *
 *     C(U) = U - step + 1e-6 * max(1, |U|)   where that is below U,   C(U) = U otherwise,   +inf without an incumbent.
 *
 * WHERE.  C(U) replaces U wherever the host decides from a bound whether a node goes on -- the pop of a step's
 * batch, the evaluation of a solved node, the dive chain of the pseudo-cost updates -- and wherever the incumbent
 * is handed to a kernel as a cutoff: the dive of the node LPs, the bound propagation (mipx_prop.h), the reduced-cost
 * tightening (mipx_rcfix.h).  Those kernels do not change.  What assigns, reports or exchanges the incumbent does
 * not change either: an integral node LP or a point of the heuristic becomes the incumbent when its value is below
 * U, and the gap is measured from U.
 * DUAL BOUND.  A node closed only because of the step (C(U) <= z < U), at the pop or after its LP, counts as a
 * closed leaf of value U, not z: by the guarantee below nothing in it is better than U.  So a search that empties
 * its queue ends with the dual bound on the primal bound, optimal at mip_gap 0.
 * THE CALLER GUARANTEES that the objective values of any two integer-feasible points differ by a multiple of step.
 * A bound given through mipx_tree_set_primal_bound must then be the objective of a feasible point (a bound that is
 * merely above the optimum would cut off the optimum that lies less than a step below it).
 */
#ifndef MIPX_OBJSTEP_H
#define MIPX_OBJSTEP_H

#ifdef __cplusplus
extern "C" {
#endif

/*
 * step > 0 and finite; set before the first step.  Every step is then finished on the host, as with
 * mipx_tree_set_heuristic.  It works beside the host spill, anchors, dives, both search rules, the propagation, the
 * reduced-cost tightening and the heuristic.
 * MIPX_EINVAL: a step that is not positive and finite, a tree with cut rounds, with a communicator, with the dual
 * function or the tree record on (a recorded bound would depend on the incumbent), a tree that has stepped.
 * A tree made by mipx_tree_create_restart has the tree record on from its creation and is refused with it.
 * mipx_tree_set_comm, mipx_tree_set_dual_record and mipx_tree_set_tree_record refuse a tree that has the step.
 */
int mipx_tree_set_objective_step(mipx_tree *t, double step);
/*
 * [0] nodes closed unevaluated at the pop under the step (C(U) <= bound < U), [1] evaluated nodes left unbranched
 * under the step, [2] launches whose cutoff was below the incumbent, [3] reserved (0), [4] reserved (0),
 * [5] reserved (0), [6] reserved (0), [7] reserved (0).  All 0 on a tree without the step.
 */
int mipx_tree_objective_step_stats(mipx_tree *t, int64_t out[8]);

#ifdef __cplusplus
}
#endif
#endif /* MIPX_OBJSTEP_H */
