/*
 * mipx_complete.h -- complete heuristic points over the continuous columns by one batched LP (included by mipx.h).
 *
 * The heuristics of mipx_heur.h, mipx_lsearch.h, mipx_fixprop.h, mipx_wrepair.h and mipx_cube.h move integer columns
 * only: "the other columns keep x_j", the value they had in the node's LP point.  On a model with continuous columns
 * that leaves a rounded point infeasible where other values of the continuous columns would satisfy every row, and
 * a feasible one short of the objective its integers allow.  The standard cure: hold the integer columns where the
 * heuristic put them and solve the LP over the rest.  That LP is a node LP -- the problem's rows and objective,
 * bounds with l = u on the integer columns -- and is solved by the node-LP kernels, a batch of points in one launch.
 * The engine can run this on the points its heuristics end on (mipx_tree_set_completion) or a caller on points of
 * their own (mipx_complete_batch).
 *
 * For one point x~ of the problem's rows A x >= b (m x n), objective c, bounds l, u (the root's), the integer
 * columns int_idx and a tolerance ctol >= 0:
 *
 * ROUNDED BOUNDS.  lr_j = ceil(l_j - ctol), ur_j = floor(u_j + ctol) for an integer column j.
 * PREPARE.  L_j = U_j = x~_j for an integer column; L_j = l_j, U_j = u_j for any other (u_j may be +inf).  The point
 *           is SKIPPED if its skip byte is set, or if for an integer column x~_j is not an integer or lies outside
 *           [lr_j, ur_j].
 * SOLVE.    min c.x, A x >= b, L <= x <= U by the node-LP kernel of mipx_lp_solve_batch (K1 on the register tiles,
 *           K1b above them), with its default iteration limit, from the caller's basis codes where given (a warm
 *           start: a basis of the same rows stays dual feasible when only bounds change) and cold otherwise.  The
 *           problem's anchor, if one is set, is not used.
 * FINISH.   Only where the LP ended optimal: x^_j = x~_j exactly on the integer columns and the LP's x_j elsewhere;
 *           s_i = a_i . x^ - b_i (columns ascending, from +0, products not fused) and obj = sum of c_j x^_j (columns
 *           ascending, from +0).  The point is COMPLETED when every s_i >= -ctol and every other column has
 *           l_j - ctol <= x^_j <= u_j + ctol; otherwise it is REJECTED: the LP said optimal, the recomputed point
 *           does not hold.
 * STATUS.   COMPLETED 0, INFEASIBLE 1 (the LP is infeasible), LIMIT 2 (the LP hit its iteration limit or is
 *           unbounded), SKIPPED 3, REJECTED 4.  0 and 3 are the heuristic's feasible and skipped, as the cube's are.
 * OUTPUT.   x^, obj, the status and the LP's pivot count (tableau pivots, the warm start's refactorisation
 *           included; 0 for a SKIPPED point).  A point that is not COMPLETED returns x~ unchanged and obj 0.
 *
 * VALIDITY.  A COMPLETED point satisfies every row within ctol, is integral in the integer columns and equal there
 *           to x~; its objective is the LP's optimum for those integers.  The other statuses say nothing about the
 *           problem.
 * ARITHMETIC.  The LP is the node-LP kernel's, bit for bit what mipx_lp_solve_batch gives on (L, U) and the codes;
 *           FINISH's sums are one add per term in the stated order.  A restatement around that LP gives the same
 *           bits (tests/support/completion_reference.py).
 * NO HOST WAIT.  The launch always hands the LP kernel a row of basis codes per point: the caller's, or all 0, which
 *           the kernels read as "no basis" -- the same cold start as a null pointer, to the bit.  A launch with
 *           codes never takes the path of the single cold LP above the register tiles (K1c, one launch per pivot
 *           with the host reading a status word between chunks), so a completion of one point inside a step queues
 *           like any other and the host does not wait for it.  A SKIPPED point still occupies its workgroup: its
 *           columns are all fixed at l_j, an LP that ends without a pivot.
 */
#ifndef MIPX_COMPLETE_H
#define MIPX_COMPLETE_H

#ifdef __cplusplus
extern "C" {
#endif

#define MIPX_COMPLETE_COMPLETED 0
#define MIPX_COMPLETE_INFEASIBLE 1
#define MIPX_COMPLETE_LIMIT 2
#define MIPX_COMPLETE_SKIPPED 3
#define MIPX_COMPLETE_REJECTED 4

/*
 * Host buffers, one call.  x: batch x n points; l, u: n each; int_idx: n_int distinct columns (n_int == n is legal:
 * the LP then only confirms or refutes the point); vstat: null (cold), or batch x (n + m) basis codes in the layout
 * of mipx_lp_solve_batch; skip: null, or batch bytes (non-zero: the point is skipped).  x_out: batch x n; obj_out,
 * status_out, pivots_out: batch.
 * MIPX_EINVAL: a null or out-of-range argument, ctol < 0 or NaN, int_idx out of range or repeated, an l that is not
 * finite (the LP kernels' form), a u that is NaN or -inf, an integer column whose u is not finite, an x that is not
 * finite; MIPX_ETOOBIG: m or n above 1024.  A batch of 0 is no launch.
 */
int mipx_complete_batch(mipx_problem *p, int batch, const double *x, const double *l, const double *u,
                        const int32_t *int_idx, int n_int, const int8_t *vstat, double ctol, const uint8_t *skip,
                        double *x_out, double *obj_out, int32_t *status_out, int32_t *pivots_out);
/*
 * Run the completion inside the search, once in every step the primal heuristic runs in, behind the last stage of
 * every block of points (the lift, and the local search where that is on) and before the step is handed to the
 * host: the heuristic's block (its own points and those of the dive or the weighted repair in its slots), every
 * point that is not skipped, whatever its status, and the cube's FOUND points, in ONE LP launch, with the root's
 * bounds and ctol = 1e-6.  A COMPLETED point takes its source point's place in the contest for the step's
 * incumbent, with the source's family and position (a tie goes to the earlier family, then to the lowest position);
 * a point whose LP does not end COMPLETED competes as before.  What is completed is what a slot holds at that time:
 * a slot in which the dive or the weighted repair ran and failed holds the LP point again (their OUTPUT), and PREPARE
 * skips it unless it is integral; a cube without a point leaves the LP point too, which is no heuristic's point and
 * is skipped.
 * Warm start: point k of either block starts from the final basis codes of node LP k of the step -- the LP whose
 * solution the heuristics took as point k; the step buffers hold that basis whenever they hold the point, so every
 * completion inside a step is warm.  Points a caller passes to mipx_complete_batch without codes start cold.
 * Nothing depends on which: both end in an optimal basis of the same LP.
 * on = 1 sets it, 0 switches it off again.  Set before the first step.  On a problem with no continuous column
 * (n_int == n) the setter succeeds, nothing is launched and the stats stay 0.  With the option on, every step is
 * finished on the host, as with the heuristic.
 * MIPX_EINVAL: a tree without the heuristic (mipx_tree_set_heuristic first, which refuses cut rounds and a
 * communicator), a tree that has stepped.  A later mipx_tree_set_heuristic with more points than this was set for
 * is refused, as with the cube search.
 */
int mipx_tree_set_completion(mipx_tree *t, int on);
/*
 * [0] points tried (not skipped), [1] of those, ended COMPLETED, [2] LP infeasible, [3] limit or rejected,
 * [4] completed points that no family had ended feasible (rescued), [5] incumbents installed from a completed
 * point, [6] LP pivots, [7] device time of the two kernels and the LP launch in microseconds.  All 0 on a tree
 * without the option.
 */
int mipx_tree_completion_stats(mipx_tree *t, int64_t out[8]);

#ifdef __cplusplus
}
#endif
#endif /* MIPX_COMPLETE_H */
