/*
 * mipx_wrepair.h -- a weighted row repair on the GPU: a second chance for rounded LP points (included by mipx.h).
 *
 * The rounding heuristic of mipx_heur.h repairs a rounded LP point by unit moves and stops (STUCK) where no single
 * move lowers the total violation, which happens on rows that pack and rows that cover side by side.  The weighted
 * repair keeps the heuristic's move rule and gives every row a weight: where no move helps, the weights of the
 * violated rows go up by one, until a move that mends them outweighs the rows it breaks.  A move or a bump costs one
 * sweep over A, as a move of the heuristic's repair does.  One workgroup per point; the engine can run it on the
 * points its rounding heuristic left infeasible (mipx_tree_set_weighted_repair) or a caller on points of their own
 * (mipx_weighted_repair_batch).
 *
 * For one point x of the problem's rows A x >= b (m x n), objective c, bounds l, u (the root's), the integer
 * columns int_idx, a tolerance tol >= 0 and a cap max_steps >= 0:
 *
 * ROUND.   Exactly the ROUND of mipx_heur.h: for an integer column j
 *          x~_j = min(max(floor(x_j + 0.5), ceil(l_j - tol)), floor(u_j + tol)), the other columns keep x_j (a
 *          rounded zero is +0); s_i = a_i . x~ - b_i (columns ascending, from +0).  Every weight w_i = 1.
 * STEP.    Repeat while some s_i < -tol.  If moves + bumps = max_steps the point is CAPPED.  Else V is the sum of
 *          w_i (-s_i) over the rows with s_i < -tol (rows ascending, from +0).  A candidate is an integer column j
 *          and d = +1 or -1 with x~_j + d inside the rounded bounds; its V' is the same sum over s_i + d a_ij.  The
 *          candidate with the smallest key (V', c_j d, j, +1 before -1) is the only one considered.  If its V' < V
 *          it is a move: x~_j += d, s_i += d a_ij.  Otherwise, or with no candidate at all, it is a bump:
 *          w_i += 1 for every row with s_i < -tol.
 * OUTPUT.  FEASIBLE returns x~ and obj = sum of c_j x~_j (columns ascending, from +0); CAPPED and SKIPPED return x
 *          unchanged and obj 0.  Each comes with the status and two counts (moves, bumps; none for SKIPPED).  The
 *          status numbering is the heuristic's; there is no STUCK.
 *
 * VALIDITY.  A FEASIBLE point satisfies every row within tol, is integral in the integer columns, inside the rounded
 *          bounds, and unchanged in the other columns.  Nothing is said about a CAPPED point: the problem may hold
 *          no such point at all, and then every point ends CAPPED.
 * ARITHMETIC.  As mipx_heur.h: products are not fused and every sum is one add per term in the stated order.  A
 *          term of V or V' is the product w_i * (-(s_i + d a_ij)), rounded once.  Weights are small integers (at
 *          most max_steps + 1) held as doubles in every product.  A restatement in that order gives the same bits
 *          (tests/support/weighted_repair_reference.py).
 */
#ifndef MIPX_WREPAIR_H
#define MIPX_WREPAIR_H

#ifdef __cplusplus
extern "C" {
#endif

#define MIPX_WR_FEASIBLE 0
#define MIPX_WR_CAPPED 2
#define MIPX_WR_SKIPPED 3

/*
 * Host buffers, one launch.  x: batch x n points; l, u: n each; int_idx: n_int distinct columns; skip: null, or
 * batch bytes (non-zero: the point is skipped); gate: null, or per point the status the rounding heuristic gave it
 * (a point whose entry is not 1 or 2, stuck or capped, is skipped).  x_out: batch x n; obj_out, status_out: batch;
 * counts_out: 2 per point (moves, bumps).
 * MIPX_EINVAL: a null or out-of-range argument, tol < 0, max_steps < 0, int_idx out of range or repeated, an l that
 * is not finite, a u that is NaN or -inf, an x that is not finite (as mipx_fix_propagate_batch);
 * MIPX_ETOOBIG: m or n above 1024.
 */
int mipx_weighted_repair_batch(mipx_problem *p, int batch, const double *x, const double *l, const double *u,
                               const int32_t *int_idx, int n_int, double tol, int max_steps, const uint8_t *skip,
                               const int32_t *gate, double *x_out, double *obj_out, int32_t *status_out,
                               int32_t *counts_out);
/*
 * Run the weighted repair inside the search, behind the primal heuristic of every step it runs in: on the same LP
 * points, but only those the rounding ended STUCK or CAPPED on, with the root's bounds, the heuristic's tol and
 * max_steps moves and bumps per point.  A point it ends FEASIBLE takes the place of the heuristic's and goes through
 * the heuristic once more, which lifts it (rounding an integral point changes nothing and its repair is empty), and
 * with mipx_tree_set_local_search through the pair search; it then competes for the step's incumbent like the
 * heuristic's own points.  Set before the first step.
 * MIPX_EINVAL: max_steps < 0, a tree without the heuristic (mipx_tree_set_heuristic first, which refuses cut rounds
 * and a communicator), a tree that has stepped, a tree that has the fix-and-propagate dive on: running the two one
 * behind the other is out of scope, and mipx_tree_set_fix_propagate refuses a tree with this option in turn.
 * max_steps = 0 switches it off again.  A later mipx_tree_set_heuristic with more points than this was set for is
 * refused, as with the local search.
 */
int mipx_tree_set_weighted_repair(mipx_tree *t, int max_steps);
/*
 * [0] points tried (not skipped), [1] of those, ended feasible, [2] capped, [3] moves, [4] bumps,
 * [5] incumbents installed from such a point, [6] reserved (0), [7] device time of the kernel and of the lift
 * behind it in microseconds.  All 0 on a tree without the option.
 */
int mipx_tree_weighted_repair_stats(mipx_tree *t, int64_t out[8]);

#ifdef __cplusplus
}
#endif
#endif /* MIPX_WREPAIR_H */
