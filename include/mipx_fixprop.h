/*
 * mipx_fixprop.h -- a second primal heuristic on the GPU: a fix-and-propagate dive (included by mipx.h).
 *
 * The rounding heuristic of mipx_heur.h repairs a rounded LP point by unit moves and stops (STUCK) where no single
 * move lowers the total violation, which happens on rows that pack and rows that cover side by side.  The dive
 * needs no LP either and works the other way round: it fixes one integer column after the other to a value near
 * the LP point and lets the bound propagation of mipx_prop.h tighten the others, so that a fixing the rows cannot
 * follow shows at once and the next value is tried.  One workgroup per point; the engine can run it on the points
 * its rounding heuristic left infeasible (mipx_tree_set_fix_propagate) or a caller on points of their own
 * (mipx_fix_propagate_batch).
 *
 * For one point x of the problem's rows A x >= b (m x n), objective c, bounds l, u (the root's; l finite, u
 * possibly +inf), the integer columns int_idx, a tolerance tol >= 0, a cutoff (+inf or -inf: none), max_rounds >= 1
 * propagation rounds per propagation call and max_tries >= 0 propagation calls for the values of the point:
 *
 * PROPAGATE.  A box (L, U) through the rounds of mipx_prop.h exactly as stated there (ONE ROUND to STOP), with this
 *          tol, max_rounds and the cutoff row when the cutoff is finite.  It ends infeasible, or with the
 *          tightened box.
 * START.   L = l, U = u, for an integer column j the heuristic's rounded bounds L_j = ceil(l_j - tol),
 *          U_j = floor(u_j + tol) (a zero is +0).  PROPAGATE this box: infeasible gives INFEASIBLE_BOX.
 * PICK.    Among the integer columns with L_j < U_j the one with the smallest key (|x^_j - rint(x^_j)|, j), where
 *          x^_j = min(max(x_j, L_j), U_j) and rint rounds halves to even.  None left: END.
 * VALUES.  The integers w of [L_j, U_j] in ascending (|w - x^_j|, w): below x^_j they are floor(x^_j),
 *          floor(x^_j) - 1, ..., above it floor(x^_j) + 1, ...; the next below is taken when its distance
 *          x^_j - w is not larger than the next above's w - x^_j, or when none is left above.  For each w: with
 *          max_tries tries made the point is CAPPED; else one try is counted and the box with L_j = U_j = w is
 *          PROPAGATEd.  The first w that does not end infeasible is the fixing: its tightened box replaces (L, U),
 *          one fixing is counted, back to PICK.  No w left: the point is STUCK.  (There is no backtracking: a
 *          fixing once made stays.)
 * END.     x~_j = L_j for the integer columns, min(max(x_j, L_j), U_j) for the others (their bounds are the
 *          root's: the propagation moves integer columns only).  s_i = a_i . x~ - b_i (columns ascending, from
 *          +0).  Every s_i >= -tol: FEASIBLE.  Otherwise ROWS: the propagation had every row's largest activity
 *          at b_i - tol or above when it last looked, so this needs continuous columns (their best value is not
 *          the clamped x_j), a last propagation that max_rounds ended while it still changed bounds, or a sum that
 *          rounds differently in the propagation's order.
 * OUTPUT.  FEASIBLE and ROWS return x~ and obj = sum of c_j x~_j (columns ascending, from +0); every other status
 *          returns x unchanged and obj 0.  With them the status, the number of fixings and the number of tries.  A
 *          skipped point returns x unchanged, obj 0, SKIPPED and no counts, as the heuristic returns it.
 *
 * VALIDITY.  A FEASIBLE point satisfies every row within tol, is integral in the integer columns and inside the
 *          bounds; with a finite cutoff its objective is at most cutoff + tol when all columns are integer.
 *          INFEASIBLE_BOX is given only when the box holds no integer point with c . x <= cutoff.
 * ARITHMETIC.  Products are not fused.  Each propagation is the Jacobi round of mipx_prop.h, so the result does not
 *          depend on how the work is split; its row sums S_i run in the kernel's own order (lanes stride the
 *          columns, then a butterfly over the wave), which gives the same bits as any other on integer data.  The
 *          keys of PICK and VALUES, the clamps, s_i and obj are each one operation per term in the stated order,
 *          and a restatement in that order gives the same bits (tests/support/fix_propagate_reference.py).
 */
#ifndef MIPX_FIXPROP_H
#define MIPX_FIXPROP_H

#ifdef __cplusplus
extern "C" {
#endif

#define MIPX_FP_FEASIBLE 0
#define MIPX_FP_STUCK 1
#define MIPX_FP_CAPPED 2
#define MIPX_FP_SKIPPED 3
#define MIPX_FP_INFEASIBLE_BOX 4
#define MIPX_FP_ROWS 5

/*
 * Host buffers, one launch.  x: batch x n points; l, u: n each; int_idx: n_int distinct columns; cutoff: +inf or
 * -inf for no cutoff row; skip: null, or batch bytes (non-zero: the point is skipped).  x_out: batch x n; obj_out,
 * status_out: batch; counts_out: 2 per point (fixings, tries).
 * MIPX_EINVAL: a null or out-of-range argument, tol < 0, max_rounds < 1, max_tries < 0, a NaN cutoff, int_idx out
 * of range or repeated, an l that is not finite, a u that is NaN or -inf, an x that is not finite;
 * MIPX_ETOOBIG: m or n above 1024.
 */
int mipx_fix_propagate_batch(mipx_problem *p, int batch, const double *x, const double *l, const double *u,
                             const int32_t *int_idx, int n_int, double cutoff, double tol, int max_rounds,
                             int max_tries, const uint8_t *skip, double *x_out, double *obj_out, int32_t *status_out,
                             int32_t *counts_out);
/*
 * Run the dive inside the search, behind the primal heuristic of every step it runs in: on the same LP points, but
 * only those the rounding ended STUCK or CAPPED on, with the root's bounds, the heuristic's tol, the cutoff the
 * host holds at the launch (the incumbent, one objective step lower with mipx_tree_set_objective_step; none yet: no
 * cutoff row), max_rounds rounds per propagation and max_tries tries per point.  A point the dive ends FEASIBLE
 * takes the place of the heuristic's and goes through the heuristic once more, which lifts it (rounding an
 * integral point changes nothing and its repair is empty), and with mipx_tree_set_local_search through the pair
 * search; it then competes for the step's incumbent like the heuristic's own points.  Set before the first step.
 * MIPX_EINVAL: max_rounds < 1, max_tries < 0, a tree without the heuristic (mipx_tree_set_heuristic first, which
 * refuses cut rounds and a communicator), a tree that has stepped.  max_tries = 0 switches the dive off again.
 * A later mipx_tree_set_heuristic with more points than the dive was set for is refused, as with the local search.
 * A tree that has the weighted row repair of mipx_wrepair.h on is refused as well (MIPX_EINVAL): one of the two.
 */
int mipx_tree_set_fix_propagate(mipx_tree *t, int max_rounds, int max_tries);
/*
 * [0] points tried (not skipped), [1] of those, ended feasible, [2] stuck, [3] capped, [4] fixings, [5] tries,
 * [6] incumbents installed from a dive point, [7] device time of the dive and of the lift behind it in
 * microseconds.  All 0 on a tree without the dive.
 */
int mipx_tree_fix_propagate_stats(mipx_tree *t, int64_t out[8]);

#ifdef __cplusplus
}
#endif
#endif /* MIPX_FIXPROP_H */
