/*
 * mipx_heur.h -- a primal heuristic on the GPU: round an LP point, repair it, lift it (included by mipx.h).
 *
 * The frontier engine finds an incumbent only where a node LP ends integral.  This heuristic makes integral
 * points out of LP points, one workgroup per point, and the engine can run it on the node LP solutions of its
 * steps (mipx_tree_set_heuristic) or a caller on points of their own (mipx_round_repair_batch).
 *
 * For one point x of the problem's rows A x >= b (m x n), objective c, bounds l, u (the root's), the integer
 * columns int_idx, a tolerance tol >= 0 and a move cap max_moves >= 0:
 *
 * ROUND.   For an integer column j: x~_j = min(max(floor(x_j + 0.5), ceil(l_j - tol)), floor(u_j + tol)); the
 *          other columns keep x_j (a rounded zero is +0).  s_i = a_i . x~ - b_i (columns ascending, from +0).
 * REPAIR.  While some s_i < -tol and fewer than max_moves moves have been made: V is the sum of -s_i over the
 *          rows with s_i < -tol (rows ascending).  A candidate is an integer column j and a step d = +1 or -1
 *          with x~_j + d inside the rounded bounds; its V' is the same sum over s_i + d a_ij.  The candidate with
 *          the smallest key (V', c_j d, j, +1 before -1) is taken if its V' < V: x~_j += d, s_i += d a_ij.  With
 *          no such candidate the point is STUCK; with the cap reached while a row is violated it is CAPPED.
 * LIFT.    Only from a point whose repair ended with every row satisfied, and while fewer than max_moves moves
 *          have been made in all: candidates are (j, d) inside the rounded bounds with c_j d < 0 and
 *          s_i + d a_ij >= -tol in every row; the smallest key (c_j d, j, +1 before -1) is applied; it stops
 *          when there is no candidate.
 * OUTPUT.  x~; obj = sum of c_j x~_j (columns ascending); a status (0 feasible: every row within tol, every
 *          integer column integral and inside its rounded bounds; 1 stuck; 2 capped; 3 skipped); the number
 *          of repair moves and of lift moves.  A skipped point returns x unchanged, obj 0 and no moves.
 *
 * Every sum is one add per term in the stated order, products are not fused: on integer data the result is
 * exact, and a restatement in the same order gives the same bits (tests/support/heuristic_reference.py).
 */
#ifndef MIPX_HEUR_H
#define MIPX_HEUR_H

#ifdef __cplusplus
extern "C" {
#endif

#define MIPX_HEUR_FEASIBLE 0
#define MIPX_HEUR_STUCK 1
#define MIPX_HEUR_CAPPED 2
#define MIPX_HEUR_SKIPPED 3

/*
 * Host buffers, one launch.  x: batch x n points; l, u: n each; int_idx: n_int distinct columns; skip: null, or
 * batch bytes (non-zero: the point is skipped).  x_out: batch x n; obj_out, status_out: batch; moves_out: 2 per
 * point (repair, lift).  MIPX_EINVAL: a null or out-of-range argument, tol < 0, max_moves < 0;
 * MIPX_ETOOBIG: m or n above 1024.
 */
int mipx_round_repair_batch(mipx_problem *p, int batch, const double *x, const double *l, const double *u,
                            const int32_t *int_idx, int n_int, double tol, int max_moves, const uint8_t *skip,
                            double *x_out, double *obj_out, int32_t *status_out, int32_t *moves_out);
/*
 * Run the heuristic inside the search: every every_steps-th step, behind that step's node LPs, on the LP
 * solutions of the first min(batch, points_per_step) nodes of the step (those whose LP ended optimal; the others
 * are skipped), with the root's bounds, tol = 1e-9 and the move cap max_moves.  The best feasible point of a
 * step (ties: the lowest position) becomes the incumbent if it is strictly better than the one the tree holds,
 * before the step's own nodes are evaluated against it.  Every step is then finished on the host, as with
 * mipx_tree_set_dual_record and mipx_tree_set_tree_record.  Set before the first step.
 * MIPX_EINVAL: a non-positive argument, a tree with cut rounds or with a communicator, a tree that has stepped.
 * mipx_tree_set_comm refuses a tree that has the heuristic on.
 */
int mipx_tree_set_heuristic(mipx_tree *t, int points_per_step, int every_steps, int max_moves);
/*
 * [0] points tried (not skipped), [1] of those, ended feasible, [2] stuck, [3] capped, [4] repair moves,
 * [5] lift moves, [6] incumbents installed, [7] device time of the kernel in microseconds.  All 0 on a tree
 * without the heuristic.
 */
int mipx_tree_heuristic_stats(mipx_tree *t, int64_t out[8]);

#ifdef __cplusplus
}
#endif
#endif /* MIPX_HEUR_H */
