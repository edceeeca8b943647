/*
 * mipx_lsearch.h -- a pair-move local search on the GPU behind the primal heuristic (included by mipx.h).
 *
 * The heuristic of mipx_heur.h ends at a point no unit move of one column improves.  This search goes on from such
 * a point with moves of one column or of two columns at once, one workgroup per point.  The engine can run it on
 * the feasible points of the heuristic of its steps (mipx_tree_set_local_search), or a caller on points of their
 * own (mipx_pair_search_batch).
 *
 * For one point x of the problem's rows A x >= b (m x n), objective c, bounds l, u, the integer columns int_idx, a
 * tolerance tol >= 0 and a move cap max_moves >= 0:
 *
 * BOUNDS.     The rounded bounds of an integer column are those of mipx_heur.h: ceil(l_j - tol) and floor(u_j + tol).
 * CHECK.      s_i = a_i . x - b_i (columns ascending, from +0, products not fused).  If some s_i < -tol, or an
 *             integer column is not integral (x_j != floor(x_j)) or lies outside its rounded bounds, the status is
 *             NOT_FEASIBLE and x comes back as it went in.
 * CANDIDATES. Both kinds move integer columns by d = +1 or -1 and stay inside the rounded bounds.
 *             A single (j, d):  g = c_j d < 0, and s_i + d a_ij >= -tol in every row.
 *             A pair (j, dj), (k, dk) with j < k by column index:  g = (c_j dj) + (c_k dk) < 0, and
 *             (s_i + dj a_ij) + dk a_ik >= -tol in every row, evaluated in exactly that order.
 * MOVE.       The candidate with the smallest key (g, j, k, dj, dk) is applied; a single has k = -1 and dk = 0, and
 *             +1 sorts before -1.  No two candidates have the same key.  x_j += dj, x_k += dk, and
 *             s_i = (s_i + dj a_ij) + dk a_ik (a single: s_i = s_i + dj a_ij).
 * STOP.       No candidate: LOCAL_OPT.  max_moves moves made and a candidate remains: CAPPED.
 * OUTPUT.     The point; obj = sum of c_j x_j (columns ascending, from +0); the status; the number of single moves
 *             and of pair moves.  A skipped point (status SKIPPED) returns x unchanged, obj 0 and no moves.
 *
 * Every sum is one add per term in the stated order and nothing is fused, so a restatement in the same order gives
 * the same bits on any data (tests/support/local_search_reference.py).  Every move lowers c . x and keeps the point
 * feasible to tol, so the search ends.
 *
 * COST.  The search for one move walks every integer column j against every integer column k > j: it reads A about
 * n_int times (less where the cost test or the rows leave no pair alive).  At 256 x 128 that is 256 KiB per column
 * j, which stays in L2; at 1024 x 1024 it is up to 8 GiB of traffic per move, which is slow.  Cap the moves there
 * (the engine's default cap is 64).
 */
#ifndef MIPX_LSEARCH_H
#define MIPX_LSEARCH_H

#ifdef __cplusplus
extern "C" {
#endif

#define MIPX_LS_LOCAL_OPT 0
#define MIPX_LS_CAPPED 1
#define MIPX_LS_NOT_FEASIBLE 2
#define MIPX_LS_SKIPPED 3

/*
 * Host buffers, one launch.  x: batch x n points; l, u: n each; int_idx: n_int distinct columns; skip: null, or
 * batch bytes (non-zero: the point is skipped).  x_out: batch x n (it may be x); obj_out, status_out: batch;
 * moves_out: 2 per point (singles, pairs).  MIPX_EINVAL: a null or out-of-range argument, tol < 0, max_moves < 0;
 * MIPX_ETOOBIG: m or n above 1024.
 */
int mipx_pair_search_batch(mipx_problem *p, int batch, const double *x, const double *l, const double *u,
                           const int32_t *int_idx, int n_int, double tol, int max_moves, const uint8_t *skip,
                           double *x_out, double *obj_out, int32_t *status_out, int32_t *moves_out);
/*
 * Run the search inside the tree search: right behind the heuristic of a step, in place on the points the
 * heuristic ended feasible on (the others are skipped), with the root's bounds, the heuristic's tol and the move
 * cap max_moves (the Python layer's default: 64).  The objective of every point it runs on is written again, as the
 * same ordered sum over the point it leaves, moved or not.  The step's best point is then chosen as before, from
 * the improved objectives.  max_moves = 0 turns it off again.  Set after mipx_tree_set_heuristic and before the
 * first step.  MIPX_EINVAL: max_moves < 0, a tree without the heuristic, a tree that has stepped.
 */
int mipx_tree_set_local_search(mipx_tree *t, int max_moves);
/*
 * [0] points run: every point the heuristic ended feasible on (the search's own check passes them: it takes the same
 * sums with the same tol; one it did call NOT_FEASIBLE would still count here), [1] of those, improved (at least
 * one move), [2] single moves, [3] pair moves, [4] points capped, [5] incumbents installed from an improved point,
 * [6] reserved (0), [7] device time of the kernel in microseconds.  All 0 on a tree without the search.
 */
int mipx_tree_local_search_stats(mipx_tree *t, int64_t out[8]);

#ifdef __cplusplus
}
#endif
#endif /* MIPX_LSEARCH_H */
