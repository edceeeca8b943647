/*
 * mipx_lpdive.h -- LP diving: fix one integer column, re-solve the batch, repeat (included by mipx.h).
 *
 * The heuristics of mipx_heur.h, mipx_lsearch.h, mipx_fixprop.h, mipx_wrepair.h and mipx_cube.h move integer columns
 * without an LP; mipx_complete.h solves one LP after every integer column has been fixed at once.  On a model with
 * continuous columns that last LP is often infeasible where fixing the integers one by one, with the LP re-solved in
 * between so that the continuous columns and the integers still free adapt, ends on a point.  That is the LP dive.
 * Every round of P dives is ONE warm-started launch of the node-LP kernels over P boxes.  (The `dive` of the search is
 * the in-place plunge of the node-LP kernel, mipx_lp_dive_batch; mipx_fixprop.h is the dive without an LP.)  The engine
 * can run it on the LP points of a step's first nodes (mipx_tree_set_lpdive) or a caller on points of their own
 * (mipx_lpdive_batch).
 *
 * INPUTS, for one point: the problem's rows A x >= b (m x n) and objective c; the integer columns int_idx; a box
 * L0 <= x <= U0 (the node's bounds in the search, the caller's or the root's in the batch entry); a point x0 that is
 * the optimum of the LP over that box; optionally the basis codes of that LP (all 0, or none: no basis); a cutoff
 * (+inf: none); a round cap R >= 1; ftol = ctol = 1e-6.
 *
 * STATE per point: the current box (L, U); the last optimal LP point x and its basis codes; the last fixing
 * (j, old L_j, old U_j, v, x_j), or none; a phase: ACTIVE, FINAL, or ended.
 *
 * PREPARE.  A point is SKIPPED when its skip byte is set, when x0 is not finite, or when an integer column has a bound
 *           b with |b - rint(b)| > ctol or an infinite one.  Otherwise L = L0 and U = U0 with the bounds of the integer
 *           columns replaced by rint of themselves (so every value a column is fixed at below is an integer), x = x0,
 *           the codes are the caller's or all 0, no fixing is on record and the phase is ACTIVE.
 * ROUNDS.   Round r = 1 .. R is STEP, then one LP over every point's (L, U) from its codes; behind round R a last
 *           STEP (r = R + 1) reads the last LP.
 * STEP.     Round 1 goes straight to 3 with x0.  A later round reads its point's LP of the round before: status,
 *           objective, point, codes, pivots (added to the point's pivot count).
 *           1. The LP ended optimal: its x and codes become current.  An objective that is not below the cutoff
 *              ends the point CUTOFF.  In phase FINAL the point goes to FINISH.
 *           2. The LP did not end optimal.  Iteration limit or unbounded: the point ends LIMIT.  Infeasible with no
 *              fixing on record: INFEASIBLE.  Infeasible with one, and r <= R: FLIP -- for v <= x_j the column gets
 *              [v + 1, old U_j], otherwise [old L_j, v - 1]; the record is cleared; an empty range ends the point
 *              INFEASIBLE; nothing else changes, and the next LP starts from the last optimal codes, which stay dual
 *              feasible because only bounds moved.
 *           3. Otherwise, and r <= R: SELECT.  frac_j = |x_j - rint(x_j)|.  Candidates are the integer columns with
 *              L_j < U_j and frac_j > ftol.
 *              No candidate: every free integer column is fixed at floor(x_j + 0.5) clipped to [L_j, U_j], the phase
 *              becomes FINAL and the next LP is the completion's LP.
 *              Rule 0 (fractional): the candidate of smallest frac_j, ties to the earlier position in int_idx;
 *              v = floor(x_j + 0.5).
 *              Rule 1 (coefficient): down_j = the number of rows with a_ij > 0 (those lowering x_j can break), up_j
 *              the number with a_ij < 0; the candidate of smallest min(down_j, up_j), ties by rule 0's order;
 *              v = floor(x_j) if down_j < up_j, ceil(x_j) if up_j < down_j, floor(x_j + 0.5) on a tie.
 *              v is clipped to [L_j, U_j]; L_j = U_j = v and (j, old L_j, old U_j, v, x_j) is the record.
 *           4. A point that would need the LP of round R + 1 (still ACTIVE, or in need of a flip) ends LIMIT.
 *           5. A point that ends, or goes to FINISH, has every column fixed at L0 and its codes zeroed: its remaining
 *              LPs end without a pivot, as those of the completion's SKIPPED points do, and are not counted.
 * FINISH.   mipx_complete.h's FINISH on the FINAL LP's point, with ctol and the box (L0, U0): the integer columns are
 *           exactly the fixed integers, every row and the objective are recomputed in the order stated there; the
 *           point is FEASIBLE when every row and bound holds within ctol and REJECTED otherwise.
 * STATUS.   FEASIBLE 0, INFEASIBLE 1, LIMIT 2, SKIPPED 3, REJECTED 4, CUTOFF 5.  0 and 3 are the heuristic's feasible
 *           and skipped, as in the other families.
 * OUTPUT.   The point (x0 where the dive is not FEASIBLE), its objective (0 where it is not), the status, the rounds
 *           (LPs solved for the point while it had not ended), the fixings (those of SELECT; FINAL's are not counted),
 *           the flips, and the LP pivots summed over those rounds (the warm start's refactorisation included).
 *
 * VALIDITY.  A FEASIBLE point satisfies every row and bound of its box within ctol, is integral in the integer
 *           columns, and its objective is the LP's optimum for those integers, below the cutoff.  The other statuses
 *           say nothing about the problem: the dive is a heuristic, and one flip is all its backtracking.
 * ARITHMETIC.  Every LP is the node-LP kernel's, bit for bit what mipx_lp_solve_batch gives on (L, U) and the codes.
 *           STEP compares and copies; its arithmetic is rint, floor, ceil, one subtraction and v +- 1.  A restatement
 *           around that LP gives the same bits (tests/support/lp_dive_reference.py).
 * NO HOST WAIT.  Inside a search PREPARE, R x (STEP, LP) and the last STEP with FINISH are queued without a host
 *           read; an ended point costs one trivial workgroup per round.  Every LP launch carries codes, so none takes
 *           the path of the single cold LP (see mipx_complete.h).  The batch entry reads a counter of live points
 *           between rounds and stops launching when it is 0; the outputs do not depend on that.
 */
#ifndef MIPX_LPDIVE_H
#define MIPX_LPDIVE_H

#ifdef __cplusplus
extern "C" {
#endif

#define MIPX_LPDIVE_FEASIBLE 0
#define MIPX_LPDIVE_INFEASIBLE 1
#define MIPX_LPDIVE_LIMIT 2
#define MIPX_LPDIVE_SKIPPED 3
#define MIPX_LPDIVE_REJECTED 4
#define MIPX_LPDIVE_CUTOFF 5

#define MIPX_LPDIVE_RULE_FRACTIONAL 0
#define MIPX_LPDIVE_RULE_COEFFICIENT 1
#define MIPX_LPDIVE_MAX_ROUNDS 1024

/*
 * Host buffers, one call.  x: batch x n points; l, u: batch x n boxes; int_idx: n_int distinct columns (n_int == n is
 * legal); vstat: null (no basis), or batch x (n + m) basis codes in the layout of mipx_lp_solve_batch; skip: null, or
 * batch bytes (non-zero: the point is skipped).  x_out: batch x n; obj_out, status_out, rounds_out, fixings_out,
 * flips_out, pivots_out: batch.
 * MIPX_EINVAL: a null or out-of-range argument, int_idx out of range or repeated, an l that is not finite (the LP
 * kernels' form), a u that is NaN or -inf, max_rounds outside 1..1024, a rule other than 0 or 1, a NaN cutoff;
 * MIPX_ETOOBIG: m or n above 1024.  A batch of 0 is no launch.  (A point that is not finite, or an integer column
 * whose bounds are not integers, makes its point SKIPPED, not the call fail: the boxes are per point.)
 */
int mipx_lpdive_batch(mipx_problem *p, int batch, const double *x, const double *l, const double *u,
                      const int32_t *int_idx, int n_int, const int8_t *vstat, const uint8_t *skip,
                      double cutoff, int max_rounds, int rule,
                      double *x_out, double *obj_out, int32_t *status_out,
                      int32_t *rounds_out, int32_t *fixings_out, int32_t *flips_out, int32_t *pivots_out);
/*
 * Run the dive inside the search, in a step the primal heuristic runs in, when the host holds no incumbent at that
 * step's launch, or when every > 0 and the step index is a multiple of every (every = 0: only without an incumbent).
 * The points are the heuristic's, the LP points of the step's first nodes, each inside its node's bounds as the pool
 * row holds them at the launch and warm from that node LP's final codes; a node whose LP did not end optimal is
 * skipped.  The cutoff is the search's at the launch.  A FEASIBLE point competes for the step's incumbent as a family
 * of its own behind the others: a tie goes to the earlier family, then to the lowest position.  It is not passed to
 * the lift or the local search.  max_rounds = 0 switches the option off again.  Set before the first step.  With the
 * option on, every step is finished on the host, as with the heuristic.
 * MIPX_EINVAL: max_rounds outside 0..1024, every < 0, a rule other than 0 or 1, a tree without the heuristic
 * (mipx_tree_set_heuristic first, which refuses cut rounds and a communicator), a tree that has stepped.  A later
 * mipx_tree_set_heuristic with more points than this was set for is refused, as with the completion.
 */
int mipx_tree_set_lpdive(mipx_tree *t, int max_rounds, int every, int rule);
/*
 * [0] points tried (not skipped), [1] of those, ended FEASIBLE, [2] INFEASIBLE or CUTOFF, [3] LIMIT or REJECTED,
 * [4] fixings + flips, [5] incumbents installed from a dive point, [6] LP pivots, [7] device time of the dive's
 * kernels and LP launches in microseconds.  All 0 on a tree without the option.
 */
int mipx_tree_lpdive_stats(mipx_tree *t, int64_t out[8]);

#ifdef __cplusplus
}
#endif
#endif /* MIPX_LPDIVE_H */
