/*
 * mipx_cglp_screen.h -- support sessions that keep their duals: the dual screen of the leaves, and the cold retry
 * (included by mipx.h behind mipx_cglp.h, whose sessions and output block these entries extend).
 *
 * THE BOUND.  For a leaf t with box (l, u), rows A x >= b and any y >= 0, with r = pi - A'y,
 *
 *     L_t(pi; y) = y.b + sum_j min(r_j l_j, r_j u_j)  <=  h_t(pi) = min {pi.x : A x >= b, l <= x <= u}
 *
 * (weak duality: pi.x = y.(A x) + r.x >= y.b + r.x for every x of the leaf).  A session opened with
 * MIPX_SUPPORT_KEEP_DUALS keeps, per leaf, the row duals y that the leaf's last OPTIMAL LP of a screening evaluation
 * wrote (the y output of the node-LP kernels), and uses y+ = max(y, 0) componentwise.  Any y+ >= 0 gives a valid
 * bound, so duals on record never go stale; at the pi they were computed for the bound equals h_t up to rounding.
 *
 * THE ARITHMETIC is fixed, so that a plain restatement gives the same bits (tests/support/cglp_screen_reference.py):
 *   y+_i = y_i if y_i > 0, else 0 (a NaN reads as 0);
 *   per column j:  s_j = 0, then s_j = fma(A_ij, y+_i, s_j) over the rows i in ascending order with y+_i > 0;
 *                  r_j = pi_j - s_j;  p1 = r_j l_j, p2 = r_j u_j;  term_j = p2 if p2 < p1, else p1;
 *   over columns:  64 partial sums, sum q adding (from 0) the terms of the columns q, q + 64, q + 128, ... in
 *                  ascending order; then six rounds v_q = v_q + v_(q xor off), off = 32, 16, 8, 4, 2, 1, on all 64 at
 *                  once; every entry then holds the same bits: the columns' sum;
 *   over rows:     the same with the products y+_i b_i (product, then sum; nothing is fused) in the place of the terms;
 *   L_t = columns' sum + rows' sum.
 *
 * A leaf is SCREENED in an evaluation iff it has duals on record, L_t is finite, and L_t - pi0 >= -screen_tol.  A
 * screened leaf gets no LP: its margin is L_t - pi0, a lower bound on its true margin; its basis, x and duals stay as
 * they were; its iterations and pivots in this evaluation are 0.  The minimum margin in the block's head runs over
 * screened and solved leaves alike, so pi0 + the minimum margin remains a certified right-hand side.  A SCREENED LEAF
 * THAT APPEARS AMONG THE ROWS of the block carries its bound in the place of h_t and the x of its last LP, which is no
 * minimiser for this pi: a caller that builds on rows must leave alone every row whose h_t - pi0 is at or above -tol
 * (with screen_tol <= tol every screened leaf is such a row).
 *
 * The unscreened leaves are packed in ascending order of their position in the session (a block scan and the
 * segments' counts: the order does not depend on how the launch was scheduled), their bounds and bases gathered into
 * launch buffers, solved by the unchanged node-LP launch, and scattered back.
 */
#ifndef MIPX_CGLP_SCREEN_H
#define MIPX_CGLP_SCREEN_H

#ifdef __cplusplus
extern "C" {
#endif

#define MIPX_SUPPORT_KEEP_DUALS 1   /* flags bit 0 of mipx_tree_support_open_ex */

/*
 * mipx_tree_support_open with flags; flags = 0 is mipx_tree_support_open.  MIPX_SUPPORT_KEEP_DUALS adds, per leaf,
 * m doubles of duals and the launch buffers of a packed subset (another 3 n + m + 1 doubles, 2 (n + m) bytes of basis
 * codes and 26 bytes of words), all counted in the session's device bytes.  MIPX_EINVAL: an unknown flag, and what
 * mipx_tree_support_open refuses.
 */
int mipx_tree_support_open_ex(mipx_tree *t, const int64_t *ids, int64_t K, int flags, mipx_support **out);
/*
 * mipx_tree_support_eval with the screen and the retry.  The block keeps its layout (mipx_cglp.h).
 *   screen_tol < 0     no screening: needs no flag, records no duals, and with retry_cold = 0 is
 *                      mipx_tree_support_eval bit for bit.
 *   screen_tol >= 0    needs MIPX_SUPPORT_KEEP_DUALS (else MIPX_EINVAL; MIPX_ETOOBIG above 1024 rows or columns).
 *                      The session's first evaluation solves every leaf and records its duals; later ones screen
 *                      first.  One small read (16 bytes: the packed count) comes down between the screen and the launch.
 *   retry_cold != 0    needs the flag too, with or without screening: the leaves whose LP did not end optimal are
 *                      packed, solved once more without a basis, and scattered back; block word [4] counts what is
 *                      still not optimal; iterations and pivots of both attempts count.
 * extra (null, or 6 doubles): [0] leaves screened, [1] leaves LP-solved ([0] + [1] = the session's leaves),
 * [2] the smallest screened margin (+inf if none), [3] leaves retried cold, [4] of those, ended optimal,
 * [5] device microseconds of screen + pack + gather + scatter (the retry's included).
 */
int mipx_tree_support_eval_ex(mipx_support *s, const double *pi, double pi0, double tol, double screen_tol, int retry_cold,
                              int max_points, double *block, double *margins, double *extra);
/*
 * TEST SCAFFOLDING in the library, as mipx_finish.h and mipx_cutround.h are: no product code calls this entry.
 * support_screen and the two pack kernels on a caller's data (host pointers), through the launch the session uses:
 * pi (n), l and u (T x n), y (T x m), has_y (T bytes: duals on record) against the rows A x >= b of p.  Out: bound_out
 * (T doubles: L_t, -inf without duals), screened_out (T bytes), packed_out (T int32: the positions of the unscreened
 * leaves in ascending order, then -1) and count_out (their number).  MIPX_EINVAL: a null argument, T < 0 or above
 * 2^30, screen_tol negative or NaN, pi0 NaN;  MIPX_ETOOBIG: m or n above 1024.  T = 0 is no launch.
 */
int mipx_support_screen_batch(mipx_problem *p, int64_t T, const double *pi, double pi0, double screen_tol, const double *l,
                              const double *u, const double *y, const uint8_t *has_y, double *bound_out,
                              uint8_t *screened_out, int32_t *packed_out, int32_t *count_out);

#ifdef __cplusplus
}
#endif
#endif /* MIPX_CGLP_SCREEN_H */
