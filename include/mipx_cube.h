/*
 * mipx_cube.h -- a cube search on the GPU: every rounding of an LP point's fractional columns (included by mipx.h).
 *
 * The heuristics of mipx_heur.h, mipx_lsearch.h, mipx_fixprop.h and mipx_wrepair.h walk by unit moves of one or two
 * columns or by sequential fixing, and end in shallow local optima.  An LP point of the search has far fewer
 * fractional integer columns than rows (9 to 20 on the generator's instances up to 144 columns); with every other
 * column held where the rounding puts it, the 2^k ways to round the k fractional ones up or down are few enough to
 * try them all.  The engine can run this on the LP points its rounding heuristic takes (mipx_tree_set_cube_search)
 * or a caller on points of their own (mipx_cube_search_batch).
 *
 * For one point x of the problem's rows A x >= b (m x n), objective c, bounds l, u (the root's), the integer
 * columns int_idx, tolerances tol >= 0 and ftol >= 0, a column cap 1 <= K <= 20 and a cutoff U (+inf for none):
 *
 * ROUNDED BOUNDS.  lr_j = ceil(l_j - tol), ur_j = floor(u_j + tol), as in mipx_heur.h.
 * SELECT.  An integer column j is a candidate when f_j = |x_j - floor(x_j + 0.5)| > ftol and
 *          lr_j <= floor(x_j) and floor(x_j) + 1 <= ur_j.  F holds the min(K, number of candidates) candidates with
 *          the largest f_j; ties go to the lower column index.  F is listed in ascending column order,
 *          F_0 < ... < F_{k-1}; k may be 0.
 * BASE.    x~_j = floor(x_j) for j in F; every other integer column takes the ROUND of mipx_heur.h,
 *          min(max(floor(x_j + 0.5), lr_j), ur_j); the other columns keep x_j (a rounded zero is +0).
 *          s_i = a_i . x~ - b_i (columns ascending, from +0, products not fused); obj0 = sum of c_j x~_j (columns
 *          ascending, from +0).
 * CODES.   For e in [0, 2^k), bit t of e raises column F_t by one: s_i(e) = s_i plus a_{i,F_t} for every set bit,
 *          t ascending, one add per term; obj(e) = obj0 plus c_{F_t} for every set bit, t ascending.  e is feasible
 *          when s_i(e) >= -tol in every row, and improving when obj(e) < U.
 * PICK.    The feasible, improving code with the smallest key (obj(e), e).
 * OUTPUT.  FOUND (0) returns x~ with the picked bits applied (x~_{F_t} + 1 where bit t is set), obj(e), and the two
 *          counts k and e.  NONE (1) returns x unchanged, obj 0, and the counts k and -1.  SKIPPED (3) returns x
 *          unchanged, obj 0, and the counts 0 and -1.
 *
 * VALIDITY.  A FOUND point satisfies every row within tol, is integral in the integer columns, inside the rounded
 *          bounds, and unchanged in the other columns; its objective is below U; no point of the cube has a smaller
 *          key.  NONE says that the cube holds no feasible point below U, nothing about the problem.
 * ARITHMETIC.  Products are not fused and every sum is one add per term in the stated order.  A kernel that walks
 *          the codes incrementally (Gray code) would not reproduce these sums on non-integer data, so each code's
 *          sums are formed as stated, from s_i and obj0.  A restatement in that order gives the same bits
 *          (tests/support/cube_search_reference.py).
 */
#ifndef MIPX_CUBE_H
#define MIPX_CUBE_H

#ifdef __cplusplus
extern "C" {
#endif

#define MIPX_CUBE_FOUND 0
#define MIPX_CUBE_NONE 1
#define MIPX_CUBE_SKIPPED 3

#define MIPX_CUBE_MAX_COLUMNS 20

/*
 * Host buffers, one call.  x: batch x n points; l, u: n each; int_idx: n_int distinct columns; cutoff: U, +inf for
 * none; skip: null, or batch bytes (non-zero: the point is skipped).  x_out: batch x n; obj_out, status_out: batch;
 * counts_out: 2 per point (k, code).
 * MIPX_EINVAL: a null or out-of-range argument, tol < 0, ftol < 0, a NaN cutoff, max_columns outside 1..20, int_idx
 * out of range or repeated, an l that is not finite, a u that is NaN or -inf, an x that is not finite (as
 * mipx_weighted_repair_batch); MIPX_ETOOBIG: m or n above 1024.  A batch of 0 is no launch; the batch has no
 * limit of its own (above 65535 points the enumeration is split into several launches, to the same result).
 */
int mipx_cube_search_batch(mipx_problem *p, int batch, const double *x, const double *l, const double *u,
                           const int32_t *int_idx, int n_int, double cutoff, double tol, double ftol, int max_columns,
                           const uint8_t *skip, double *x_out, double *obj_out, int32_t *status_out,
                           int32_t *counts_out);
/*
 * Run the cube search inside the search, in every step the primal heuristic runs in and on the same LP points (the
 * step's first nodes whose LP ended optimal), whatever the rounding made of them: with the root's bounds, the
 * heuristic's tol, the engine's integrality tolerance as ftol, max_columns as K and the tree's cutoff at launch as
 * U.  A FOUND point lives in a block of its own, goes through the heuristic once more, which lifts it, and with
 * mipx_tree_set_local_search through the pair search; it then competes for the step's incumbent beside the
 * heuristic's points and those of the dive or the weighted repair (a tie goes to the earlier family, then to the
 * lowest position).  Set before the first step.
 * MIPX_EINVAL: max_columns outside 0..20, a tree without the heuristic (mipx_tree_set_heuristic first, which refuses
 * cut rounds and a communicator), a tree that has stepped.  max_columns = 0 switches it off again.  A later
 * mipx_tree_set_heuristic with more points than this was set for is refused, as with the weighted repair.
 */
int mipx_tree_set_cube_search(mipx_tree *t, int max_columns);
/*
 * [0] points tried (not skipped), [1] of those, ended FOUND, [2] ended NONE, [3] sum of k, [4] points whose k hit
 * the cap, [5] incumbents installed from a cube point, [6] reserved (0), [7] device time of the kernels and of the
 * lift behind them in microseconds.  All 0 on a tree without the option.
 */
int mipx_tree_cube_search_stats(mipx_tree *t, int64_t out[8]);

#ifdef __cplusplus
}
#endif
#endif /* MIPX_CUBE_H */
