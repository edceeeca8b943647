/*
 * mipx_supportkernels.h -- the kernels behind a support evaluation, run on a caller's leaves (included by mipx.h
 * behind mipx_cglp_screen.h).
 *
 * TEST SCAFFOLDING in the library, as mipx_noderows.h and mipx_cutround.h are: no product code calls these entries.
 * A support session (mipx_cglp.h, mipx_cglp_screen.h) reaches support_select, support_select_merge
 * (csrc/cglp_kernels.hip.h), support_pack_count, support_pack, support_gather, support_scatter and support_mark
 * (csrc/cglp_screen_kernels.hip.h) only with what leaf LPs produce, and a leaf of a polytope does not fail on demand:
 * the failed-LP path of the scatter, the retry's packing by verdict, the second LP's added counts and the selection's
 * empty tails are out of a session's reach.  These entries run the kernels on synthetic leaves through the functions
 * the session launches them with (the enqueue_support_* functions of csrc/tree_engine.hip.h: the same kernels and
 * grids), so that every output bit can be compared with a plain restatement
 * (tests/support/support_kernels_reference.py, tests/test_support_kernels_gpu.py).  support_screen has its entry in
 * mipx_cglp_screen.h (mipx_support_screen_batch): it alone reads the rows of a problem.
 *
 * Every entry takes host buffers, uploads them, runs the kernels on the context's stream, copies back and frees.  An
 * array marked in and out is uploaded whole, then copied back whole whatever the kernels wrote, so that a caller's
 * sentinel bytes show what they left alone.  Everything a kernel indexes with is checked on the host before any launch:
 * a refused call (MIPX_EINVAL, with a message) launches nothing and leaves every array as it was.  T = 0 and count = 0
 * launch nothing and write nothing.  A SEGMENT is 2048 consecutive positions; G = ceil(T / 2048).
 *
 * What the kernels promise, pinned by the tests of these entries:
 *   - a leaf is OK iff its verdict is 0 and its objective is no NaN; its margin is obj - pi0, +inf if it is not OK; its
 *     key is (margin, node id); the rows of the block are the P smallest keys in ascending order, whatever the segments;
 *   - a failed LP (verdict != 0) leaves the leaf's duals and its has_y as they were, and overwrites x, codes, objective
 *     and verdict; a second LP of an evaluation (add != 0) adds its iterations and pivots to the leaf's;
 *   - the packed positions ascend, at any number of segments; min_margin runs over the skipped leaves alone.
 */
#ifndef MIPX_SUPPORTKERNELS_H
#define MIPX_SUPPORTKERNELS_H

#ifdef __cplusplus
extern "C" {
#endif

/*
 * support_select, then support_select_merge, on T leaves of n columns, P rows asked for.  In: ids (T int64), status,
 * iters, npivots (T int32), obj (T), x (T x n).  In and out: margin (T), cand_m (G x P doubles), cand_id, cand_t
 * (G x P int32), seg_sum (G x 4), block (8 + P (n + 2)).
 *   margin[t]      obj[t] - pi0, +inf if the leaf is not OK
 *   cand_*[g]      the P smallest keys of segment g in ascending order with their positions, then (+inf, 0x7fffffff, -1)
 *   seg_sum[g]     [OK leaves with margin < -tol, leaves not OK, sum of iters, sum of npivots] of segment g
 *   block          the head [min margin or +inf, its id or -1, below, nsel, not OK, iters, pivots, T] and nsel rows
 *                  [id, obj, x] (nsel = min(P, OK leaves)); the rows from nsel on are not written
 * MIPX_EINVAL: a null array; T < 0 or above 2^30; P outside 1 .. 1024; n < 1; tol negative or NaN; pi0 NaN; an id
 * outside 0 .. 2^31 - 2 (the kernels narrow ids to int, and 0x7fffffff means "no leaf").
 */
int mipx_support_select_batch(mipx_ctx *ctx, int64_t T, int n, int P, double pi0, double tol, const int64_t *ids,
                              const int32_t *status, const double *obj, const double *x, const int32_t *iters,
                              const int32_t *npivots, double *margin, double *cand_m, int32_t *cand_id, int32_t *cand_t,
                              double *seg_sum, double *block);

/*
 * support_pack_count, then support_pack, on T leaves.  mode 0: a leaf is taken iff skip[t] == 0 (skip: T bytes), and
 * bound (T doubles, or null) gives min_margin; mode 1: a leaf is taken iff status[t] != 0 (status: T int32), and
 * neither skip nor bound is read (they are handed to the kernels as given).  In and out: seg_count (G int32: leaves
 * taken per segment), seg_min (G doubles: the smallest bound - pi0 over the segment's leaves NOT taken in mode 0 with
 * a bound, else +inf), packed (T int32: the first *count_out entries are the taken positions in ascending order, the
 * rest is not written), count_out (one int32) and min_margin_out (one double: the smallest seg_min).
 * MIPX_EINVAL: a null array the mode needs (or a null output); T < 0 or above 2^30; mode not 0 or 1; pi0 NaN.
 */
int mipx_support_pack_batch(mipx_ctx *ctx, int64_t T, int mode, double pi0, const uint8_t *skip, const int32_t *status,
                            const double *bound, int32_t *seg_count, double *seg_min, int32_t *packed,
                            int32_t *count_out, double *min_margin_out);

/*
 * support_gather: rows packed[k] of l, u (T x n) and, where v (T x (n + m) codes) is given, of v, into rows k of pl, pu
 * (count x n) and pv_in (count x (n + m)), all three in and out.  v = null is the cold launch: pv_in is not written
 * (and may be null).
 * MIPX_EINVAL: a null array; count or T negative or above 2^30; count > T; n < 1; m < 0; a packed[k] outside 0 .. T-1.
 */
int mipx_support_gather_batch(mipx_ctx *ctx, int64_t count, int64_t T, int n, int m, const int32_t *packed,
                              const double *l, const double *u, const int8_t *v, double *pl, double *pu, int8_t *pv_in);

/*
 * support_scatter: what a launch over the packed leaves wrote -- px (count x n), pobj (count), py (count x m), pv_out
 * (count x (n + m)), pstatus, piters, pnpivots (count) -- to the leaves' rows packed[k] of x, obj, y, v, status, iters,
 * npivots and has_y (T bytes), all in and out.  x, v, obj and status are overwritten; y is written and has_y set to 1
 * iff pstatus[k] == 0; iters and npivots are replaced (add = 0) or added to (add != 0).
 * MIPX_EINVAL: as mipx_support_gather_batch, and a position named twice in packed (two workgroups would write one leaf).
 */
int mipx_support_scatter_batch(mipx_ctx *ctx, int64_t count, int64_t T, int n, int m, const int32_t *packed, int add,
                               const double *px, const double *pobj, const double *py, const int8_t *pv_out,
                               const int32_t *pstatus, const int32_t *piters, const int32_t *pnpivots, double *x,
                               double *obj, double *y, int8_t *v, int32_t *status, int32_t *iters, int32_t *npivots,
                               uint8_t *has_y);

/*
 * support_mark: has_y[t] = (status[t] == 0) for every t < T (has_y: T bytes, in and out).
 * MIPX_EINVAL: a null array; T < 0 or above 2^30.
 */
int mipx_support_mark_batch(mipx_ctx *ctx, int64_t T, const int32_t *status, uint8_t *has_y);

#ifdef __cplusplus
}
#endif
#endif /* MIPX_SUPPORTKERNELS_H */
