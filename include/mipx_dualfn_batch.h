/*
 * mipx_dualfn_batch.h -- the four kernels of the dual function, run on a caller's data (included by mipx.h).
 *
 * TEST SCAFFOLDING in the library, as mipx_debug_enable is: no product code calls these entries.  The kernels of
 * csrc/dualfn_kernels.hip.h (dualfn_record, dualfn_save, dualfn_gemm, dualfn_lineage) record the duals of a search and
 * evaluate its dual function (mipx_dualfn.h), and nothing but a whole search reaches them; f(w) is a minimum over leaves
 * of a maximum over a lineage, so most of what they compute never shows in the scalar that comes out.  These three
 * entries run them on synthetic records through the same functions the engine launches them with (enqueue_df_record,
 * enqueue_df_save and df_eval_tiles in csrc/dualfn.hip.h: the same kernels, grids and tile rule), so that every output
 * can be compared with a plain restatement (tests/support/dualfn_reference.py, tests/test_dualfn_kernels_gpu.py).
 *
 * Every entry takes host buffers, uploads them, runs the kernels on the context's stream, copies back and frees.
 * An array marked in and out is uploaded, then copied back whole whatever the kernels wrote, so that a caller's
 * sentinels show what they left alone.  Everything a kernel indexes with is checked on the host before any launch:
 * a refused call (MIPX_EINVAL, with a message) launches nothing.
 *
 * What the kernels promise, pinned by the tests of these entries:
 *   - d_j = c_j - acc_j with acc_j one FMA chain over the rows i = 0 .. m-1 from 0.0; the column's term is
 *     max(d_j, 0) fin(l_j) + min(d_j, 0) fin(u_j), fin(+-inf) = +-DBL_MAX (so 0 x inf enters as 0); thread tid of 256
 *     adds the terms of its columns tid, tid + 256, ... in that order, and t is the pairwise tree s = 128, 64, .. 1
 *     over the 256 running sums;
 *   - a record block of fewer than 4 entries reads its first entry for the idle slots and writes nothing for them;
 *   - V[k, r] = T[r] + acc with acc one FMA chain over i = 0 .. m-1 from 0.0, whatever R, K, the tile of right-hand
 *     sides and the 32-row slab of the kernel: the padding of a partial slab is never summed;
 *   - the lineage pass is max and min alone: given V it rounds nothing.
 */
#ifndef MIPX_DUALFN_BATCH_H
#define MIPX_DUALFN_BATCH_H

#ifdef __cplusplus
extern "C" {
#endif

/*
 * dualfn_record on `count` entries.  A (m x n, row-major) and c (n) are the LP's; entry e takes its duals from row
 * src[e] of y_src (y_rows x m), its bounds from row lrow[e] of l and u (b_rows x n each) and writes record dst[e]:
 * row dst[e] of store_y (store_rows x m, in and out) and store_t[dst[e]] (store_rows, in and out).  count = 0 launches
 * nothing.
 * MIPX_EINVAL: a null array (src, lrow, dst may be null with count = 0), m, n, y_rows, b_rows or store_rows < 1,
 * count < 0, a src, lrow or dst outside its rows, two equal dst.
 */
int mipx_dualfn_record_batch(mipx_ctx *ctx, int m, int n, const double *A, const double *c, int count, const int32_t *src,
                             const int32_t *lrow, const int64_t *dst, int y_rows, const double *y_src, int b_rows,
                             const double *l, const double *u, int store_rows, double *store_y, double *store_t);
/*
 * dualfn_save on `count` entries: entry e copies row lrow[e] of l and u (b_rows x n) and row vpos[e] of vstat
 * (v_rows x nv int8) into row dst[e] of out_l, out_u (out_rows x n) and out_v (out_rows x nv), all three in and out.
 * count = 0 launches nothing.
 * MIPX_EINVAL: a null array (lrow, vpos, dst may be null with count = 0), n, nv, b_rows, v_rows or out_rows < 1,
 * count < 0, an lrow, vpos or dst outside its rows, two equal dst.
 */
int mipx_dualfn_save_batch(mipx_ctx *ctx, int n, int nv, int count, const int32_t *lrow, const int32_t *vpos,
                           const int64_t *dst, int b_rows, const double *l, const double *u, int v_rows,
                           const int8_t *vstat, int out_rows, double *out_l, double *out_u, int8_t *out_v);
/*
 * dualfn_gemm then dualfn_lineage on R records (Y: R x m, T: R) and K right-hand sides (W: K x m), tile by tile as an
 * evaluation of the engine runs them.  k_tile = 0 takes the engine's tile (min(K, 1024, 256 MB / 8 R) right-hand
 * sides); k_tile > 0 caps it at k_tile.  The lineage: prec[r] the record of r's nearest recorded ancestor (-1: none),
 * order the records by level, lvl_off the nlvl + 1 offsets of the levels in order, leaf the nleaf records that bound a
 * leaf, bare = 1 if some leaf has no record at all (every value is then -inf).
 * Out: V_gemm (K x R, or null): V between the two kernels;  V_max (K x R, or null): V after the lineage pass;
 * out (K): the values.
 * MIPX_EINVAL: a null array (leaf may be null with nleaf = 0), R, m, K or nlvl < 1, k_tile or nleaf < 0, nleaf = 0
 * with bare = 0 (the engine answers that on the host: +inf), lvl_off not ascending from 0 to R, order no permutation
 * of 0 .. R-1, a record of level 0 with prec != -1, a record of a level L >= 1 whose prec is not a record of a lower
 * level, a leaf outside 0 .. R-1.
 */
int mipx_dualfn_eval_batch(mipx_ctx *ctx, int R, int m, int K, int k_tile, const double *Y, const double *T,
                           const double *W, const int32_t *prec, const int32_t *order, const int32_t *lvl_off, int nlvl,
                           const int32_t *leaf, int nleaf, int bare, double *V_gemm, double *V_max, double *out);

#ifdef __cplusplus
}
#endif
#endif /* MIPX_DUALFN_BATCH_H */
