/*
 * mipx_noderows.h -- the kernels that move node rows, run on a caller's pools (included by mipx.h).
 *
 * TEST SCAFFOLDING in the library, as mipx_dualfn_batch.h is: no product code calls these entries.  The kernels that
 * create, copy, pack, rebuild and migrate the (l, u, basis codes, cut list) rows of the node pool -- make_children,
 * pack_nodes, unpack_nodes, gather_plain_nodes (csrc/tree_kernels.hip.h), treerec_bounds (csrc/treerec_kernels.hip.h),
 * restart_seed (csrc/restart_kernels.hip.h), the four cutmig_* kernels (csrc/cutmig_kernels.hip.h) and the five spill_*
 * kernels (csrc/spill_kernels.hip.h) -- are bandwidth kernels that nothing but a whole search reaches, and a search
 * absorbs a wrong stride or a missed tail.  These entries run them on synthetic pools through the functions the engine
 * launches them with (the enqueue_* functions at the top of csrc/tree_engine.hip.h: the same kernels, grids and LDS
 * rule), so that every output bit can be compared with a plain restatement (tests/support/node_rows_reference.py,
 * tests/test_node_rows_gpu.py).
 *
 * Every entry takes host buffers, uploads them, runs the kernels on the context's stream, copies back and frees.
 * An array marked in and out is uploaded whole, then copied back whole whatever the kernels wrote, so that a caller's
 * sentinel bytes show what they left alone.  Everything a kernel indexes with is checked on the host before any
 * launch: a refused call (MIPX_EINVAL, with a message) launches nothing and leaves every array as it was.  count = 0
 * launches nothing.
 *
 * What the kernels promise, pinned by the tests of these entries:
 *   - a child row is its parent's pool row with one bound replaced, u[var] = floor(x) (left) or l[var] = ceil(x)
 *     (right), and the parent's n + m + kcut codes; codes past them, ids past kcut and every other row stay;
 *   - a message row is [l (n f64) | u (n f64) | nvs codes | pad to 8]; the pad bytes are never written;
 *   - a lineage row is the root's row with the branchings of the node's ancestors applied root-down, each overwriting
 *     the bound, at any width and depth; treerec_bounds and restart_seed write the same bits; malformed entries (an id
 *     past the mirror, a parent not below its child, a variable outside 0 .. n-1) end or skip and write nothing wild;
 *   - a cut list that does not fit is counted in bad, gets ncut = 0 and its ids are left alone;
 *   - spill offsets are the exclusive prefix sums of the record sizes at any count, the records the layout of
 *     mipx_spill.h, and unpack is pack's inverse on the rows named, leaving every other row alone.
 */
#ifndef MIPX_NODEROWS_H
#define MIPX_NODEROWS_H

#ifdef __cplusplus
extern "C" {
#endif

/*
 * make_children on `count` (parent, variable) pairs.  src_l, src_u: the source pool (src_rows x n).  x (batch_rows x n)
 * and vstat (batch_rows x (n + stride), stride = mstride in cut mode, m in plain mode) are the dense step outputs.
 * Pair p reads pool row parent_slot[p], batch row parent_pos[p], branches on var[p] and writes rows child_slot[2p]
 * (left) and child_slot[2p + 1] (right) of the destination pool: dst_l, dst_u (dst_rows x n), dst_v (dst_rows x
 * (n + stride)), and in cut mode dst_ncut (dst_rows) and dst_ids (dst_rows x kc), all in and out.
 * Plain mode: mstride = kc = 0 and the four cut arrays null.  Cut mode: mstride > 0, src_ncut (batch_rows) and src_ids
 * (batch_rows x kc) the parents' dense cut lists; the id arrays may be null with kc = 0.
 * MIPX_EINVAL: a null array; n, m, src_rows, batch_rows or dst_rows < 1; count < 0; a parent_slot, parent_pos, var or
 * child_slot outside its array; two equal child slots; plain mode with kc != 0 or a cut array given; kc outside 0 .. 64;
 * m + kc > mstride in cut mode; a src_ncut[parent_pos] outside 0 .. kc.
 */
int mipx_noderows_children(mipx_ctx *ctx, int n, int m, int mstride, int kc, int count, int src_rows,
                           const double *src_l, const double *src_u, int batch_rows, const double *x,
                           const int8_t *vstat, const int32_t *src_ncut, const int32_t *src_ids,
                           const int32_t *parent_slot, const int32_t *parent_pos, const int32_t *var,
                           const int32_t *child_slot, int dst_rows, double *dst_l, double *dst_u, int8_t *dst_v,
                           int32_t *dst_ncut, int32_t *dst_ids);

/*
 * pack_nodes: rows slot[k] of a pool (pool_rows x n bounds, pool_rows x nvs codes) into rows k of msg (count x rowbytes
 * bytes, rowbytes = 16 n + nvs rounded up to 8; in and out).
 * MIPX_EINVAL: a null array; n, nvs or pool_rows < 1; count < 0; a slot outside the pool.
 */
int mipx_noderows_pack(mipx_ctx *ctx, int n, int nvs, int count, const int32_t *slot, int pool_rows,
                       const double *pool_l, const double *pool_u, const int8_t *pool_v, void *msg);
/*
 * unpack_nodes: rows k of msg into rows slot[k] of the pool (in and out).
 * MIPX_EINVAL: as mipx_noderows_pack, and two equal slots.
 */
int mipx_noderows_unpack(mipx_ctx *ctx, int n, int nvs, int count, const int32_t *slot, const void *msg, int pool_rows,
                         double *pool_l, double *pool_u, int8_t *pool_v);
/*
 * gather_plain_nodes: rows slot[k] of a pool that keeps nvs_pool >= n + m codes per row into dense l, u (count x n) and
 * v (count x (n + m)), all three in and out.
 * MIPX_EINVAL: a null array; n, m or pool_rows < 1; nvs_pool < n + m; count < 0; a slot outside the pool.
 */
int mipx_noderows_gather_plain(mipx_ctx *ctx, int n, int m, int nvs_pool, int count, const int32_t *slot, int pool_rows,
                               const double *pool_l, const double *pool_u, const int8_t *pool_v, double *l, double *u,
                               int8_t *v);

/*
 * treerec_bounds on a caller's mirror of nodes_count records (parent, vd = 2 variable + direction, val), uploaded as
 * the engine's 16-byte entries, launched in the engine's chunks with the engine's LDS size.  ids: count node ids.
 * root_l, root_u: n.  root_v: nv codes, or null (out_v is then left alone).  out_l, out_u (count x n) and out_v
 * (count x nv) are in and out.
 * MIPX_EINVAL: n outside 1 .. 1024; nv < 1; a null array (root_v may be null; parent, vd, val with nodes_count = 0 and
 * ids with count = 0 too); count or nodes_count < 0; an id < 0.
 * NOT refused, because the kernel guards itself and the tests must reach the guards: an id >= nodes_count (the root's
 * row comes out), a parent >= its child's id (the walk ends there), a vd whose variable is outside 0 .. n-1 (skipped).
 */
int mipx_noderows_lineage_bounds(mipx_ctx *ctx, int n, int nv, int64_t nodes_count, const int32_t *parent,
                                 const int32_t *vd, const double *val, int count, const int64_t *ids,
                                 const double *root_l, const double *root_u, const int8_t *root_v, double *out_l,
                                 double *out_u, int8_t *out_v);
/*
 * restart_seed on the same mirror: seed k writes row slots[k] of a pool of `capacity` rows (pool_l, pool_u: capacity x n;
 * pool_v: capacity x nv; in and out); root_v null writes zero codes.
 * MIPX_EINVAL: as mipx_noderows_lineage_bounds; capacity < 1; two equal slots inside the pool.
 * NOT refused: a slot outside 0 .. capacity-1 (nothing of that seed is written), and the three above.
 */
int mipx_noderows_lineage_seed(mipx_ctx *ctx, int n, int nv, int64_t nodes_count, const int32_t *parent,
                               const int32_t *vd, const double *val, int count, const int64_t *ids,
                               const int32_t *slots, int64_t capacity, const double *root_l, const double *root_u,
                               const int8_t *root_v, double *pool_l, double *pool_u, int8_t *pool_v);

/*
 * cutmig_lists: the cut lists of pool rows slot[k] (pool_ncut: pool_rows; pool_ids: pool_rows x kc) as records
 * [ncut, kc ids (0 past ncut)] in lists (count x (1 + kc), in and out).
 * MIPX_EINVAL: a null array; kc outside 1 .. 64; pool_rows < 1; count < 0; a slot outside the pool.
 */
int mipx_noderows_cut_lists(mipx_ctx *ctx, int kc, int count, const int32_t *slot, int pool_rows,
                            const int32_t *pool_ncut, const int32_t *pool_ids, int32_t *lists);
/*
 * cutmig_gather: table row r <- store row src[r].  store_pi (store_rows x n), store_pi0 (store_rows); tab_pi (count x n)
 * and tab_pi0 (count) in and out.
 * MIPX_EINVAL: a null array; n or store_rows < 1; count < 0; a src outside the store.
 */
int mipx_noderows_cut_gather(mipx_ctx *ctx, int n, int count, const int32_t *src, int64_t store_rows,
                             const double *store_pi, const double *store_pi0, double *tab_pi, double *tab_pi0);
/*
 * cutmig_scatter: store row base + r <- table row r; the store in and out.
 * MIPX_EINVAL: a null array; n or store_rows < 1; count or base < 0; base + count > store_rows.
 */
int mipx_noderows_cut_scatter(mipx_ctx *ctx, int n, int count, int64_t base, const double *tab_pi, const double *tab_pi0,
                              int64_t store_rows, double *store_pi, double *store_pi0);
/*
 * cutmig_unpack_lists: record k of lists ([ncut, kc table refs]) into the cut list of pool row slot[k] (pool_ncut,
 * pool_ids: in and out), ids = base + ref.  *bad: the records whose list does not fit (ncut outside 0 .. kc, a ref
 * outside 0 .. ctab-1); such a record gets ncut = 0 and its ids stay.  Those records are NOT refused.
 * MIPX_EINVAL: a null array; kc outside 1 .. 64; pool_rows < 1; count, base or ctab < 0; base + ctab > INT32_MAX; a
 * slot outside the pool; two equal slots.
 */
int mipx_noderows_cut_unpack_lists(mipx_ctx *ctx, int kc, int count, const int32_t *slot, const int32_t *lists,
                                   int64_t base, int ctab, int pool_rows, int32_t *pool_ncut, int32_t *pool_ids,
                                   int32_t *bad);

/*
 * spill_count, spill_scan, spill_pack as a spill event runs them: record r is row slot[r] of the pool (l, u: pool_rows
 * x n; v: pool_rows x nv; cut mode, kc > 0: ncut (pool_rows), ids (pool_rows x kc)), or row r where slot is null; its
 * header id is node_id[r], or r where node_id is null.  out_offsets (count + 1) and out_bytes (cap bytes) are in and
 * out; *used is the records' total.  MIPX_ENOMEM with *used set where cap is too small (out_offsets then holds the
 * offsets, out_bytes is as it was).
 * MIPX_EINVAL: a null array (slot, node_id may be null; ncut, ids with kc = 0); n, nv or pool_rows < 1; kc outside
 * 0 .. 64; count or cap < 0; a slot outside the pool; count > pool_rows without a slot list; an ncut of a named row
 * outside 0 .. kc.
 */
int mipx_noderows_spill_pack(mipx_ctx *ctx, int n, int nv, int kc, int count, const double *root_l, const double *root_u,
                             int pool_rows, const double *l, const double *u, const int8_t *v, const int32_t *ncut,
                             const int32_t *ids, const int32_t *slot, const int64_t *node_id, int64_t *out_offsets,
                             void *out_bytes, int64_t cap, int64_t *used);
/*
 * spill_unpack: record r (bytes offsets[r] .. offsets[r + 1] of in_bytes) into row slot[r] of the pool (row r where
 * slot is null); the pool's five arrays in and out.
 * MIPX_EINVAL: as above; two equal slots; records that disagree with their headers (as mipx_node_unpack_batch).
 */
int mipx_noderows_spill_unpack(mipx_ctx *ctx, int n, int nv, int kc, int count, const double *root_l,
                               const double *root_u, const int64_t *offsets, const void *in_bytes, const int32_t *slot,
                               int pool_rows, double *l, double *u, int8_t *v, int32_t *ncut, int32_t *ids);
/*
 * spill_gather_rows: rows slot[k] of a pool (src_rows x n, src_rows x nv) into rows k of l, u (count x n) and v
 * (count x nv), in and out; a row with slot[k] < 0 is left alone.
 * MIPX_EINVAL: a null array; n, nv or src_rows < 1; count < 0; a slot >= src_rows.
 */
int mipx_noderows_spill_gather_rows(mipx_ctx *ctx, int n, int nv, int count, const int32_t *slot, int src_rows,
                                    const double *src_l, const double *src_u, const int8_t *src_v, double *l, double *u,
                                    int8_t *v);

#ifdef __cplusplus
}
#endif
#endif /* MIPX_NODEROWS_H */
