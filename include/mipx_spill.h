/*
 * mipx_spill.h -- host spill of the frontier engine's open nodes (included by mipx.h).
 *
 * COMPACT NODE RECORD.  A node's pool row (bounds l, u: n f64 each; basis codes: nv int8, nv = n + mrows;
 * in cut mode its cut list) differs from the root's bounds only in the columns branched on along its path
 * and its basis codes fit in 4 bits.  One record, all fields little-endian, every section 8-byte aligned:
 *
 *   offset 0    int64  node id          (mipx_node_pack_batch: the record's position in the batch)
 *          8    int32  ndiff            columns whose l or u differs BITWISE from the root's
 *                                       (-0.0 vs 0.0 differs; infinities compare exactly)
 *         12    int32  ncut             cut rows the node carries (0 without cut rounds)
 *         16    int32  col[ndiff]       ascending column indices, zero-padded to a multiple of 8 bytes
 *               f64    l[ndiff]         the node's lower bounds of those columns
 *               f64    u[ndiff]         ... and upper bounds
 *               uint8  code[ceil(nv/2)] basis code j in the low nibble of byte j/2 (j even) or the high
 *                                       nibble (j odd), two's complement in 4 bits (Clp codes 0..5);
 *                                       an odd nv leaves the last high nibble 0; zero-padded to 8 bytes
 *               int32  cut_id[ncut]     cut mode only (kcut > 0): ids into the cut store, zero-padded to 8
 *
 *   bytes(ndiff, ncut) = 16 + pad8(4 ndiff) + 16 ndiff + pad8(ceil(nv / 2)) + (kcut > 0 ? pad8(4 ncut) : 0)
 *
 * Records are stored back to back; record k starts at offsets[k], offsets[count] is the total.
 * Unpacking fills the row with the root's bounds, scatters the diffs and expands the nibbles; cut ids
 * beyond ncut are not part of a record (unpack leaves them as they were).
 */
#ifndef MIPX_SPILL_H
#define MIPX_SPILL_H

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The spill kernels on host buffers (for tests and tools; the engine runs them on its pool).
 * count rows: l, u count x n, vstat count x nv; cut mode when kcut > 0: ncut (count), cut_ids count x kcut.
 * root_l, root_u: n.  Pack writes count + 1 offsets and the records into out_bytes (cap bytes) and the
 * total into *used; with cap too small it writes nothing but *used and returns MIPX_ENOMEM.
 */
int mipx_node_pack_batch(mipx_ctx *ctx, int n, int nv, int count, const double *root_l, const double *root_u,
                         const double *l, const double *u, const int8_t *vstat, const int32_t *ncut,
                         const int32_t *cut_ids, int kcut, int64_t *out_offsets, void *out_bytes, int64_t cap,
                         int64_t *used);
/* The inverse: records at offsets[0..count] of in_bytes back into rows (same shapes as above). */
int mipx_node_unpack_batch(mipx_ctx *ctx, int n, int nv, int count, const double *root_l, const double *root_u,
                           const int64_t *offsets, const void *in_bytes, double *l, double *u, int8_t *vstat,
                           int32_t *ncut, int32_t *cut_ids, int kcut);

/*
 * Opt-in host spill of the frontier engine (max_host_bytes > 0; 0 turns it off, the default).  When the
 * free pool rows fall below the headroom a step launch needs, the open nodes the queue will pop last are
 * packed into compact records, copied to pinned host memory and their rows freed; a spilled node is
 * copied back and unpacked into a row when it is popped.  A run with spill evaluates the same nodes in the
 * same order, with bit-identical results, as a run whose pool never fills.
 *
 *   headroom rows   H = S x B x (2 (1 + dive) + 1),  S = 3 steps in flight when max_batch > 1, else 1,
 *                                                     B = max_batch, dive = mipx_tree_set_dive depth
 *   minimum pool    pool_capacity >= 2 H + 1
 *
 * MIPX_EINVAL with a communicator (mipx_tree_set_comm), with a pool below the minimum, or when the dive
 * depth set later raises the headroom above the pool (mipx_tree_solve checks it again).  When the
 * spilled records would exceed max_host_bytes the search stops as it does when the pool is full
 * (status 4, mipx_tree_stats.pool_exhausted = 1).  mipx_tree_peek_open / mipx_tree_peek_cuts decode
 * spilled nodes on the host.  mipx_tree_reanchor decodes the spilled nodes among the first max_nodes into a
 * scratch block for its refactor launch, so they get the anchors they would get in a pool that never fills.
 * Turned off (0) after spilling, nodes on the host still come back when popped; the batches then leave a
 * row per node for that, and the search may stop on a full pool as it would without the spill.
 */
int mipx_tree_set_host_spill(mipx_tree *t, int64_t max_host_bytes);
/* [0] nodes spilled, [1] nodes reloaded, [2] nodes on the host now, [3] host bytes now, [4] peak host
 * bytes, [5] spill events, [6] spill and [7] reload time in microseconds (host wall time of the spill
 * events; of staging and queueing the reloads). */
int mipx_tree_spill_stats(mipx_tree *t, int64_t out[8]);

#ifdef __cplusplus
}
#endif
#endif /* MIPX_SPILL_H */
