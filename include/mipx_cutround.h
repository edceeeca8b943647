/*
 * mipx_cutround.h -- the kernels of a cut round of the frontier engine, run on a caller's data (included by mipx.h).
 *
 * TEST SCAFFOLDING in the library, as mipx_finish.h is: no product code calls these entries.  A cut round is six
 * kernels in a row with no host between them (cut_gather_state, cut_round_begin, K2 gomory_cuts in its slab form,
 * pool_append, K3 select_cuts over the pool lists, cut_round_apply), and nothing but a whole search reaches them in
 * that form.  The two entries run them on a synthetic round through the same two functions the engine launches them
 * with (enqueue_cut_begin and enqueue_cut_generate in csrc/tree_engine.hip.h: the same grids, block sizes and LDS
 * sizes), so that every output can be compared with a plain restatement of the reference's loop
 * (tests/support/cut_round_reference.py, tests/test_cut_round_kernels_gpu.py).
 *
 * A round has B nodes.  Node k has the m0 shared rows of the problem and ncut[k] <= kc cut rows; its cut row i is row
 * ids[k][i] of the cut store (store_pi: n doubles a row, store_pi0).  ms = m0 + kc rows are allotted per node in vstat,
 * y, T and idx.  state is CF_FIELDS = 12 int32 arrays of B entries, field-major: rounds | it_created | n_created |
 * it_added | n_added | it_removed | n_removed | ncut_out | stalled | pool_n | slab_n | dropped.  A node's candidate
 * cuts live in its slab of slab_rows rows (slab_pi, slab_pi0); rows below slab_n are taken, and pool_list[k][0..pool_n)
 * names the slab rows that are still in the pool, in pool order.  counters: n_active | n_changed | max_ncut |
 * n_need_tab; the kernels only add to them (max_ncut: a running maximum), the engine clears them between rounds.
 *
 * What the engine does not say anywhere else, pinned by the tests of these entries:
 *   - n_added counts K3's selection, including the cuts that were then dropped for lack of room; dropped counts a
 *     cut once, for whichever of the three causes (slab full, node list full, store full);
 *   - a node whose list is full takes no store entry for a dropped cut; a node that finds the store full does
 *     (store_count runs past store_cap by the number of such attempts);
 *   - a cut that is selected leaves the pool whether or not there was room for it;
 *   - cut_round_begin and cut_round_apply leave the entries of ids and vstat past the new ncut as they were.
 */
#ifndef MIPX_CUTROUND_H
#define MIPX_CUTROUND_H

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The first half of a round on host buffers: with gather = 1 cut_gather_state first (ncut, ids from the caller's pool
 * lists pool_ncut[pool_rows], pool_ids[pool_rows x kc] at the rows slot[B]; state zeroed; counters[2] raised to the
 * largest ncut), then cut_round_begin: the stall test of the round before (round > 0), who goes on generating, the
 * removal of the cut rows whose dual is exactly 0.
 * In:      status, mipf (B int32), obj (B f64), y (B x ms f64: row duals)
 * In/out:  vstat (B x (n + ms) int8), ncut (B), ids (B x kc), state (12 x B), obj_before (B f64), active (B),
 *          counters (4) -- uploaded, then copied back whatever the kernels wrote
 * Out:     resolve (B), need_tab (B)
 * MIPX_EINVAL: a null argument; n, m0, kc, B, round, max_rounds, have_dump or gather out of range (kc in 1..64); a
 * shape mipx_tree_create_ex would refuse (m0 + kc rows must fit where m0 rows do); gather = 1 with a slot outside
 * pool_rows or a pool_ncut outside 0..kc; gather = 0 with an ncut outside 0..kc.
 */
int mipx_cut_round_begin_batch(mipx_ctx *ctx, int n, int m0, int kc, int B, int round, int max_rounds,
                               double progress_tol, double max_dual_bound, int have_dump, int gather, int pool_rows,
                               const int32_t *slot, const int32_t *pool_ncut, const int32_t *pool_ids,
                               const int32_t *status, const double *obj, const int32_t *mipf, const double *y,
                               int8_t *vstat, int32_t *ncut, int32_t *ids, int32_t *state, double *obj_before,
                               int32_t *active, int32_t *counters, int32_t *resolve, int32_t *need_tab);

/*
 * The second half: K2 (GMI cuts of the dumped tableaux T (B x ms x n) and idx (B x (2 n + ms): nvar | bvar | side),
 * safely rounded, into the slabs), pool_append, K3 (selection over the pool lists, x read as max(x, 0)) and
 * cut_round_apply (the selection into the store, the node lists and the bases; the pool without it).  A and b are the
 * problem's.  chunks (workgroups per node: 0, 1, 4 or 16) and group (cuts a workgroup works out together: 0..8); 0
 * selects the engine's own rule, and used[0..1] returns the two values the launch ran with.
 * In:      T, idx, x (B x n), is_int (n bytes), active (B)
 * In/out:  vstat, ncut, ids, state, pool_list (B x slab_rows), slab_pi (B x slab_rows x n), slab_pi0 (B x slab_rows),
 *          store_pi (store_cap x n), store_pi0 (store_cap), store_count (1), resolve (B), counters (4)
 * Out:     k2_ncuts (B), k3_nadded (B), k3_added (B x slab_rows), k3_term (B), used (2)
 * MIPX_EINVAL: a null argument; B < 1, kc outside 1..64, slab_rows outside 1..2040, chunks not in {0, 1, 4, 16}, group
 * outside 0..8, store_cap < 1, a cut parameter mipx_tree_create_ex would refuse, a shape it would refuse, a group
 * whose staging does not fit the LDS; an ncut outside 0..kc, an id of a node's list outside the store, a negative
 * store_count, pool and slab counts outside slab_rows (or more pool entries than slab rows taken), a pool_list entry
 * outside slab_rows; for an active node, nvar and bvar of idx that are not a split of 0 .. n + m0 + ncut - 1.
 */
int mipx_cut_round_generate_batch(mipx_problem *p, int B, int kc, int slab_rows, int chunks, int group, int store_cap,
                                  double max_term, int max_nonzero_coefs, double min_cut_depth, double cos_parallel,
                                  double max_abs_coef, const double *T, const int32_t *idx, const double *x,
                                  const uint8_t *is_int, const int32_t *active, int8_t *vstat, int32_t *ncut,
                                  int32_t *ids, int32_t *state, int32_t *pool_list, double *slab_pi, double *slab_pi0,
                                  double *store_pi, double *store_pi0, int32_t *store_count, int32_t *resolve,
                                  int32_t *counters, int32_t *k2_ncuts, int32_t *k3_nadded, int32_t *k3_added,
                                  int32_t *k3_term, int32_t *used);

#ifdef __cplusplus
}
#endif
#endif /* MIPX_CUTROUND_H */
