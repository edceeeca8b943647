/*
 * mipx_restart.h -- restart a recorded search at another right-hand side from its leaves (included by mipx.h).
 *
 * Branching only moves variable bounds, so the childless nodes of any search tree partition the integer points
 * of the root box whatever b is, and their LPs at a new b are independent.  mipx_tree_create_restart makes a
 * new tree on a problem with the same A and c and the new b that starts where the recorded one (src, see
 * mipx_treerec.h) stands: it holds a copy of src's records -- the SKELETON -- and every childless record of
 * src is an open node of the new search, a SEED.  It does not matter what became of a seed in src
 * (infeasible, integral, closed at pop, probed, still open): at another b any of them may hold the optimum.
 *
 * The skeleton keeps ids, parents, branchings and depths; LP verdict, objective and inherited bound are
 * reset (status -1, never solved) and every flag but MIPX_TR_HAS_CHILDREN is cleared.  New nodes continue
 * the id sequence at src's created_nodes; the counters of the new tree start at 0; recording is on.  A seed's
 * pool row is written on the device: the root's bounds with the branchings of its lineage applied (as
 * mipx_tree_node_bounds rebuilds them), and src's root basis codes as its warm start -- a basis that was
 * dual feasible stays dual feasible when only b and bounds change (cold where src kept no root basis).  A
 * seed inherits the bound -inf: best first pops every seed before any child; depth first keys it by -depth.
 * With the anchor mode on, the anchor of `p` is that root basis, set before the first step.
 *
 * src is not modified and may be destroyed straight afterwards.
 */
#ifndef MIPX_RESTART_H
#define MIPX_RESTART_H

#ifdef __cplusplus
extern "C" {
#endif

/*
 * `p`: a problem of src's context with src's m and n, created by the caller from the same A and c and the new
 * b.  The new tree takes src's creation parameters (integer indices, root bounds, branch and search rule,
 * strong-branch iterations, max_batch, pool capacity), its pseudo-cost table and its root basis codes.
 * MIPX_EINVAL: src keeps no record, has cut rounds or a communicator, or p differs in shape or context.
 * MIPX_ENOMEM: the seeds and the rows a step reserves do not fit the pool (the message names the numbers).
 * A restarted tree takes no dual record (mipx_tree_set_dual_record: MIPX_EINVAL).
 */
int mipx_tree_create_restart(mipx_tree *src, mipx_problem *p, mipx_tree **out);
/*
 * [0] skeleton records, [1] seeds, [2] device bytes written by seeding, [3] device time of the seeding kernel
 * in microseconds, [4] seeds evaluated so far, [5] of those, ended infeasible, [6] of those, integral,
 * [7] reserved (0).  All 0 on a tree that is no restart.
 */
int mipx_tree_restart_stats(mipx_tree *t, int64_t out[8]);
/* The seed ids in ascending order, up to cap of them (ids may be null with cap 0); returns their number. */
int64_t mipx_tree_restart_seeds(mipx_tree *t, int64_t cap, int64_t *ids);

#ifdef __cplusplus
}
#endif
#endif /* MIPX_RESTART_H */
