/*
 * mipx_treerec.h -- the search tree of a frontier-engine search, kept as records (included by mipx.h).
 *
 * With recording on, the engine keeps one RECORD per node it ever creates, beside its node table (branching
 * variable, direction, value, depth, inherited bound): the parent's id, the verdict and objective of the
 * node's LP, and flags.  Host memory, 14 bytes per node, no cap.  A record says who a node is, not where it
 * is: its bounds are the root's with the branchings of its lineage applied, and are rebuilt on request on
 * the device (mipx_tree_node_bounds); its LP solution is not stored and is re-solved on request, warm-started
 * from the root's optimal basis (mipx_tree_node_solve).
 *
 * Node ids are the engine's: the root is 0, the two children of a branching get consecutive ids, left
 * (x <= floor) first, in the order the nodes are branched on.  A parent's id is below its children's.
 *
 * Recording makes every step of the search be finished on the host (the host knows each child's parent),
 * as the dual function does (mipx_dualfn.h); the two can be on together.
 */
#ifndef MIPX_TREEREC_H
#define MIPX_TREEREC_H

#ifdef __cplusplus
extern "C" {
#endif

/* flags of a record */
#define MIPX_TR_MIP_FEASIBLE 1   /* the LP was solved and its solution is integral */
#define MIPX_TR_HAS_CHILDREN 2   /* the node was branched on */
#define MIPX_TR_CLOSED_AT_POP 4  /* popped and closed unsolved: its inherited bound could not beat the incumbent */
#define MIPX_TR_OPEN 8           /* still in the queue */
#define MIPX_TR_PROBED 16        /* strong-branching probes were made from the node (pseudo-cost rule) */

/*
 * Turn recording on (on != 0) before the first step of the search.
 * MIPX_EINVAL after the first step, with a communicator, or with cut rounds.
 */
int mipx_tree_set_tree_record(mipx_tree *t, int on);
/*
 * Copy the records [first, first + count) to host arrays (null outputs are skipped): parent id (-1 at the
 * root), branching variable (-1 at the root), direction (0 left, 1 right), value, depth, LP status (-1: never
 * solved, else 0 optimal / 1 infeasible / 2 unbounded / 3 stopped), flags (MIPX_TR_*), the bound inherited
 * from the parent and the LP objective (only meaningful with status 0 or 2).  Returns the number copied
 * (count clipped to the records there are) or an error.
 */
int64_t mipx_tree_records(mipx_tree *t, int64_t first, int64_t count, int64_t *parent, int32_t *bvar, int32_t *bdir,
                          double *bval, int32_t *depth, int32_t *lp_status, int32_t *flags, double *dual_bound,
                          double *objective);
/*
 * The bounds of the K nodes ids[0..K) (l, u: K x n, host buffers): on the device, one workgroup per node
 * copies the root's row and applies the branchings of the node's lineage (left: u[var] = floor(val), right:
 * l[var] = ceil(val), the deepest branching of a variable's side last, as the search wrote its pool rows).
 */
int mipx_tree_node_bounds(mipx_tree *t, int64_t K, const int64_t *ids, double *l, double *u);
/*
 * Re-solve the LPs of the K nodes ids[0..K): their bounds are rebuilt on the device and all K are solved in
 * one launch of the node-LP kernel, warm-started from the root's optimal basis (cold when the root did not
 * end optimal).  Outputs (host, null ones skipped): status (K), obj (K), x (K x n), vstat (K x (n + m)).
 */
int mipx_tree_node_solve(mipx_tree *t, int64_t K, const int64_t *ids, int32_t *status, double *obj, double *x,
                         int8_t *vstat);
/*
 * [0] nodes recorded, [1] host bytes of the records, [2] bytes of their device mirror, [3] nodes whose bounds
 * were rebuilt, [4] nodes re-solved, [5] device time of the query kernels in microseconds.
 */
int mipx_tree_record_stats(mipx_tree *t, int64_t out[6]);

#ifdef __cplusplus
}
#endif
#endif /* MIPX_TREEREC_H */
