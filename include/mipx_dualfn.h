/*
 * mipx_dualfn.h -- the branch-and-bound dual function of a frontier-engine search (included by mipx.h).
 *
 * After a search, every solved node j with an optimal LP holds a dual solution: row duals y_j (one per
 * engine row, A x >= b) and reduced costs d_j = c - A^T y_j.  At a new right-hand side w (engine rows)
 *
 *   f(w) = min over leaves L of  max over solved nodes j on L's lineage of  y_j . w + t_j,
 *   t_j  = sum_i max(d_ji, 0) l_ji + min(d_ji, 0) u_ji        (infinite bounds enter as +-DBL_MAX)
 *
 * is a lower bound on the MILP optimum at w (BranchAndBound.find_parameterized_dual_bound).  With
 * recording on, the engine appends one RECORD (y_j, t_j) per node it solves to optimality, to an
 * append-only store in device memory: y as m f64 (record-major), t as one f64, plus on the host the
 * record's node id and, per node, its parent and its record.  A node whose LP is infeasible keeps its bounds and
 * final basis codes instead; the first evaluation re-solves all such leaves in one batched launch of the
 * penalised LP
 *
 *   [A | S] (x, s) >= b,  costs (c, M 1),  0 <= s,   S[e, pos_e] = sign_e (one slack per LP row)
 *
 * warm-started from the leaf's codes with the slacks at their lower bound, and records the result as the
 * leaf's own term.  A leaf whose penalised LP has no kernel (n + rows > 1024 columns) or does not end
 * optimal has no term of its own: its ancestors' terms bound it, and it is counted.
 *
 * Leaves are the nodes without children: open nodes at a stop, nodes closed at pop by their inherited
 * bound, integral, pruned and infeasible nodes.  A leaf without a record uses its nearest recorded
 * ancestor's; a leaf with none at all bounds nothing (f = -inf).
 *
 * Recording makes every step of the search be finished on the host (the host knows each child's
 * parent); its per-step cost is a y output of the node-LP kernels and one record kernel per step.
 */
#ifndef MIPX_DUALFN_H
#define MIPX_DUALFN_H

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Turn recording on (max_bytes > 0: the store's byte cap; -1: half of the device memory free now) before
 * the first step of the search.  rows
 * (the LP's own rows, the penalised LP's slacks), pos[e] in [0, rows) and sign[e] = +1 / -1 per engine
 * row describe the slack block S above.  When the store is full the search goes on and later nodes get
 * no record (counted as dropped): the bound stays valid, only weaker.
 * MIPX_EINVAL after the first step, with a communicator, with cut rounds, or with bad arguments.
 */
int mipx_tree_set_dual_record(mipx_tree *t, int64_t max_bytes, int rows, const int32_t *pos, const double *sign);
/*
 * out[k] = f(w_k) for the K right-hand sides w (K x m, engine rows), M the slack price of the penalised
 * re-solve.  The sum behind each value runs in a fixed order, whatever K: one w alone gives the same bits.
 */
int mipx_tree_dual_function(mipx_tree *t, int K, const double *w, double M, double *out);
/*
 * [0] records, [1] store bytes in use, [2] dropped nodes (no record: store full), [3] infeasible leaves,
 * [4] penalised re-solves, [5] leaves without a term of their own, [6] record time and [7] evaluation
 * time in microseconds (device time of the record kernels; host wall time of the evaluations).
 */
int mipx_tree_dual_function_stats(mipx_tree *t, int64_t out[8]);
/*
 * Test hook: the first min(max_records, records) records in store order -- node id, node id of the
 * parent (-1 at the root), LP status (0; 1 for a penalised re-solve of an infeasible leaf), t and y
 * (max_records x m).  Null outputs are skipped.  Returns the number of records.
 */
int64_t mipx_tree_dual_records(mipx_tree *t, int64_t max_records, int64_t *node, int64_t *parent, int32_t *status,
                               double *tval, double *y);

#ifdef __cplusplus
}
#endif
#endif /* MIPX_DUALFN_H */
