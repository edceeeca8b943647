/*
 * mipx_prop.h -- node presolve on the GPU: activity-based bound propagation over the rows (included by mipx.h).
 *
 * The frontier engine hands every popped node to the node LP with exactly the bounds its branchings gave it.
 * Bound propagation tightens the bounds of the integer columns from the rows, the incumbent's objective cutoff
 * included, one workgroup per node; the engine can run it on the nodes of its steps before their LPs
 * (mipx_tree_set_propagation) or a caller on boxes of their own (mipx_propagate_batch).
 *
 * For one node with the problem's rows A x >= b (m x n), objective c, bounds l, u (l finite, u possibly +inf),
 * the integer columns int_idx, a tolerance tol >= 0, a round cap max_rounds >= 1 and a cutoff: when the cutoff is
 * finite, one more row (-c) x >= -cutoff takes part as row m.
 *
 * ONE ROUND.  Everything is computed from the bounds the round started with (Jacobi), so the result does not
 *          depend on how the work is split.
 * ACTIVITY.  For a row i and a column j with a_ij != 0 the largest its term can be is h_ij = a_ij u_j when
 *          a_ij > 0, else a_ij l_j.  ninf_i counts the infinite h_ij of the row, S_i is the sum of the finite ones.
 * CONFLICT.  A row with ninf_i = 0 and S_i < b_i - tol: the node is infeasible, and the round ends here.
 * CANDIDATES.  Only for integer columns.  Row i gives column j (a_ij != 0) a candidate when ninf_i = 0, or when
 *          ninf_i = 1 and h_ij is the infinite term: q = (b_i - (S_i - h_ij)) / a_ij, an infinite h_ij subtracted
 *          as 0.  For a_ij > 0 it is the lower bound ceil(q - tol), for a_ij < 0 the upper bound floor(q + tol)
 *          (a zero candidate is +0).
 * UPDATE.  l'_j is the largest of l_j and the lower candidates of j, u'_j the smallest of u_j and its upper
 *          candidates; the other columns only contribute terms and keep their bounds.  l'_j > u'_j for some j: the
 *          node is infeasible.
 * STOP.    After a round that changed no bound, after max_rounds rounds, or with the node found infeasible.
 * OUTPUT.  l', u'; a status (0 unchanged, 1 tightened, 2 infeasible; an infeasible node returns its bounds exactly
 *          as they came in); the number of bounds changed (l'_j != l_j and u'_j != u_j count one each), summed
 *          over the rounds that ended with an update and no conflict; the number of rounds started.
 *
 * VALIDITY.  No integer-feasible point of the box with c . x <= cutoff is cut off, and status 2 is given only when
 *          there is none.
 * ARITHMETIC.  Products are not fused.  The order in which S_i is summed is the kernel's (lanes stride the columns,
 *          then a butterfly over the wave): on integer data every order gives the same bits, and the bounds that
 *          come out are integers from floor and ceil (tests/support/propagation_reference.py restates it).
 */
#ifndef MIPX_PROP_H
#define MIPX_PROP_H

#ifdef __cplusplus
extern "C" {
#endif

#define MIPX_PROP_UNCHANGED 0
#define MIPX_PROP_TIGHTENED 1
#define MIPX_PROP_INFEASIBLE 2

/*
 * Host buffers, one launch.  l, u: batch x n boxes; int_idx: n_int distinct columns; cutoff: +inf or -inf for no
 * cutoff row.  l_out, u_out: batch x n; status_out, changed_out, rounds_out: batch.
 * MIPX_EINVAL: a null or out-of-range argument, tol < 0, max_rounds < 1, a NaN cutoff, int_idx out of range or
 * repeated, an l that is not finite, a u that is NaN or -inf;  MIPX_ETOOBIG: m or n above 1024.
 */
int mipx_propagate_batch(mipx_problem *p, int batch, const double *l, const double *u, const int32_t *int_idx,
                         int n_int, double cutoff, double tol, int max_rounds, double *l_out, double *u_out,
                         int32_t *status_out, int32_t *changed_out, int32_t *rounds_out);
/*
 * Run the propagation inside the search: in every step, behind the reload of spilled nodes and before the node
 * LPs, on the step's nodes in place (their pool rows), with tol = 1e-6, at most max_rounds rounds and, with
 * use_cutoff != 0, the incumbent the host holds at the launch as the cutoff (none yet: no cutoff row).  Children
 * are written from their parent's row, so a tightened bound is inherited by the whole subtree.  A node found
 * infeasible is finished as a node whose LP ended primal infeasible, whatever the LP launched on its unchanged row
 * returned: no children, its plunge children dropped.  Every step is then finished on the host, as with
 * mipx_tree_set_dual_record and mipx_tree_set_tree_record.  Set before the first step.
 * MIPX_EINVAL: max_rounds < 1, a tree with cut rounds, with a communicator, with the dual function or the tree
 * record on (a propagated bound depends on b, and a bound rebuilt from a lineage would miss it), a tree that has
 * stepped;  MIPX_ETOOBIG: m or n above 1024.  mipx_tree_set_comm, mipx_tree_set_dual_record and
 * mipx_tree_set_tree_record refuse a tree that has the propagation on.
 */
int mipx_tree_set_propagation(mipx_tree *t, int max_rounds, int use_cutoff);
/*
 * [0] nodes propagated, [1] of those, tightened, [2] found infeasible, [3] bounds changed, [4] rounds,
 * [5] nodes that stopped on max_rounds with their last round still changing a bound, [6] reserved (0),
 * [7] device time of the kernel in microseconds.  All 0 on a tree without the propagation.
 */
int mipx_tree_propagation_stats(mipx_tree *t, int64_t out[8]);

#ifdef __cplusplus
}
#endif
#endif /* MIPX_PROP_H */
