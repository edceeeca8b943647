/*
 * mipx_rcfix.h -- reduced-cost bound tightening on the GPU (included by mipx.h).
 *
 * Every node LP of the frontier engine ends with row duals.  Given an incumbent, the duals of a node bound every
 * column of that node's subtree from its reduced cost: a column whose reduced cost is d_j > 0 cannot rise more than
 * (cutoff - z) / d_j above its lower bound without the objective passing the cutoff, z being the bound the duals
 * give.  The engine can run this on the branching parents of its steps, before their children are written
 * (mipx_tree_set_reduced_cost), or a caller on boxes and dual vectors of their own
 * (mipx_reduced_cost_tighten_batch).  One workgroup per node.
 *
 * For one node with the problem's rows A x >= b (m x n) and objective c (min), a box l, u (l finite, u possibly
 * +inf), ANY vector y of m doubles, the integer columns int_idx, a cutoff U, tol >= 0 and dtol >= 0:
 *
 * 1 DUALS.    yp_i = y_i if y_i > 0, else +0 (a NaN counts as 0).
 * 2 REDUCED COSTS.  d_j = c_j, then for i ascending d_j = d_j - (a_ij * yp_i): product and subtraction rounded
 *           separately, not fused.  (A row with yp_i = 0 changes no d_j and may be skipped.)
 * 3 TERMS.    t_j = d_j * l_j if d_j > 0, d_j * u_j if d_j < 0, else +0.  It is -inf where u_j = +inf and d_j < 0.
 * 4 BOUND.    z = YB + T.  YB = sum_i yp_i * b_i, rows ascending from +0.  T = sum_j t_j in this order: with 256
 *           partial sums, partial k adds the terms of its columns k, k + 256, k + 512, ... ascending from +0; the
 *           partials are then folded in place with strides s = 128, 64, ..., 1 (p[k] += p[k + s] for k < s); T = p[0].
 * 5 NO BOUND.  U is not finite, or z is -inf or NaN: status 3, nothing changes.
 * 6 GAP.      g = U - z.  g < -1e-6 * max(1, |U|): status 2 (cut off), nothing changes.  Otherwise g = max(g, 0).
 * 7 BOUNDS.   For the integer columns only:
 *           d_j > dtol:                   v = l_j + floor(g / d_j + tol);     u'_j = v if v < u_j, else u_j;
 *           d_j < -dtol and u_j finite:   v = u_j - floor(g / (-d_j) + tol);  l'_j = v if v > l_j, else l_j;
 *           every other column keeps its bounds.
 * 8 OUTPUT.   l', u'; z; a status (0 unchanged, 1 tightened, 2 cut off, 3 no bound); the number of bounds changed
 *           (l'_j != l_j and u'_j != u_j count one each).
 *
 * VALIDITY holds for any y, not only for the duals of an optimal basis.  With yp >= 0 every x of the box with
 * A x >= b has c . x >= yp . b + d . x >= z + d_j (x_j - l_j) for d_j > 0, and >= z + d_j (x_j - u_j) for d_j < 0.
 * So no point of the box with A x >= b and c . x <= U is lost, status 2 is given only when there is none (up to the
 * stated slack), and l'_j <= u'_j always holds because g >= 0.  dtol only decides which columns are skipped.
 * ARITHMETIC.  Nothing is fused; the orders above are the kernel's, and tests/support/reduced_cost_reference.py
 * restates them, so l', u' and z agree bit for bit.
 */
#ifndef MIPX_RCFIX_H
#define MIPX_RCFIX_H

#ifdef __cplusplus
extern "C" {
#endif

#define MIPX_RCFIX_UNCHANGED 0
#define MIPX_RCFIX_TIGHTENED 1
#define MIPX_RCFIX_CUT_OFF 2
#define MIPX_RCFIX_NO_BOUND 3

/*
 * Host buffers, one launch.  l, u: batch x n boxes; y: batch x m; int_idx: n_int distinct columns; cutoff: +inf or
 * -inf for none (every node then ends with status 3).  l_out, u_out: batch x n (they may be l, u); z_out,
 * status_out, changed_out: batch.  A batch of 0 is no launch.
 * MIPX_EINVAL: a null or out-of-range argument, tol < 0, dtol < 0, a NaN cutoff, int_idx out of range or repeated,
 * an l that is not finite, a u that is NaN or -inf;  MIPX_ETOOBIG: m or n above 1024.
 */
int mipx_reduced_cost_tighten_batch(mipx_problem *p, int batch, const double *l, const double *u, const double *y,
                                    const int32_t *int_idx, int n_int, double cutoff, double tol, double dtol,
                                    double *l_out, double *u_out, double *z_out, int32_t *status_out,
                                    int32_t *changed_out);
/*
 * Run the tightening inside the search (on != 0): the node LPs of every step then also write their row duals, and
 * when a step is finished its branching parents -- the batch's nodes, then their plunge children level by level --
 * are tightened in place on their pool rows with those duals, tol = 1e-6, dtol = 1e-9 and the incumbent the host
 * holds then as the cutoff, in front of the launch that writes their children.  Children are written from their
 * parent's row, so the whole subtree inherits the bounds.  With no incumbent there is no launch.  Nodes that come
 * out cut off or without a bound are only counted.  Every step is then finished on the host, as with
 * mipx_tree_set_propagation.  Set before the first step.
 * MIPX_EINVAL: a tree with cut rounds, with a communicator, with the dual function or the tree record on (a
 * tightened bound depends on b and on the incumbent, and a bound rebuilt from a lineage would miss it), a tree that
 * has stepped;  MIPX_ETOOBIG: m or n above 1024.  mipx_tree_set_comm, mipx_tree_set_dual_record and
 * mipx_tree_set_tree_record refuse a tree that has the tightening on.
 */
int mipx_tree_set_reduced_cost(mipx_tree *t, int on);
/*
 * [0] nodes run, [1] of those, tightened, [2] cut off, [3] without a bound, [4] bounds changed, [5] launches,
 * [6] reserved (0), [7] device time of the kernel in microseconds.  All 0 on a tree without the tightening.
 */
int mipx_tree_reduced_cost_stats(mipx_tree *t, int64_t out[8]);

#ifdef __cplusplus
}
#endif
#endif /* MIPX_RCFIX_H */
