/*
 * mipx_cglp.h -- disjunctive cuts from a recorded tree by batched leaf separation (included by mipx.h).
 *
 * A cut pi.x >= pi0 is valid for the disjunction of the leaves P_t = {A x >= b, l_t <= x <= u_t} of a subtree
 * iff pi0 <= h_t(pi) := min {pi.x : x in P_t} for every t.  A SUPPORT SESSION holds the leaves of one
 * disjunction on the device -- their bounds, rebuilt from the tree record (mipx_treerec.h), and the basis each
 * leaf LP ended on -- and evaluates h_t(pi) for all of them in one node-LP launch with pi in the place of the
 * objective.  The cut-generating LP then is solved by row generation in the space of (pi, pi0) alone: the
 * session is its separation oracle.
 *
 * Every leaf must be a polytope (finite bounds on every column): no leaf LP is unbounded for any pi.
 *
 * The first evaluation warm-starts every leaf from the root's optimal basis (as mipx_tree_node_solve does) and
 * DROPS the leaves whose LP is infeasible: they are empty terms.  Where it drops any, the leaves left are
 * packed and solved once more, so that from then on position k of the session is the same leaf in every
 * buffer.  Later evaluations warm-start each leaf from the basis its last LP ended on.
 *
 * Layout of the output block of mipx_tree_support_eval, 8 + max_points (n + 2) doubles:
 *   [0] the minimum margin  min_t h_t(pi) - pi0  over the session's leaves (+inf without any)
 *   [1] the node id of a leaf that attains it (the lowest id among them; -1 without any)
 *   [2] leaves with margin below -tol
 *   [3] P, the rows that follow: min(max_points, leaves of the session)
 *   [4] leaves whose LP did not end optimal (iteration limit, or unbounded: the session's premise is broken);
 *       they count as margin +inf and are never among the rows
 *   [5] simplex iterations and [6] pivots (refactorisation included) of this evaluation, over all leaves
 *   [7] leaves of the session after this evaluation
 * then P rows of n + 2: node id, h_t(pi), x_t (a minimiser, n doubles) -- the P leaves of smallest margin in
 * ascending order of (margin, node id), so the rows do not depend on how the launch was scheduled.
 *
 * A session may also keep the row duals of its leaves and screen with them: a leaf whose stored duals y+ >= 0 prove
 * L_t(pi; y+) = y+.b + sum_j min(r_j l_j, r_j u_j) >= pi0 - screen_tol (r = pi - A'y+; L_t <= h_t by weak duality)
 * gets no LP in that evaluation.  mipx_cglp_screen.h states the bound, its arithmetic and the entries
 * (mipx_tree_support_open_ex, mipx_tree_support_eval_ex); the two entries below are those with the options off.
 */
#ifndef MIPX_CGLP_H
#define MIPX_CGLP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mipx_support mipx_support;

/*
 * Open a session on the K recorded nodes ids[0..K) of a tree with recording on (distinct ids; no cut rounds).
 * Their bounds are rebuilt on the device, in launches of 2^14 nodes, and stay there: 3 K n doubles (l, u, x),
 * 2 K (n + m) bytes of basis codes and 40 K bytes of per-leaf words.  Syncs the stream.  MIPX_EINVAL if a
 * bound of any of the nodes is infinite.  The session must be closed before its tree is destroyed.
 */
int mipx_tree_support_open(mipx_tree *t, const int64_t *ids, int64_t K, mipx_support **out);
/*
 * h_t(pi) for every leaf of the session (pi: n doubles, host) and the selection against pi0 described above
 * into block (host, 8 + max_points (n + 2) doubles; 1 <= max_points <= 1024).  margins (host, null or one
 * double per leaf of the session as it stands after the call, in the order of mipx_tree_support_leaves) gets
 * every h_t - pi0.  Syncs the stream; only the block (and margins, if asked for) comes down.
 */
int mipx_tree_support_eval(mipx_support *s, const double *pi, double pi0, double tol, int max_points,
                           double *block, double *margins);
/*
 * The node ids of the session's leaves now (ids: null, or room for `cap` of them) and, with dropped != 0, of
 * the leaves dropped as infeasible instead.  Returns how many there are.
 */
int64_t mipx_tree_support_leaves(mipx_support *s, int dropped, int64_t cap, int64_t *ids);
/*
 * [0] leaves of the session, [1] leaves dropped as infeasible, [2] evaluations, [3] leaf LPs solved,
 * [4] simplex iterations, [5] pivots, [6] device bytes held, [7] device time of the evaluations'
 * kernels in microseconds (node LPs and selection), [8] of which the selection kernels.
 */
int mipx_tree_support_stats(mipx_support *s, int64_t out[9]);
/* Free the session's device memory (syncs the stream). */
void mipx_tree_support_close(mipx_support *s);

#ifdef __cplusplus
}
#endif
#endif /* MIPX_CGLP_H */
