/*
 * mipx_clique.h -- clique cuts on the GPU: a conflict graph from the rows of the problem and batched greedy separation
 * (included by mipx.h).
 *
 * The MIR cuts of mipx_mir.h round a row, the cover cuts of mipx_cover.h use the 0/1 structure of one row.  A clique
 * cut combines the 0/1 structure of several rows: where the rows say, pair by pair, that no two of a set of literals
 * can be 1 together, at most one of the whole set is.  This header states the graph and the separation of one cut; the
 * root loop that uses them is Python (simple_mip_solver_amd/utils/mir_cuts.py root_cut_loop(clique=True)), and the
 * stand-alone entries are in simple_mip_solver_amd/utils/clique_cuts.py.
 *
 * LITERALS.  Column j of n gives literal 2j, of value y = x_j - l_j, and literal 2j + 1, its complement, of value
 *          y = u_j - x_j.  BINARY is that of mipx_cover.h (in int_idx, u_j finite, l_j and u_j integers,
 *          u_j - l_j = 1 exactly).  A literal is LIVE when its column is binary in the box (l, u); there is one box
 *          per call, n entries each for l and u.  The adjacency has 2n rows of Wd = ceil(2n / 32) uint32_t words;
 *          literal k is bit k mod 32 of word k div 32.
 * GRAPH.   From the problem's m rows and the box.  Every row i is taken in the KNAPSACK FORM of mipx_cover.h,
 *          unchanged: g = 0 - a_i, d = 0 - b_i, the items, their weights w, W = d - K with the BLOCK SUM K, and
 *          tau = 1e-9 * max(1, |W|) as defined there; a row is skipped (row status 4) under the same two conditions
 *          (a column that is not binary needs an infinite bound; W is not >= 0).  An item with g_j > 0 is literal 2j,
 *          one with g_j < 0 literal 2j + 1.  Two different items e, f of one row CONFLICT when
 *          (w_e + w_f) - W > tau: one addition, one subtraction, one comparison, as written.  Bit (k, h) of the
 *          adjacency is set exactly when some row makes the literals k and h conflict.  a + b = b + a, so the matrix
 *          is symmetric; a row holds a column once, so a literal is never joined to itself or to its own complement;
 *          the rows of literals that are not live and the bits at 2n and above are 0.  The result is a set: it does
 *          not depend on the order of the work.  Outputs: the adjacency and a status per row (0 used, 4 skipped).
 * SEPARATION.  One cut from a point x*, the box, an adjacency and a seed literal s.  y*_k is the value of literal k at
 *          x*, clipped to [0, 1], and 0 for a literal that is not live.  Status 4 if s is not live; status 1 unless
 *          y*_s > 0.  Q = {s}, C = the live literals of adj[s] without s.  While C is not empty: t is the literal of C
 *          with the largest y*, ties to the smallest literal number; Q gains t; C becomes C and adj[t] without t.
 *          Literals of value 0 come last, so the clique ends maximal among the live literals: that is the lifting.
 *          |Q| < 2: status 1.  The cut is the sum of y_k over Q <= 1.  Only comparisons decide Q, so it does not
 *          depend on how the maximum is reduced.
 * OUTPUT.  As pi . x >= pi0, the project's convention: pi_j = 0 - 1 for literal 2j in Q, 1 for literal 2j + 1 in Q,
 *          0 otherwise; pi0 = T - 1, with T, the efficacy (pi0 - V) / sqrt(Qn) and the BLOCK SUMs T, V, Qn over the n
 *          columns exactly as in OUTPUT of mipx_cover.h (Qn = |Q| there).  Every term is an integer, so pi and pi0 are
 *          exact.  Status, the first that applies:
 *            4  skipped (the seed is not live);
 *            1  no clique (y*_s is not positive, or the seed has no live neighbour);
 *            2  efficacy <= min_efficacy (or not a number);
 *            0  a cut.
 *          With status 1 or 4 every output of the seed is 0; with 0 and 2 the seed's pi, pi0, efficacy and |Q| are
 *          written.
 *
 * VALIDITY.  An edge between two literals means that some row of the problem, with every other column at the bound
 *          that helps the row most inside the box, cannot hold both literals at 1: their weights exceed the capacity W
 *          by more than tau, a margin far above the rounding error of the sums involved.  So no point of the box that
 *          satisfies the rows has both at 1, and of the literals of a clique, joined pair by pair, at most one is 1:
 *          the sum of their values, each 0 or 1 at an integer point, is at most 1.  A literal and its complement are
 *          never joined, so Q holds a column at most once and |Q| <= n.  The graph is valid for the box it was built
 *          from and for every box inside it: with the model's own box a cut is valid for the model.  An adjacency
 *          handed in from elsewhere is the caller's claim; the entry checks only its form.
 * ARITHMETIC.  Nothing is fused (the library is built with -ffp-contract=off).  clique_graph runs one workgroup of 256
 *          threads per row, through the device code of the knapsack form that cover_separate uses, and sets the bits
 *          with integer atomic OR, which has no order to depend on.  clique_separate runs one workgroup of 256 threads
 *          (4 waves of 64) per (point, seed).  tests/support/clique_reference.py restates all of it in NumPy.
 */
#ifndef MIPX_CLIQUE_H
#define MIPX_CLIQUE_H

#ifdef __cplusplus
extern "C" {
#endif

#define MIPX_CLIQUE_CUT 0
#define MIPX_CLIQUE_NO_CLIQUE 1
#define MIPX_CLIQUE_SHALLOW 2
#define MIPX_CLIQUE_SKIPPED 4

/*
 * Host buffers.  l, u: n entries, one box; int_idx: n_int distinct columns.  adj_out: 2n x Wd words, every one of them
 * written; row_status_out: m entries, or NULL.  One launch of m workgroups; its device time is what
 * mipx_last_kernel_ms returns afterwards.
 * MIPX_EINVAL: a null or out-of-range argument, int_idx out of range or repeated, an l that is not finite, a u that is
 * NaN or -inf; MIPX_ETOOBIG: m or n above 1024.
 */
int mipx_clique_graph(mipx_problem *p, const double *l, const double *u, const int32_t *int_idx, int n_int,
                      uint32_t *adj_out, int32_t *row_status_out);

/*
 * Host buffers, one launch of batch x R workgroups, R = n_seeds with seeds (n_seeds distinct literals in [0, 2n),
 * shared by the points) or 2n with seeds = NULL.  x: batch x n; l, u: n entries, one box; adj: 2n x Wd words.
 * pi_out: batch x R x n; pi0_out, efficacy_out, size_out, status_out: batch x R.
 * Bits of adj at 2n and above, and the rows and bits of literals that are not live in the box, are ignored: the
 * kernel masks them, and the check below does not look at them.
 * MIPX_EINVAL: a null or out-of-range argument, n_seeds < 0 (or 0 seeds with batch > 0), a NaN min_efficacy, int_idx
 * or seeds out of range or repeated, an x or l that is not finite, a u that is NaN or -inf, and an adj that, among the
 * live literals, is not symmetric, has a diagonal bit, or joins the two literals of one column (a host check over the
 * 2n x Wd words); MIPX_ETOOBIG: m or n above 1024.
 */
int mipx_clique_separate_batch(mipx_problem *p, int batch, const double *x, const double *l, const double *u,
                               const int32_t *int_idx, int n_int, const uint32_t *adj, const int32_t *seeds,
                               int n_seeds, double min_efficacy, double *pi_out, double *pi0_out,
                               double *efficacy_out, int32_t *size_out, int32_t *status_out);

#ifdef __cplusplus
}
#endif
#endif /* MIPX_CLIQUE_H */
