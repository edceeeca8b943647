/*
 * mipx_cutmig.h -- migration of open nodes between ranks in cut-round mode (included by mipx.h).
 *
 * A node of a tree with cut rounds carries a cut list: ids into its rank's append-only cut store.  Those
 * ids mean nothing on another rank, so with cut migration on, a donation also carries the cut rows
 * themselves: per record its ncut and up to kc refs, in list order (the LP row order, kept so that results
 * stay bit-exact), into a table of C rows (pi: n f64, pi0), each distinct store id of the donated nodes once.
 *
 *   C = min(rows the receiver's region can still take (record [13]), 16384, amount x kc)
 *
 * so the table of one message is at most 16384 x (n + 1) x 8 bytes (33.7 MB at n = 256).  The donor picks
 * its candidates as without cut rounds (every second of its best 2 x amount open nodes); in that order a
 * node travels if the distinct rows it adds still fit in C, else it stays and goes back into the queue (a
 * node without cut rows always fits).  The receiver appends the table to its MIGRATION REGION, the top
 * `rows` rows of its cut store, [store_capacity - rows, store_capacity), in order; the nodes' lists point
 * there.  A row received twice (in two donations) is stored twice: it costs region rows.
 *
 * Nodes move in cut mode only when every rank has cut migration on with the same kc (records [14], [15]:
 * mipx.h, mipx_exchange_decide); a rank with it off and a peer with it on exchange no node.
 */
#ifndef MIPX_CUTMIG_H
#define MIPX_CUTMIG_H

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Opt-in cut migration (rows > 0; 0 turns it off, the default).  rows > 0 reserves the top `rows` rows of
 * the existing cut store for cut rows received from other ranks (no new allocation).  The rank's own cuts
 * then stop at store_capacity - rows: K3 drops a cut once that smaller cap is reached, the existing "store
 * is full" behaviour (mipx_tree_cut_stats [7], dropped) reached sooner.  mipx_tree_cut_store returns the
 * rank's own appends only, clamped at that cap.  MIPX_EINVAL: the tree runs no cut rounds, a step is in
 * flight, rows < 0, rows >= store_capacity, the store already holds more than store_capacity - rows cuts, or
 * the region (once rows have been received into it) would change.
 */
int mipx_tree_set_cut_migration(mipx_tree *t, int64_t rows);
/* Test hook: pi (count x n) and pi0 (count) of the cut store rows `ids`, own or migrated (HOST buffers; either
 * output may be NULL).  MIPX_EINVAL for an id outside [0, store_capacity). */
int mipx_tree_cut_rows(mipx_tree *t, int64_t count, const int32_t *ids, double *pi, double *pi0);
/* [0] nodes sent with cut rows, [1] cut rows sent, [2] cut rows received, [3] region rows used. */
int mipx_tree_cut_migration_stats(mipx_tree *t, int64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* MIPX_CUTMIG_H */
