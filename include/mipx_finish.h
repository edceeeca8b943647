/*
 * mipx_finish.h -- the device finish of a frontier step, run on a caller's data (included by mipx.h).
 *
 * TEST SCAFFOLDING in the library, as mipx_debug_enable is: no product code calls these entries.  The kernels of
 * csrc/finish_kernels.hip.h end every batched step without cut rounds, and nothing but a whole search reaches them;
 * these two entries run them on a synthetic step, through the same function the engine launches them with
 * (enqueue_finish in csrc/tree_engine.hip.h: the same kernels, grids and dispatch on n), so that every decision can
 * be compared with a plain restatement of the reference's loop (tests/support/finish_reference.py,
 * tests/test_finish_kernels_gpu.py).
 *
 * A step has B chains; chain k is the node at output position k and the children solved in place below it, at the
 * positions k + B, k + 2 B, ... up to level `dive`.  P = (dive + 1) B positions, per = 2 (1 + dive) pool rows a chain
 * may take.  INPUT CONTRACT: obj does not decrease down a chain wherever the child counts (status >= 0 and nprobe = 0
 * at the child's position), as the LP values of a plunge do.
 */
#ifndef MIPX_FINISH_H
#define MIPX_FINISH_H

#ifdef __cplusplus
extern "C" {
#endif

/*
 * One device finish on host buffers.  Inputs:
 *   out_i     7 x P int32: status | bidx | mipf | nprobe | npiv | dvar | ddir  (what K1 and K4 wrote)
 *   out_d     3 x P f64:   obj | bval | dval
 *   vout      P x (n + m) int8: the basis every LP ended with
 *   slot      B int32: the pool rows of the batch
 *   par_i     4 x B int32: b_idx | b_dir | depth | anchor of the batch's nodes;  par_d  2 x B f64: dual_bound | b_val
 *   budget    B x per int32: the pool rows chain k's children may take (level p, direction d: budget[k][2 p + d])
 *   ask_count, ask_cap: K4's request counter and the length of its compact list (ask_count > ask_cap: the step is
 *             the host's; host_path = 1 in the summary and nothing else is written)
 * In and out (uploaded, then copied back whatever the kernels wrote, so that a caller's sentinels show what they
 * left alone):
 *   pool_l, pool_u   pool_rows x n f64;  pool_v  pool_rows x (n + m) int8
 *   primal    1 f64: the incumbent value
 *   cost_l, cost_r (n f64), has (n bytes), times (2 n int32: left | right), own (4 n f64: sum_l | sum_r | times_l |
 *             times_r): the pseudo-cost table; read and written with rule = 1 only, and may be null otherwise
 *   summary   128 bytes (FinishSummary of csrc/finish_records.h);  open  per x B records of 32 bytes (OpenEntry);
 *   dead      per x B int32;  samples  P records of 32 bytes (PcSample) and sample_keys  P int32: with rule = 1
 *             only, and may be null otherwise
 * MIPX_EINVAL: a null argument, B < 1, dive outside 0..8, n outside 1..1024, m < 0, rule outside 0..1, pool_rows < 1,
 * a slot or budget row outside the pool.
 */
int mipx_finish_step_batch(mipx_ctx *ctx, int n, int m, int B, int dive, int rule, int ask_count, int ask_cap,
                           const int32_t *out_i, const double *out_d, const int8_t *vout, const int32_t *slot,
                           const int32_t *par_i, const double *par_d, const int32_t *budget, int pool_rows,
                           double *pool_l, double *pool_u, int8_t *pool_v, double *primal, double *cost_l,
                           double *cost_r, uint8_t *has, int32_t *times, double *own, void *summary, void *open,
                           int32_t *dead, void *samples, int32_t *sample_keys);
/*
 * The pseudo-cost recurrence alone, on `count` host-sent samples (the way in that a step finished by the host
 * takes): samples  count records of 32 bytes, keys  their var_dir again, densely; the table as above, in and out.
 * MIPX_EINVAL: a null table, n outside 1..1024, count < 0, null samples or keys with count > 0.
 */
int mipx_pc_apply_batch(mipx_ctx *ctx, int n, int count, const void *samples, const int32_t *keys, double *cost_l,
                        double *cost_r, uint8_t *has, int32_t *times, double *own);

#ifdef __cplusplus
}
#endif
#endif /* MIPX_FINISH_H */
