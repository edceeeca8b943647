"""Cost of the dual function (include/mipx_dualfn.h) on a frontier-engine search: per-step time of a search
with and without recording, and the evaluation time for K right-hand sides against a numpy restatement of
the same formula on the copied-out records.  Prints one JSON line.

    python3 scripts/dual_function_profile.py [n m B dive steps]     (default: C3, 256 128 8192 8 10)
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from simple_mip_solver_amd import _ffi  # noqa: E402
from simple_mip_solver_amd.generators import random_dense_milp_arrays  # noqa: E402

n, m, B, dive, steps = (int(a) for a in (sys.argv[1:6] + ['256', '128', '8192', '8', '10'][len(sys.argv[1:6]):]))
ctx = _ffi.default_context()
A, b, c, l, u, ints = random_dense_milp_arrays(n, m, seed=0)
pool = max(1 << 16, 3 * B * (2 * (1 + dive) + 1) * 8)


def run(record):
    p = _ffi.Problem(ctx, A, b, c)
    t = _ffi.Tree(p, ints, l, u, branch_rule='pseudo cost', max_batch=B, pool_capacity=pool)
    t.set_anchor_mode(True)
    t.set_dive(dive)
    if record:
        t.set_dual_record(-1, m, np.arange(m), np.ones(m))
    st = t.stats()
    while st['open_nodes'] < B and st['status'] in (0, 4):   # ramp-up as the bench's: up to a full batch
        st = t.solve(mip_gap=0.0, frontier_batch=min(B, 256), max_steps=1)
    ctx.sync()
    t0 = time.perf_counter()
    st2 = t.solve(mip_gap=0.0, frontier_batch=B, max_steps=steps)
    ctx.sync()
    dt = time.perf_counter() - t0
    return p, t, dict(ms_per_step=1e3 * dt / steps, lps=st2['lp_solved'] - st['lp_solved'])


out = {'n': n, 'm': m, 'B': B, 'dive': dive, 'steps': steps}
p0, t0_, off = run(False)
t0_.close(); p0.close()
p1, t1, on = run(True)
out['search_off'], out['search_on'] = off, on
out['record_overhead_pct'] = 100.0 * (on['ms_per_step'] / off['ms_per_step'] - 1.0)
rng = np.random.default_rng(0)
recs = t1.dual_records()
Y, T = recs['y'], recs['t']
out['stats_after_search'] = t1.dual_function_stats()
out['y_nonzero_fraction'] = float(np.count_nonzero(Y)) / max(1, Y.size)   # (what a compact store would keep)
# lineage over the records (numpy): each record's nearest recorded ancestor is its parent's record
rec_of = {int(k): i for i, k in enumerate(recs['node'])}
prec = np.array([rec_of.get(int(pa), -1) for pa in recs['parent']])
has_child = np.zeros(len(T), bool)
has_child[prec[prec >= 0]] = True
level = np.zeros(len(T), np.int64)
for r in range(len(T)):   # records come after their ancestors
    if prec[r] >= 0:
        level[r] = level[prec[r]] + 1
by_level = [np.flatnonzero(level == L) for L in range(1, int(level.max(initial=0)) + 1)]
evals = {}
for K in (1, 64, 1024):
    W = b[None] + rng.uniform(-1, 1, (K, m))
    t1.dual_function(W[:1], 1e9)   # (the penalised re-solves and the lineage arrays, once)
    g0 = time.perf_counter()
    f = t1.dual_function(W, 1e9)
    g = time.perf_counter() - g0
    h0 = time.perf_counter()
    fn = np.empty(K)
    for k0 in range(0, K, 64):   # (V of 64 right-hand sides at a time)
        V = Y @ W[k0:k0 + 64].T + T[:, None]
        for idx in by_level:
            V[idx] = np.maximum(V[idx], V[prec[idx]])
        fn[k0:k0 + 64] = V[~has_child].min(axis=0)
    h = time.perf_counter() - h0
    evals[K] = {'gpu_ms': 1e3 * g, 'numpy_ms': 1e3 * h, 'finite': bool(np.all(np.isfinite(f))),
                'max_abs_gap_vs_numpy_records_only': float(np.max(np.abs(f - fn))) if np.all(np.isfinite(f)) else None}
out['eval'] = evals
out['stats'] = t1.dual_function_stats()
print(json.dumps(out))
t1.close(); p1.close()
