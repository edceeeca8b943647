"""What the reduced-cost bound tightening (include/mipx_rcfix.h) costs and buys, one JSON line
per run: nodes evaluated to the proven optimum (or the time limit), seconds, and the tightening's counters with the
kernel's device time per node and per launch -- without and with the option, alone and with the primal heuristic, on
the 40 x 20 packing instances, the mixed(20, 10, 5) family and 144 x 72 instances of the generator.

    python scripts/reduced_cost_profile.py [--limit 20] [--seeds 4] [--big-seeds 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from simple_mip_solver_amd import _ffi                                        # noqa: E402
from simple_mip_solver_amd.generators import random_dense_milp_arrays         # noqa: E402


def mixed(n, m, k, seed):
    """random_dense_milp_arrays(n, m, seed) plus k covering rows C x >= d (the family of tests/support/
    propagation_reference.py)."""
    A, b, c, l, u, ints = random_dense_milp_arrays(n, m, seed=seed)
    rng = np.random.default_rng(100 + seed)
    Cm = rng.integers(1, 11, (k, n)).astype(np.float64)
    Cm = Cm * (rng.random((k, n)) < 0.3)
    d = np.floor(0.06 * Cm @ np.full(n, 10.0))
    return np.vstack([A, Cm]), np.concatenate([b, d]), c, l, u, ints


def run(ctx, arrays, batch, reduced_cost, heuristic, pool_log2, **solve):
    A, b, c, l, u, ints = arrays
    p = _ffi.Problem(ctx, A, b, c)
    t = _ffi.Tree(p, ints, l, u, branch_rule='pseudo cost', max_batch=batch, pool_capacity=1 << pool_log2)
    t.set_anchor_mode(True)
    t.set_dive(True)
    if heuristic:
        t.set_heuristic(True)
    if reduced_cost:
        t.set_reduced_cost(True)
    t0 = time.perf_counter()
    s = t.solve(mip_gap=0.0, frontier_batch=batch, **solve)
    el = time.perf_counter() - t0
    rc = t.reduced_cost_stats()
    t.close()
    p.close()
    out = dict(reduced_cost=bool(reduced_cost), primal_heuristic=bool(heuristic), status=_ffi.TREE_STATUS[s['status']],
               seconds=el, steps=s['steps'], nodes=s['evaluated_nodes'], lps=s['lp_solved'], primal=s['primal_bound'],
               dual=s['dual_bound'], node_lp_ms_per_step=s['kernel_ms'] / s['steps'] if s['steps'] else None)
    if reduced_cost:
        out['tightening'] = dict(rc, kernel_us_per_node=rc['kernel_us'] / rc['nodes'] if rc['nodes'] else None,
                                 kernel_us_per_launch=rc['kernel_us'] / rc['launches'] if rc['launches'] else None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--limit', type=float, default=20.0)
    ap.add_argument('--seeds', type=int, default=4)
    ap.add_argument('--big-seeds', type=int, default=2)
    args = ap.parse_args()
    ctx = _ffi.default_context()
    families = [('40 x 20 seed %d' % s, random_dense_milp_arrays(40, 20, seed=s)) for s in range(args.seeds)]
    families += [('mixed(20, 10, 5, %d)' % s, mixed(20, 10, 5, s)) for s in range(args.seeds)]
    families += [('144 x 72 seed %d' % s, random_dense_milp_arrays(144, 72, seed=s)) for s in range(args.big_seeds)]
    for name, arrays in families:
        big = arrays[0].shape[1] > 100
        for heuristic in (False, True):
            for reduced_cost in (False, True):
                out = run(ctx, arrays, 1024 if big else 64, reduced_cost, heuristic, 21 if big else 16, max_seconds=args.limit)
                print(json.dumps(dict(out, instance=name)), flush=True)


if __name__ == '__main__':
    main()
