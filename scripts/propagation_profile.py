"""What the bound propagation (include/mipx_prop.h) costs and buys, one JSON line per leg:

  bench     the bench's instance (256 x 128 seed 0, frontier_batch 8192, the primal heuristic on) for a number of
            steps: the propagation kernel's device time per step beside the node-LP launch time (kernel_ms), the
            nodes it tightened and proved infeasible;
  closing   144 x 72 instances of the generator and the packing + covering family, searched to the proven optimum
            (or the time limit) without and with the option: nodes evaluated, seconds, the propagation's counters.

    python scripts/propagation_profile.py [--steps 40] [--limit 20] [--seeds 3] [--rounds 8]
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


def run(ctx, arrays, batch, propagate, heuristic, rounds, pool_log2, **solve):
    A, b, c, l, u, ints = arrays
    p = _ffi.Problem(ctx, A, b, c)
    t = _ffi.Tree(p, ints, l, u, branch_rule='pseudo cost', max_batch=batch, pool_capacity=1 << pool_log2)
    t.set_anchor_mode(True)
    t.set_dive(True)
    if heuristic:
        t.set_heuristic(True)
    if propagate:
        t.set_propagation(rounds)
    t0 = time.perf_counter()
    s = t.solve(mip_gap=0.0, frontier_batch=batch, **solve)
    el = time.perf_counter() - t0
    pg = t.propagation_stats()
    t.close()
    p.close()
    out = dict(propagate=bool(propagate), status=_ffi.TREE_STATUS[s['status']], seconds=el, steps=s['steps'],
               nodes=s['evaluated_nodes'], lps=s['lp_solved'], primal=s['primal_bound'], dual=s['dual_bound'],
               node_lp_ms_per_step=s['kernel_ms'] / s['steps'] if s['steps'] else None)
    if propagate:
        out['propagation'] = dict(pg, kernel_us_per_step=pg['kernel_us'] / s['steps'] if s['steps'] else None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--limit', type=float, default=20.0)
    ap.add_argument('--seeds', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=8)
    args = ap.parse_args()
    ctx = _ffi.default_context()
    arrays = random_dense_milp_arrays(256, 128, seed=0)
    for propagate in (False, True):
        out = run(ctx, arrays, 8192, propagate, True, args.rounds, 22, max_steps=args.steps)
        print(json.dumps(dict(out, leg='bench', instance='256 x 128 seed 0, frontier_batch 8192, primal heuristic')), flush=True)
    families = [('144 x 72 seed %d' % s, random_dense_milp_arrays(144, 72, seed=s)) for s in range(args.seeds)]
    families += [('mixed(40, 20, 10, %d)' % s, mixed(40, 20, 10, s)) for s in range(args.seeds)]
    families += [('mixed(20, 10, 5, %d)' % s, mixed(20, 10, 5, s)) for s in range(args.seeds)]
    for name, arrays in families:
        for propagate in (False, True):
            out = run(ctx, arrays, 1024 if arrays[0].shape[1] > 100 else 64, propagate, True, args.rounds, 21,
                      max_seconds=args.limit)
            print(json.dumps(dict(out, leg='closing', instance=name)), flush=True)


if __name__ == '__main__':
    main()
