"""What the root MIR cuts (include/mipx_mir.h) cost and buy, one JSON line per leg:

  closing   instances of the generator at 40 x 20, 64 x 32 and 144 x 72 and of the packing + covering family, searched to
            the proven optimum (or the time limit) without and with root_cuts, once alone and once beside
            primal_heuristic + objective_step + reduced_cost: the root gap closed (against the optimum the plain search
            proves), nodes evaluated, seconds, the loop's counters and the kernel's device time per separated row;
  tile      256 x 128 (the m = 128 tile of the node-LP kernel): the same comparison where the cut rows move the search
            to the 192-row tile, with the node-LP time per step of both.

The comparison is always against the same search without the option.

    python scripts/root_cuts_profile.py [--limit 20] [--seeds 3] [--rounds 10] [--rows 64] [--skip-tile]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from simple_mip_solver_amd import BranchAndBound, MILPInstance, PseudoCostBranchNode   # noqa: E402
from simple_mip_solver_amd.generators import random_dense_milp_arrays                    # noqa: E402


def mixed(n, m, k, seed):
    """random_dense_milp_arrays(n, m, seed) plus k covering rows C x >= d (the family of tests/support/
    propagation_reference.py)."""
    A, b, c, l, u, ints = random_dense_milp_arrays(n, m, seed=seed)
    rng = np.random.default_rng(100 + seed)
    Cm = rng.integers(1, 11, (k, n)).astype(np.float64)
    Cm = Cm * (rng.random((k, n)) < 0.3)
    d = np.floor(0.06 * Cm @ np.full(n, 10.0))
    return np.vstack([A, Cm]), np.concatenate([b, d]), c, l, u, ints


def run(arrays, batch, limit, root_cuts, rows, others):
    A, b, c, l, u, ints = arrays
    mdl = MILPInstance(A=A, b=b, c=c, l=l, u=u, sense=['Min', '>='], integerIndices=ints, numVars=len(c))
    extra = dict(primal_heuristic=True, objective_step=True, reduced_cost=True) if others else {}
    if root_cuts:
        extra.update(root_cuts=root_cuts, root_cut_rows=rows)
    t0 = time.perf_counter()
    bb = BranchAndBound(mdl, PseudoCostBranchNode, pseudo_costs={}, gomory_cuts=False, mip_gap=0.0, frontier_batch=batch,
                        max_run_time=limit, pool_capacity=1 << 21, **extra)
    bb.solve()
    wall = time.perf_counter() - t0
    st = bb._native_stats
    out = dict(root_cuts=bool(root_cuts), others=bool(others), status=bb.status, wall_seconds=wall,
               search_seconds=bb.solve_time, nodes=bb.evaluated_nodes, steps=st['steps'], primal=bb.primal_bound,
               dual=st['dual_bound'], node_lp_ms_per_step=st['kernel_ms'] / st['steps'] if st['steps'] else None)
    if root_cuts:
        rc = bb.root_cut_stats
        out['root_cut_stats'] = rc
        out['rows'] = A.shape[0] + rc['kept']
        out['kernel_us_per_row'] = rc['kernel_us'] / rc['base_rows'] if rc['base_rows'] else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--limit', type=float, default=20.0)
    ap.add_argument('--seeds', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--rows', type=int, default=64)
    ap.add_argument('--skip-tile', action='store_true')
    args = ap.parse_args()
    families = []
    for n, m in ((40, 20), (64, 32), (144, 72)):
        families += [('%d x %d seed %d' % (n, m, s), random_dense_milp_arrays(n, m, seed=s), 'closing') for s in range(args.seeds)]
    families += [('mixed(20, 10, 5, %d)' % s, mixed(20, 10, 5, s), 'closing') for s in range(args.seeds)]
    families += [('mixed(40, 20, 10, %d)' % s, mixed(40, 20, 10, s), 'closing') for s in range(args.seeds)]
    if not args.skip_tile:
        families += [('256 x 128 seed 0', random_dense_milp_arrays(256, 128, seed=0), 'tile')]
    for name, arrays, leg in families:
        batch = 1024 if arrays[0].shape[1] > 100 else 64
        for others in (False, True):
            base = run(arrays, batch, args.limit, None, args.rows, others)
            cut = run(arrays, batch, args.limit, args.rounds, args.rows, others)
            rc = cut['root_cut_stats']
            if base['status'] == 'optimal' and rc['bound_before'] is not None and base['primal'] > rc['bound_before']:
                cut['root_gap_closed'] = (rc['bound_after'] - rc['bound_before']) / (base['primal'] - rc['bound_before'])
            for out in (base, cut):
                print(json.dumps(dict(out, leg=leg, instance=name)), flush=True)


if __name__ == '__main__':
    main()
