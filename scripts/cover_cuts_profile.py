"""What the lifted cover cuts at the root (include/mipx_cover.h) cost and buy, one JSON line per
leg:

  closing   the sparse knapsack family (generators.sparse_knapsack_milp_arrays) at 16 x 8 x 6, 40 x 20 x 8, 64 x 32 x 10
            and 144 x 72 x 12, searched to the proven optimum (or the time limit) plain, with root_cuts and with
            root_cuts + cover_cuts, once alone and once beside primal_heuristic + objective_step + reduced_cost: the
            root gap closed (against the optimum a search proves), nodes evaluated, seconds, the counters of both cut
            families, the device time per separated row of both kernels, and whether the rows kept move the node LPs
            to another kernel (a K1 row tile crossed);
  kernel    the two separation kernels on the same root LP points, 64 copies in a batch, at 40, 144 and 256 columns:
            device time per separated row.

The comparison is always against the same search without the option.  Single runs.

    python scripts/cover_cuts_profile.py [--limit 20] [--seeds 2] [--rounds 10] [--rows 64] [--skip-kernel]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from simple_mip_solver_amd import BranchAndBound, MILPInstance, PseudoCostBranchNode, _ffi   # noqa: E402
from simple_mip_solver_amd.generators import sparse_knapsack_milp_arrays                    # noqa: E402
from simple_mip_solver_amd.utils.mir_cuts import row_integral_flags                         # noqa: E402

SIZES = ((16, 8, 6), (40, 20, 8), (64, 32, 10), (144, 72, 12))


def run(arrays, batch, limit, root_cuts, cover, rows, others):
    A, b, c, l, u, ints = arrays
    mdl = MILPInstance(A=A, b=b, c=c, l=l, u=u, sense=['Min', '>='], integerIndices=ints, numVars=len(c))
    extra = dict(primal_heuristic=True, objective_step=True, reduced_cost=True) if others else {}
    if root_cuts:
        extra.update(root_cuts=root_cuts, root_cut_rows=rows)
    if cover:
        extra.update(cover_cuts=True)
    t0 = time.perf_counter()
    bb = BranchAndBound(mdl, PseudoCostBranchNode, pseudo_costs={}, gomory_cuts=False, mip_gap=0.0, frontier_batch=batch,
                        max_run_time=limit, pool_capacity=1 << 21, **extra)
    bb.solve()
    wall = time.perf_counter() - t0
    st = bb._native_stats
    out = dict(root_cuts=bool(root_cuts), cover_cuts=bool(cover), others=bool(others), status=bb.status, wall_seconds=wall,
               search_seconds=bb.solve_time, nodes=bb.evaluated_nodes, steps=st['steps'], primal=bb.primal_bound,
               dual=st['dual_bound'], node_lp_ms_per_step=st['kernel_ms'] / st['steps'] if st['steps'] else None)
    if root_cuts:
        rc = bb.root_cut_stats
        m, n = A.shape
        kept = len(bb.root_cuts)
        out['root_cut_stats'] = rc
        out['rows'] = m + kept
        out['node_lp_kernel'] = [_ffi.kernel_name(m, n), _ffi.kernel_name(m + kept, n)]
        out['tile_crossed'] = out['node_lp_kernel'][0] != out['node_lp_kernel'][1]
        out['mir_us_per_row'] = rc['kernel_us'] / rc['base_rows'] if rc['base_rows'] else None
    if cover:
        cs = bb.cover_cut_stats
        out['cover_cut_stats'] = cs
        out['cover_us_per_row'] = cs['kernel_us'] / cs['rows'] if cs['rows'] else None
    return out


def kernels(n, m, k, copies=64, repeats=5):
    """Both kernels on the root LP point of one instance, `copies` times in a batch: device microseconds per row."""
    A, b, c, l, u, ints = sparse_knapsack_milp_arrays(n, m, k, seed=0)
    p = _ffi.Problem(_ffi.default_context(), A, b, c)
    x = p.solve_batch(l[None], u[None])['x'][0]
    X, L, U = np.tile(x, (copies, 1)), np.tile(l, (copies, 1)), np.tile(u, (copies, 1))
    flags = row_integral_flags(A, b, ints)
    mir, cov = [], []
    for _ in range(repeats + 1):   # (alternating; the first pair warms up)
        mir.append(p.mir_separate_batch(X, L, U, ints, flags)['kernel_us'] / (copies * m))
        res = p.cover_separate_batch(X, L, U, ints)
        cov.append(res['kernel_us'] / (copies * m))
    p.close()
    return dict(leg='kernel', instance='%d x %d x %d' % (n, m, k), rows=copies * m, mir_us_per_row=sorted(mir[1:]),
                cover_us_per_row=sorted(cov[1:]), covers_found=int(np.sum(res['status'][0] == 0)),
                largest_cover=int(res['cover_size'].max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--limit', type=float, default=20.0)
    ap.add_argument('--seeds', type=int, default=2)
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--rows', type=int, default=64)
    ap.add_argument('--skip-kernel', action='store_true')
    args = ap.parse_args()
    if not args.skip_kernel:
        for n, m, k in ((40, 20, 8), (144, 72, 12), (256, 128, 12), (256, 128, 128)):
            print(json.dumps(kernels(n, m, k)), flush=True)
    for n, m, k in SIZES:
        for seed in range(args.seeds):
            arrays = sparse_knapsack_milp_arrays(n, m, k, seed=seed)
            batch = 1024 if n > 100 else 64
            for others in (False, True):
                legs = [run(arrays, batch, args.limit, None, False, args.rows, others),
                        run(arrays, batch, args.limit, args.rounds, False, args.rows, others),
                        run(arrays, batch, args.limit, args.rounds, True, args.rows, others)]
                proven = [out['primal'] for out in legs if out['status'] == 'optimal']
                for out in legs[1:]:
                    rc = out['root_cut_stats']
                    if proven and rc['bound_before'] is not None and proven[0] > rc['bound_before']:
                        out['root_gap_closed'] = (rc['bound_after'] - rc['bound_before']) / (proven[0] - rc['bound_before'])
                for out in legs:
                    print(json.dumps(dict(out, leg='closing', instance='%d x %d x %d seed %d' % (n, m, k, seed))), flush=True)


if __name__ == '__main__':
    main()
