"""What the clique cuts at the root (include/mipx_clique.h) cost and buy, one JSON line per leg:

  closing   the conflict packing family (generators.conflict_packing_milp_arrays) at 24 x 70 x 4 x 8, 40 x 200 x 8 x 10
            and 60 x 450 x 8 x 12, searched to the proven optimum (or the time limit) plain, with root_cuts, with
            root_cuts + cover_cuts and with root_cuts + cover_cuts + clique_cuts: the root gap closed (against the
            optimum a search proves), nodes evaluated, seconds, the counters of the three cut families, and whether
            the rows kept move the node LPs to another kernel (a K1 row tile crossed).  Where the cuts kept fill
            root_cut_rows, the last leg is run again with --more-rows;
  graph     the device time of clique_graph at the sizes above and at 1024 x 1024, sparse (12 nonzeros a row) and dense;
  kernel    clique_separate with all 2n seeds beside cover_separate with all m rows on the same root LP points, 64
            copies in a batch, from the same build: device microseconds per seed and per row.

The comparison is always against the same search without the option.  Single runs.

    python scripts/clique_cuts_profile.py [--limit 20] [--seeds 3] [--rounds 10] [--rows 64] [--more-rows 256] [--skip-kernel]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from simple_mip_solver_amd import BranchAndBound, MILPInstance, PseudoCostBranchNode, _ffi   # noqa: E402
from simple_mip_solver_amd.generators import conflict_packing_milp_arrays                   # noqa: E402

SIZES = ((24, 70, 4, 8), (40, 200, 8, 10), (60, 450, 8, 12))


def run(arrays, batch, limit, root_cuts, cover, clique, rows):
    A, b, c, l, u, ints = arrays
    mdl = MILPInstance(A=A, b=b, c=c, l=l, u=u, sense=['Min', '>='], integerIndices=ints, numVars=len(c))
    extra = {}
    if root_cuts:
        extra.update(root_cuts=root_cuts, root_cut_rows=rows)
    if cover:
        extra.update(cover_cuts=True)
    if clique:
        extra.update(clique_cuts=True)
    t0 = time.perf_counter()
    bb = BranchAndBound(mdl, PseudoCostBranchNode, pseudo_costs={}, gomory_cuts=False, mip_gap=0.0, frontier_batch=batch,
                        max_run_time=limit, pool_capacity=1 << 21, **extra)
    bb.solve()
    wall = time.perf_counter() - t0
    st = bb._native_stats
    out = dict(root_cuts=bool(root_cuts), cover_cuts=bool(cover), clique_cuts=bool(clique), root_cut_rows=rows if root_cuts else None,
               status=bb.status, wall_seconds=wall, search_seconds=bb.solve_time, nodes=bb.evaluated_nodes, steps=st['steps'],
               primal=bb.primal_bound, dual=st['dual_bound'],
               node_lp_ms_per_step=st['kernel_ms'] / st['steps'] if st['steps'] else None)
    if root_cuts:
        m, n = A.shape
        kept = len(bb.root_cuts)
        out['root_cut_stats'] = bb.root_cut_stats
        out['rows'] = m + kept
        out['node_lp_kernel'] = [_ffi.kernel_name(m, n), _ffi.kernel_name(m + kept, n)]
        out['tile_crossed'] = out['node_lp_kernel'][0] != out['node_lp_kernel'][1]
        out['rows_bind'] = kept >= rows
    if cover:
        out['cover_cut_stats'] = bb.cover_cut_stats
    if clique:
        qs = bb.clique_cut_stats
        out['clique_cut_stats'] = qs
        out['clique_us_per_seed'] = qs['kernel_us'] / qs['seeds'] if qs['seeds'] else None
    return out


def dense_rows(n, m, seed=0):
    """m dense knapsacks over n binaries, integer weights 5..30, the capacity at 1.5 times the heaviest weight: the
    heavy pairs of every row conflict."""
    rng = np.random.Generator(np.random.PCG64(seed))
    W = rng.integers(5, 31, (m, n)).astype(np.float64)
    return -W, -np.floor(1.5 * W.max(1)), -np.ones(n), np.zeros(n), np.ones(n), list(range(n))


def graph(name, arrays, repeats=5):
    A, b, c, l, u, ints = arrays
    p = _ffi.Problem(_ffi.default_context(), A, b, c)
    us = []
    for _ in range(repeats + 1):   # (the first warms up)
        g = p.conflict_graph(l, u, ints)
        us.append(g['kernel_us'])
    p.close()
    edges = int(np.unpackbits(g['adj'].view(np.uint8)).sum()) // 2
    return dict(leg='graph', instance=name, rows=A.shape[0], columns=A.shape[1], edges=edges,
                rows_skipped=int(np.sum(g['row_status'] == 4)), graph_us=sorted(us[1:]))


def kernels(shape, copies=64, repeats=5):
    """clique_separate (2n seeds) and cover_separate (m rows) on the root LP point of one instance, `copies` times in a
    batch: device microseconds per seed and per row."""
    A, b, c, l, u, ints = conflict_packing_milp_arrays(*shape, seed=0)
    m, n = A.shape
    p = _ffi.Problem(_ffi.default_context(), A, b, c)
    x = p.solve_batch(l[None], u[None])['x'][0]
    X, L, U = np.tile(x, (copies, 1)), np.tile(l, (copies, 1)), np.tile(u, (copies, 1))
    adj = p.conflict_graph(l, u, ints)['adj']
    clq, cov = [], []
    for _ in range(repeats + 1):   # (alternating; the first pair warms up)
        res = p.clique_separate_batch(X, l, u, ints, adj)
        clq.append(res['kernel_us'] / (copies * 2 * n))
        cov.append(p.cover_separate_batch(X, L, U, ints)['kernel_us'] / (copies * m))
    p.close()
    return dict(leg='kernel', instance='%d x %d x %d x %d' % shape, seeds=copies * 2 * n, rows=copies * m,
                clique_us_per_seed=sorted(clq[1:]), cover_us_per_row=sorted(cov[1:]),
                cuts_found=int(np.sum(res['status'][0] == 0)), largest_clique=int(res['size'].max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--limit', type=float, default=20.0)
    ap.add_argument('--seeds', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--rows', type=int, default=64)
    ap.add_argument('--more-rows', type=int, default=256)
    ap.add_argument('--skip-kernel', action='store_true')
    args = ap.parse_args()
    if not args.skip_kernel:
        for shape in SIZES:
            print(json.dumps(graph('%d x %d x %d x %d' % shape, conflict_packing_milp_arrays(*shape, seed=0))), flush=True)
        print(json.dumps(graph('1024 x 1024 sparse', conflict_packing_milp_arrays(1024, 0, 1024, 12, seed=0))), flush=True)
        print(json.dumps(graph('1024 x 1024 dense', dense_rows(1024, 1024))), flush=True)
        for shape in SIZES:
            print(json.dumps(kernels(shape)), flush=True)
    for shape in SIZES:
        for seed in range(args.seeds):
            arrays = conflict_packing_milp_arrays(*shape, seed=seed)
            legs = [run(arrays, 64, args.limit, None, False, False, args.rows),
                    run(arrays, 64, args.limit, args.rounds, False, False, args.rows),
                    run(arrays, 64, args.limit, args.rounds, True, False, args.rows),
                    run(arrays, 64, args.limit, args.rounds, True, True, args.rows)]
            if legs[-1]['rows_bind']:
                legs.append(run(arrays, 64, args.limit, args.rounds, True, True, args.more_rows))
            proven = [out['primal'] for out in legs if out['status'] == 'optimal']
            for out in legs[1:]:
                rc = out['root_cut_stats']
                if proven and rc['bound_before'] is not None and proven[0] > rc['bound_before']:
                    out['root_gap_closed'] = (rc['bound_after'] - rc['bound_before']) / (proven[0] - rc['bound_before'])
            for out in legs:
                print(json.dumps(dict(out, leg='closing', instance='%d x %d x %d x %d seed %d' % (shape + (seed,)))), flush=True)


if __name__ == '__main__':
    main()
