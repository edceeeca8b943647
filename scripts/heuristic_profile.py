"""What the primal heuristic (include/mipx_heur.h) does to the search of section 5: the
two-phase schedule (depth first for an incumbent, then best first on a fresh tree with the incumbent installed) on
the bench's 256 x 128 seed-0 instance and on 144 x 72, in three legs each: the option off (device finish), the
option off with every step finished on the host (MIPX_HOST_FINISH=1: what the option's switch alone costs), and
the option on.  Per leg: time and node count of the first incumbent, the incumbent after 0.2 s of search and at the
end, the bounds at the end, and the heuristic kernel's device time per step it ran in.  One JSON line per leg.

    python scripts/heuristic_profile.py [--dfs-seconds 1] [--limit 4] [--pool-log2 22] [--points 32]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from simple_mip_solver_amd import _ffi                                        # noqa: E402
from simple_mip_solver_amd.generators import random_dense_milp_arrays         # noqa: E402

INF = float('inf')


def leg(ctx, n, m, mode, args):
    A, b, c, l, u, ints = random_dense_milp_arrays(n, m, seed=0)
    p = _ffi.Problem(ctx, A, b, c)
    alloc = [0.0]
    t0 = time.perf_counter()

    def clock():   # search seconds: wall time minus the creation and freeing of the trees (bench.py's clock)
        return time.perf_counter() - t0 - alloc[0]

    def timed(fn):
        a0 = time.perf_counter()
        out = fn()
        alloc[0] += time.perf_counter() - a0
        return out

    def tree(search, batch, pool_log2, primal):
        if mode == 'host finish':
            os.environ['MIPX_HOST_FINISH'] = '1'
        try:
            t = _ffi.Tree(p, ints, l, u, branch_rule='pseudo cost', search_rule=search, max_batch=batch,
                          pool_capacity=1 << pool_log2)
        finally:
            os.environ.pop('MIPX_HOST_FINISH', None)
        t.set_anchor_mode(True)
        t.set_dive(1)
        if mode == 'heuristic':
            t.set_heuristic(args.points)
        if primal < INF:
            t.set_primal_bound(primal)
        return t

    first, at02, heur = None, None, dict.fromkeys(_ffi.HEUR_STATS_KEYS, 0)
    steps_with_kernel = 0
    nodes = 0

    def run(t, batch, until, base_nodes):
        nonlocal first, at02
        s = None
        while s is None or clock() < until:
            s = t.solve(mip_gap=1e-4, frontier_batch=batch, max_steps=2 if first is None else 5)
            if first is None and s['primal_bound'] < INF:
                first = dict(seconds=clock(), nodes=base_nodes + s['evaluated_nodes'], objective=s['primal_bound'])
            if at02 is None and clock() >= 0.2:
                at02 = dict(seconds=clock(), incumbent=None if s['primal_bound'] == INF else s['primal_bound'])
            if s['status'] != 4 or s['pool_exhausted']:
                break
        return s

    def close(t, s):
        nonlocal steps_with_kernel
        h = t.heuristic_stats()
        for k in heur:
            heur[k] += h[k]
        steps_with_kernel += s['steps'] if mode == 'heuristic' else 0
        timed(t.close)

    t = timed(lambda: tree('depth first', 1024, 21, INF))
    s = run(t, 1024, args.dfs_seconds, 0)
    nodes, pb = s['evaluated_nodes'], s['primal_bound']
    phase1 = dict(seconds=clock(), nodes=nodes, incumbent=None if pb == INF else pb)
    close(t, s)
    if s['status'] == 4:
        t = timed(lambda: tree('best first', 8192, args.pool_log2, pb))
        s = run(t, 8192, args.limit, nodes)
        nodes += s['evaluated_nodes']
        close(t, s)
    el = clock()
    p.close()
    out = dict(instance=f'{n} x {m} seed 0', leg=mode, first_incumbent=first, incumbent_at_0p2_s=at02, phase_1=phase1,
               status=_ffi.TREE_STATUS[s['status']], seconds=el, nodes=nodes, nodes_per_second=nodes / el if el > 0 else None,
               incumbent=None if s['primal_bound'] == INF else s['primal_bound'], dual_bound=s['dual_bound'],
               gap=None if s['gap'] < 0 else s['gap'], pool_exhausted=bool(s['pool_exhausted']))
    if mode == 'heuristic':
        out['heuristic'] = dict(heur, kernel_us_per_step=heur['kernel_us'] / steps_with_kernel if steps_with_kernel else None,
                                points_per_step=args.points)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dfs-seconds', type=float, default=1.0)
    ap.add_argument('--limit', type=float, default=4.0)
    ap.add_argument('--pool-log2', type=int, default=22)
    ap.add_argument('--points', type=int, default=32)
    ap.add_argument('--sizes', default='256x128,144x72')
    args = ap.parse_args()
    ctx = _ffi.default_context()
    for size in args.sizes.split(','):
        n, m = (int(v) for v in size.split('x'))
        for mode in ('off', 'host finish', 'heuristic'):
            print(json.dumps(leg(ctx, n, m, mode, args)), flush=True)


if __name__ == '__main__':
    main()
