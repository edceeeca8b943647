"""What the cube search (include/mipx_cube.h) costs and buys, one JSON line per run.

Kernel: device time of one mipx_cube_search_batch call per point against k, for k from 8 to 20, on the generator's
instances at 40 x 20, 144 x 72 and 256 x 128.  The points are node LP points (scripts/fix_propagate_profile.lp_points)
on which integral columns are moved half a unit off (down where there is room) until a point has k columns off their integers, so that the cap
K = k is reached at every size; the time is the shortest of five calls over 64 points, staging copies included, and of
one point alone.
Searches: on the generator's instances at 40 x 20, 72 x 36 and 144 x 72, with the objective step, for the heuristic
alone, with the weighted repair and with the cube search: the share of points that ended with a feasible point of the
leg's own (FOUND for the cube), the step of the first incumbent, nodes to the proven optimum (or the time limit) and
seconds.

    python scripts/cube_search_profile.py [--limit 20] [--seeds 3] [--big-seeds 1] [--skip-kernel] [--columns 16]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from simple_mip_solver_amd import _ffi                                        # noqa: E402
from simple_mip_solver_amd.generators import random_dense_milp_arrays         # noqa: E402
from fix_propagate_profile import lp_points                                   # noqa: E402

CONFIGS = [('heuristic + step', dict()),
           ('heuristic + weighted + step', dict(weighted_repair=True)),
           ('heuristic + cube + step', dict(cube_search=True)),
           ('heuristic + cube + local search + step', dict(cube_search=True, local_search=True))]


def timed(ctx, call, repeats=5):
    """The call's result and the shortest of `repeats` device times in ms (the first call warms the staging buffers)."""
    call()
    best = None
    for _ in range(repeats):
        ctx.timer_start()
        out = call()
        ms = ctx.timer_stop()
        best = ms if best is None else min(best, ms)
    return out, best


def with_fractional(X, l, u, ints, k, seed):
    """X with integral integer columns moved half a unit off (inside the bounds) until every point has k columns off
    their integers, where it has that many columns to move."""
    rng = np.random.default_rng(seed)
    J = np.asarray(ints, dtype=np.int64)
    X = X.copy()
    for x in X:
        f = np.abs(x[J] - np.floor(x[J] + 0.5))
        short = k - int((f > 1e-4).sum())
        free = J[(f <= 1e-4) & ((x[J] - 1.0 >= l[J]) | (x[J] + 1.0 <= u[J]))]
        if short > 0 and free.size:
            pick = rng.choice(free, size=min(short, free.size), replace=False)
            x[pick] += np.where(x[pick] - 1.0 >= l[pick], -0.5, 0.5)   # (down where there is room, else up: the floor stays)
    return X


def run_kernel(ctx, n, m, seed, ks):
    A, b, c, l, u, ints = random_dense_milp_arrays(n, m, seed=seed)
    p = _ffi.Problem(ctx, A, b, c)
    X0 = lp_points(p, l, u, ints, 64, seed)
    for k in ks:
        X = with_fractional(X0, l, u, ints, k, seed)
        out, ms = timed(ctx, lambda: p.cube_search_batch(X, l, u, ints, max_columns=k))
        one, one_ms = timed(ctx, lambda: p.cube_search_batch(X[:1], l, u, ints, max_columns=k))
        yield dict(what='kernel', n=n, m=m, K=k, points=len(X), k_mean=float(out['counts'][:, 0].mean()),
                   k_min=int(out['counts'][:, 0].min()), found=int((out['status'] == 0).sum()), launch_ms=ms,
                   us_per_point=1000.0 * ms / len(X), one_point_ms=one_ms)
    p.close()


def run_search(ctx, name, arrays, batch, pool_log2, what, opts, limit, columns):
    A, b, c, l, u, ints = arrays
    p = _ffi.Problem(ctx, A, b, c)
    t = _ffi.Tree(p, ints, l, u, branch_rule='pseudo cost', max_batch=batch, pool_capacity=1 << pool_log2)
    t.set_anchor_mode(True)
    t.set_dive(True)
    t.set_heuristic(True)
    if opts.get('weighted_repair'):
        t.set_weighted_repair(True)
    if opts.get('cube_search'):
        t.set_cube_search(columns)
    if opts.get('local_search'):
        t.set_local_search(True)
    t.set_objective_step(1.0)
    t0 = time.perf_counter()
    first = None
    s = t.solve(mip_gap=0.0, frontier_batch=batch, max_steps=1)
    while s['status'] == 4 and time.perf_counter() - t0 < limit:   # (step by step until an incumbent, then to the end)
        if first is None and np.isfinite(s['primal_bound']):
            first = s['steps']
            s = t.solve(mip_gap=0.0, frontier_batch=batch, max_seconds=max(0.1, limit - (time.perf_counter() - t0)))
            break
        s = t.solve(mip_gap=0.0, frontier_batch=batch, max_steps=1)
    if first is None and np.isfinite(s['primal_bound']):
        first = s['steps']
    h = t.heuristic_stats()
    out = dict(instance=name, what='search', configuration=what, status=_ffi.TREE_STATUS[s['status']],
               seconds=time.perf_counter() - t0, steps=s['steps'], steps_to_first_incumbent=first, nodes=s['evaluated_nodes'],
               primal=s['primal_bound'], dual=s['dual_bound'], heuristic=h,
               rounding_feasible_share=h['feasible'] / h['points'] if h['points'] else None)
    if opts.get('weighted_repair'):
        f = t.weighted_repair_stats()
        out['weighted_repair'] = dict(f, kernel_us_per_point=f['kernel_us'] / f['points'] if f['points'] else None,
                                      feasible_share=f['feasible'] / f['points'] if f['points'] else None)
    if opts.get('cube_search'):
        f = t.cube_search_stats()
        out['cube_search'] = dict(f, kernel_us_per_point=f['kernel_us'] / f['points'] if f['points'] else None,
                                  found_share=f['found'] / f['points'] if f['points'] else None,
                                  k_mean=f['columns'] / f['points'] if f['points'] else None)
    if opts.get('local_search'):
        out['local_search'] = t.local_search_stats()
    t.close()
    p.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--limit', type=float, default=20.0)
    ap.add_argument('--seeds', type=int, default=3)
    ap.add_argument('--big-seeds', type=int, default=1)
    ap.add_argument('--columns', type=int, default=_ffi.DEFAULT_CUBE_SEARCH_COLUMNS)
    ap.add_argument('--skip-kernel', action='store_true')
    ap.add_argument('--skip-search', action='store_true')
    args = ap.parse_args()
    ctx = _ffi.default_context()
    if not args.skip_kernel:
        for n, m in ((40, 20), (144, 72), (256, 128)):
            for line in run_kernel(ctx, n, m, 0, range(8, 21)):
                print(json.dumps(line), flush=True)
    if not args.skip_search:
        families = [('generator 40 x 20 seed %d' % s, random_dense_milp_arrays(40, 20, seed=s), 64, 16) for s in range(args.seeds)]
        families += [('generator 72 x 36 seed %d' % s, random_dense_milp_arrays(72, 36, seed=s), 256, 20) for s in range(args.seeds)]
        families += [('generator 144 x 72 seed %d' % s, random_dense_milp_arrays(144, 72, seed=s), 1024, 21) for s in range(args.big_seeds)]
        for name, arrays, batch, pool_log2 in families:
            for what, opts in CONFIGS:
                print(json.dumps(run_search(ctx, name, arrays, batch, pool_log2, what, opts, args.limit, args.columns)), flush=True)


if __name__ == '__main__':
    main()
