"""What the completion over the continuous columns (include/mipx_complete.h) costs and buys, one
JSON line per run.

Families: the generator's instances with the even columns integer and the odd ones continuous ("packing"), and the
same with the first half of the rows turned into covering rows whose right-hand side is 0.8 of their activity at a
random integer point ("mixed"), at 40 x 20, 72 x 36 and 144 x 72.
Entry: 64 LP points per instance (the root's, then LPs with four random integer bounds moved to the floor or the ceil
of the root value), rounded by mipx_round_repair_batch, completed by mipx_complete_batch cold and warm from the basis of
the LP each point came from: points completed, rescued (completed where the rounding was not feasible), pivots per
completion, and the shortest of five calls' device time per point, staging copies included.
Searches: with the heuristic alone and with the completion beside it: the step and the time of the first incumbent,
nodes and seconds to the proven optimum (or the time limit), and the option's counters.

    python scripts/completion_profile.py [--limit 20] [--seeds 3] [--big-seeds 1] [--skip-entry] [--skip-search]
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


def packing(n, m, seed):
    A, b, c, l, u, _ = random_dense_milp_arrays(n, m, seed=seed)
    return A, b, c, l, u, list(range(0, n, 2))


def mixed(n, m, seed):
    A, b, c, l, u, _ = random_dense_milp_arrays(n, m, seed=seed)
    rng = np.random.default_rng(seed)
    k = m // 2
    A[:k] = -A[:k]
    xh = rng.integers(0, 4, n)
    b[:k] = np.floor(0.8 * (A[:k] @ xh))
    return A, b, c, l, u, list(range(0, n, 2))


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


def lp_points(p, l, u, ints, count, seed, moved=4):
    """(X, V) of `count` optimal LPs: the root's, then LPs with `moved` integer bounds moved to the floor or the ceil of
    the root value, warm from the root's basis; None where the root LP is not optimal."""
    root = p.solve_batch(l[None], u[None])
    if root['status'][0] != 0:
        return None
    rng = np.random.default_rng(seed)
    X, V = [root['x'][0]], [root['vstat'][0]]
    for _ in range(50):
        L, U = np.tile(l, (count, 1)), np.tile(u, (count, 1))
        for k in range(count):
            for j in rng.choice(ints, size=moved, replace=False):
                if rng.integers(0, 2):
                    U[k, j] = np.floor(root['x'][0, j])
                else:
                    L[k, j] = np.ceil(root['x'][0, j])
        r = p.solve_batch(L, U, np.repeat(root['vstat'], count, axis=0))
        for k in np.flatnonzero(r['status'] == 0):
            X.append(r['x'][k]); V.append(r['vstat'][k])
        if len(X) >= count:
            break
    return np.array(X[:count]), np.array(V[:count], dtype=np.int8)


def run_entry(ctx, family, n, m, seed, count=64):
    A, b, c, l, u, ints = (packing if family == 'packing' else mixed)(n, m, seed)
    p = _ffi.Problem(ctx, A, b, c)
    pts = lp_points(p, l, u, ints, count, seed)
    if pts is None:
        p.close()
        return dict(what='entry', family=family, n=n, m=m, seed=seed, root='not optimal')
    X, V = pts
    r = p.round_repair_batch(X, l, u, ints)
    cold, cold_ms = timed(ctx, lambda: p.complete_batch(r['x'], l, u, ints))
    warm, warm_ms = timed(ctx, lambda: p.complete_batch(r['x'], l, u, ints, vstat=V))
    one, one_ms = timed(ctx, lambda: p.complete_batch(r['x'][:1], l, u, ints, vstat=V[:1]))
    p.close()
    done = warm['status'] == 0
    frozen = r['status'] == 0
    both = done & frozen
    return dict(what='entry', family=family, n=n, m=m, seed=seed, points=len(X), frozen_feasible=int(frozen.sum()),
                completed=int(done.sum()), completed_cold=int((cold['status'] == 0).sum()), rescued=int((done & ~frozen).sum()),
                lp_infeasible=int((warm['status'] == 1).sum()), limit_or_rejected=int(np.isin(warm['status'], (2, 4)).sum()),
                mean_gain=float(np.mean(r['obj'][both] - warm['obj'][both])) if both.any() else None,
                pivots_cold=float(cold['pivots'].mean()), pivots_warm=float(warm['pivots'].mean()),
                us_per_point_cold=1000.0 * cold_ms / len(X), us_per_point_warm=1000.0 * warm_ms / len(X), one_point_ms_warm=one_ms)


def run_search(ctx, family, n, m, seed, batch, pool_log2, on, limit):
    A, b, c, l, u, ints = (packing if family == 'packing' else mixed)(n, m, seed)
    p = _ffi.Problem(ctx, A, b, c)
    t = _ffi.Tree(p, ints, l, u, branch_rule='pseudo cost', max_batch=batch, pool_capacity=1 << pool_log2)
    t.set_anchor_mode(True)
    t.set_dive(True)
    t.set_heuristic(True)
    if on:
        t.set_completion(True)
    t0 = time.perf_counter()
    first = first_s = None
    s = t.solve(mip_gap=1e-6, frontier_batch=batch, max_steps=1)
    while s['status'] == 4 and time.perf_counter() - t0 < limit:   # (step by step until an incumbent, then to the end)
        if first is None and np.isfinite(s['primal_bound']):
            first, first_s = s['steps'], time.perf_counter() - t0
            s = t.solve(mip_gap=1e-6, frontier_batch=batch, max_seconds=max(0.1, limit - (time.perf_counter() - t0)))
            break
        s = t.solve(mip_gap=1e-6, frontier_batch=batch, max_steps=1)
    if first is None and np.isfinite(s['primal_bound']):
        first, first_s = s['steps'], time.perf_counter() - t0
    h = t.heuristic_stats()
    out = dict(what='search', family=family, n=n, m=m, seed=seed, completion=bool(on), status=_ffi.TREE_STATUS[s['status']],
               seconds=time.perf_counter() - t0, steps=s['steps'], steps_to_first_incumbent=first, seconds_to_first_incumbent=first_s,
               nodes=s['evaluated_nodes'], primal=s['primal_bound'], dual=s['dual_bound'], heuristic=h)
    if on:
        f = t.completion_stats()
        out['completion_stats'] = dict(f, kernel_us_per_point=f['kernel_us'] / f['points'] if f['points'] else None,
                                       pivots_per_point=f['pivots'] / f['points'] if f['points'] else None)
    t.close()
    p.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--limit', type=float, default=20.0)
    ap.add_argument('--seeds', type=int, default=3)
    ap.add_argument('--big-seeds', type=int, default=1)
    ap.add_argument('--skip-entry', action='store_true')
    ap.add_argument('--skip-search', action='store_true')
    args = ap.parse_args()
    ctx = _ffi.default_context()
    shapes = [(40, 20, 64, 16, args.seeds), (72, 36, 256, 20, args.seeds), (144, 72, 1024, 21, args.big_seeds)]
    for family in ('mixed', 'packing'):
        for n, m, batch, pool_log2, seeds in shapes:
            for seed in range(seeds):
                if not args.skip_entry:
                    print(json.dumps(run_entry(ctx, family, n, m, seed)), flush=True)
                if not args.skip_search:
                    for on in (False, True):
                        print(json.dumps(run_search(ctx, family, n, m, seed, batch, pool_log2, on, args.limit)), flush=True)


if __name__ == '__main__':
    main()
