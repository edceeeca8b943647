"""What the LP dive (include/mipx_lpdive.h) costs and buys, one JSON line per run.

Families: the generator's instances with the even columns integer and the odd ones continuous ("packing"), and the
same with the first half of the rows turned into covering rows whose right-hand side is 0.8 of their activity at a
random integer point ("mixed"), at 40 x 20, 72 x 36 and 144 x 72.
Entry: 64 LP points per instance with their node boxes and basis codes (the root's, then LPs with four random integer
bounds moved to the floor or the ceil of the root value).  Beside each other: the rounding (mipx_round_repair_batch),
the rounding completed (mipx_complete_batch), the weighted repair completed, and the dive by either rule
(mipx_lpdive_batch): points feasible, the best objective, rounds, fixings, flips and pivots per point, and the shortest
of five calls' device time per point, staging copies and the round counter's read-backs included.
Searches: with the heuristic alone ("off"), with complete_continuous, with weighted_repair + complete_continuous, and
with lp_dive beside complete_continuous: the step and the time of the first incumbent, nodes and seconds to the proven
optimum (or the time limit), the dive's counters and its device time per point and per step it ran in.

    python scripts/lp_dive_profile.py [--limit 20] [--seeds 3] [--big-seeds 1] [--skip-entry] [--skip-search]
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
    """(X, V, L, U) of `count` optimal LPs: the root's, then LPs with `moved` integer bounds moved to the floor or the
    ceil of the root value, warm from the root's basis; None where the root LP is not optimal."""
    root = p.solve_batch(l[None], u[None])
    if root['status'][0] != 0:
        return None
    rng = np.random.default_rng(seed)
    X, V, Ls, Us = [root['x'][0]], [root['vstat'][0]], [l.copy()], [u.copy()]
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
            X.append(r['x'][k]); V.append(r['vstat'][k]); Ls.append(L[k]); Us.append(U[k])
        if len(X) >= count:
            break
    return np.array(X[:count]), np.array(V[:count], dtype=np.int8), np.array(Ls[:count]), np.array(Us[:count])


def best_of(out):
    ok = out['status'] == 0
    return float(out['obj'][ok].min()) if ok.any() else None


def run_entry(ctx, family, n, m, seed, count=64):
    A, b, c, l, u, ints = (packing if family == 'packing' else mixed)(n, m, seed)
    p = _ffi.Problem(ctx, A, b, c)
    pts = lp_points(p, l, u, ints, count, seed)
    if pts is None:
        p.close()
        return dict(what='entry', family=family, n=n, m=m, seed=seed, root='not optimal')
    X, V, L, U = pts
    r = p.round_repair_batch(X, l, u, ints)
    done, done_ms = timed(ctx, lambda: p.complete_batch(r['x'], l, u, ints, vstat=V))
    w = p.weighted_repair_batch(X, l, u, ints)
    wdone = p.complete_batch(w['x'], l, u, ints, vstat=V, skip=w['status'] != 0)
    out = dict(what='entry', family=family, n=n, m=m, seed=seed, points=len(X), rounding_feasible=int((r['status'] == 0).sum()),
               completion_feasible=int((done['status'] == 0).sum()), completion_best=best_of(done),
               completion_us_per_point=1000.0 * done_ms / len(X), weighted_repair_feasible=int((w['status'] == 0).sum()),
               weighted_repair_completed=int((wdone['status'] == 0).sum()), weighted_repair_completed_best=best_of(wdone))
    for name, rule in _ffi.LPDIVE_RULES.items():
        d, ms = timed(ctx, lambda: p.lpdive_batch(X, L, U, ints, vstat=V, rule=rule))
        cold, cold_ms = timed(ctx, lambda: p.lpdive_batch(X, L, U, ints, rule=rule))
        out[name] = dict(feasible=int((d['status'] == 0).sum()), infeasible=int((d['status'] == 1).sum()),
                         limit_or_rejected=int(np.isin(d['status'], (2, 4)).sum()), best=best_of(d),
                         rounds_per_point=float(d['rounds'].mean()), rounds_max=int(d['rounds'].max()),
                         fixings_per_point=float(d['fixings'].mean()), flips_per_point=float(d['flips'].mean()),
                         pivots_per_point=float(d['pivots'].mean()), pivots_per_point_cold=float(cold['pivots'].mean()),
                         feasible_cold=int((cold['status'] == 0).sum()), us_per_point=1000.0 * ms / len(X),
                         us_per_point_cold=1000.0 * cold_ms / len(X), call_ms=ms)
    p.close()
    return out


VARIANTS = {'off': {}, 'complete': dict(complete=True), 'wrepair+complete': dict(complete=True, wrepair=True),
            'lp_dive': dict(complete=True, lpdive=True)}


def run_search(ctx, family, n, m, seed, batch, pool_log2, variant, limit):
    A, b, c, l, u, ints = (packing if family == 'packing' else mixed)(n, m, seed)
    opt = VARIANTS[variant]
    p = _ffi.Problem(ctx, A, b, c)
    t = _ffi.Tree(p, ints, l, u, branch_rule='pseudo cost', max_batch=batch, pool_capacity=1 << pool_log2)
    t.set_anchor_mode(True)
    t.set_dive(True)
    t.set_heuristic(True)
    if opt.get('wrepair'):
        t.set_weighted_repair(True)
    if opt.get('complete'):
        t.set_completion(True)
    if opt.get('lpdive'):
        t.set_lpdive(64)
    t0 = time.perf_counter()
    first = first_s = None
    dive_steps = 0
    s = t.solve(mip_gap=1e-6, frontier_batch=batch, max_steps=1)
    while s['status'] == 4 and time.perf_counter() - t0 < limit:   # (step by step until an incumbent, then to the end)
        dive_steps += 1
        if first is None and np.isfinite(s['primal_bound']):
            first, first_s = s['steps'], time.perf_counter() - t0
            s = t.solve(mip_gap=1e-6, frontier_batch=batch, max_seconds=max(0.1, limit - (time.perf_counter() - t0)))
            break
        s = t.solve(mip_gap=1e-6, frontier_batch=batch, max_steps=1)
    if first is None and np.isfinite(s['primal_bound']):
        first, first_s = s['steps'], time.perf_counter() - t0
    out = dict(what='search', family=family, n=n, m=m, seed=seed, variant=variant, status=_ffi.TREE_STATUS[s['status']],
               seconds=time.perf_counter() - t0, steps=s['steps'], steps_to_first_incumbent=first, seconds_to_first_incumbent=first_s,
               nodes=s['evaluated_nodes'], primal=s['primal_bound'], dual=s['dual_bound'], heuristic=t.heuristic_stats())
    if opt.get('complete'):
        out['completion_stats'] = t.completion_stats()
    if opt.get('wrepair'):
        out['weighted_repair_stats'] = t.weighted_repair_stats()
    if opt.get('lpdive'):
        f = t.lpdive_stats()
        ran = first if first is not None else s['steps']   # (the dive runs in the steps without an incumbent)
        out['lp_dive_stats'] = dict(f, kernel_us_per_point=f['kernel_us'] / f['points'] if f['points'] else None,
                                    kernel_us_per_step=f['kernel_us'] / ran if ran else None,
                                    pivots_per_point=f['pivots'] / f['points'] if f['points'] else None, steps_run=ran)
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
                    for variant in VARIANTS:
                        print(json.dumps(run_search(ctx, family, n, m, seed, batch, pool_log2, variant, args.limit)), flush=True)


if __name__ == '__main__':
    main()
