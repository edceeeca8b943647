"""What the fix-and-propagate dive (include/mipx_fixprop.h) costs and buys, one JSON line per run.

Points: on node LP points of each instance (the root's and those of child boxes, solved on the GPU), the share the
rounding heuristic ends feasible on, the share the dive does, and the share either does.
Searches: steps until the first incumbent, nodes evaluated to the proven optimum (or the time limit) and seconds for
plain, heuristic, heuristic + dive, and both of those with the objective step; with the options' counters.
Kernel: device time of fixprop_dive per point at 256 x 128 and 1024 x 1024, for one point (one workgroup: the latency
of a dive) and for 512 (two workgroups per CU), at several caps on the tries.

    python scripts/fix_propagate_profile.py [--limit 20] [--seeds 4] [--big-seeds 2] [--skip-kernel]
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

CONFIGS = [('plain', dict()),
           ('heuristic', dict(heuristic=True)),
           ('heuristic + dive', dict(heuristic=True, fix_propagate=True)),
           ('heuristic + step', dict(heuristic=True, step=1.0)),
           ('heuristic + dive + step', dict(heuristic=True, fix_propagate=True, step=1.0))]


def mixed(n, m, k, seed):
    """The generator's packing rows plus k covering rows C x >= d (the family of the propagation's tests)."""
    A, b, c, l, u, ints = random_dense_milp_arrays(n, m, seed=seed)
    rng = np.random.default_rng(100 + seed)
    Cm = rng.integers(1, 11, (k, n)).astype(np.float64)
    Cm = Cm * (rng.random((k, n)) < 0.3)
    d = np.floor(0.06 * Cm @ np.full(n, 10.0))
    return np.vstack([A, Cm]), np.concatenate([b, d]), c, l, u, ints


def lp_points(p, l, u, ints, count, seed):
    """The root LP point and LP points of child boxes (a random 15 % of the integer columns fixed to a rounding of the
    root point), those whose LP is feasible."""
    rng = np.random.default_rng(500 + seed)
    root = p.solve_batch(l[None], u[None])
    x0 = root['x'][0]
    J = np.asarray(ints, dtype=np.int64)
    L, U = np.tile(l, (4 * count, 1)), np.tile(u, (4 * count, 1))
    for k in range(1, 4 * count):
        pick = J[rng.random(J.size) < 0.15]
        v = np.where(rng.random(pick.size) < 0.5, np.floor(x0[pick]), np.ceil(x0[pick]))
        L[k, pick] = U[k, pick] = np.minimum(np.maximum(v, l[pick]), u[pick])
    out = p.solve_batch(L, U)
    return out['x'][out['status'] == 0][:count]


def run_points(ctx, name, arrays, count, seed):
    A, b, c, l, u, ints = arrays
    p = _ffi.Problem(ctx, A, b, c)
    X = lp_points(p, l, u, ints, count, seed)
    h = p.round_repair_batch(X, l, u, ints)
    ctx.timer_start()
    d = p.fix_propagate_batch(X, l, u, ints)
    ms = ctx.timer_stop()
    p.close()
    hf, df = h['status'] == 0, d['status'] == 0
    both = hf & df
    return dict(instance=name, what='points', points=len(X), rounding_feasible=int(hf.sum()), dive_feasible=int(df.sum()),
                either=int((hf | df).sum()), dive_where_rounding_is_not=int((df & ~hf).sum()),
                rounding_better_where_both=int((h['obj'][both] < d['obj'][both]).sum()),
                dive_better_where_both=int((d['obj'][both] < h['obj'][both]).sum()),
                dive_status=np.bincount(d['status'], minlength=6).tolist(), tries_mean=float(d['counts'][:, 1].mean()),
                tries_max=int(d['counts'][:, 1].max()), launch_ms=ms)


def run_search(ctx, name, arrays, batch, pool_log2, what, opts, limit):
    A, b, c, l, u, ints = arrays
    p = _ffi.Problem(ctx, A, b, c)
    t = _ffi.Tree(p, ints, l, u, branch_rule='pseudo cost', max_batch=batch, pool_capacity=1 << pool_log2)
    t.set_anchor_mode(True)
    t.set_dive(True)
    if opts.get('heuristic'):
        t.set_heuristic(True)
    if opts.get('fix_propagate'):
        t.set_fix_propagate(True)
    if opts.get('step'):
        t.set_objective_step(opts['step'])
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
    out = dict(instance=name, what='search', configuration=what, status=_ffi.TREE_STATUS[s['status']],
               seconds=time.perf_counter() - t0, steps=s['steps'], steps_to_first_incumbent=first, nodes=s['evaluated_nodes'],
               primal=s['primal_bound'], dual=s['dual_bound'])
    if opts.get('heuristic'):
        out['heuristic'] = t.heuristic_stats()
    if opts.get('fix_propagate'):
        f = t.fix_propagate_stats()
        out['fix_propagate'] = dict(f, kernel_us_per_point=f['kernel_us'] / f['points'] if f['points'] else None)
    if opts.get('step'):
        out['objective_step'] = {k: v for k, v in t.objective_step_stats().items() if not k.startswith('reserved')}
    t.close()
    p.close()
    return out


def run_kernel(ctx, n, m, k):
    A, b, c, l, u, ints = mixed(n, m - k, k, 0)
    p = _ffi.Problem(ctx, A, b, c)
    rng = np.random.default_rng(7)
    x0 = l + 0.3 * (u - l) * rng.random(n)
    for batch in (1, 512):
        X = np.clip(np.tile(x0, (batch, 1)) + rng.uniform(-1, 1, (batch, n)) * (rng.random((batch, n)) < 1 / 3), l, u)
        for tries in (8, 32, 128, 4096):
            if n > 512 and tries > 128:   # (a try at that size is milliseconds: the larger caps follow from the smaller)
                continue
            p.fix_propagate_batch(X[:1], l, u, ints, max_tries=1)   # (warm: the staging buffers)
            ctx.timer_start()
            d = p.fix_propagate_batch(X, l, u, ints, max_tries=tries)
            ms = ctx.timer_stop()
            made = int(d['counts'][:, 1].sum())
            yield dict(what='kernel', n=n, m=m, batch=batch, max_tries=tries, launch_ms=ms, ms_per_point=ms / batch,
                       tries_mean=made / batch, us_per_try_of_a_point=1000.0 * ms / max(1, int(d['counts'][:, 1].max())),
                       status=np.bincount(d['status'], minlength=6).tolist())
    p.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--limit', type=float, default=20.0)
    ap.add_argument('--seeds', type=int, default=4)
    ap.add_argument('--big-seeds', type=int, default=2)
    ap.add_argument('--skip-kernel', action='store_true')
    args = ap.parse_args()
    ctx = _ffi.default_context()
    families = [('mixed 40 x 30 seed %d' % s, mixed(40, 20, 10, s), 64, 16, 64, s) for s in range(args.seeds)]
    families += [('generator 40 x 20 seed %d' % s, random_dense_milp_arrays(40, 20, seed=s), 64, 16, 64, s) for s in range(args.seeds)]
    families += [('mixed 144 x 108 seed %d' % s, mixed(144, 72, 36, s), 1024, 21, 64, s) for s in range(args.big_seeds)]
    for name, arrays, batch, pool_log2, count, seed in families:
        print(json.dumps(run_points(ctx, name, arrays, count, seed)), flush=True)
    for name, arrays, batch, pool_log2, count, seed in families:
        for what, opts in CONFIGS:
            print(json.dumps(run_search(ctx, name, arrays, batch, pool_log2, what, opts, args.limit)), flush=True)
    if not args.skip_kernel:
        for n, m, k in ((256, 128, 32), (1024, 1024, 256)):
            for line in run_kernel(ctx, n, m, k):
                print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
