"""What the weighted row repair (include/mipx_wrepair.h) costs and buys beside the fix-and-propagate dive (DESIGN.md
section 4o), one JSON line per run.  The instances, the LP points and the searches are those of
scripts/fix_propagate_profile.py; the legs are the rounding heuristic alone, with the dive, and with the weighted repair.

Points: on node LP points of each instance (the root's and those of child boxes, solved on the GPU), the share the
rounding ends feasible on, the share the dive does and the share the weighted repair does, with the device time of each
launch per point and the best and median objective after the heuristic's lift.
Searches: steps until the first incumbent, nodes evaluated to the proven optimum (or the time limit) and seconds for
plain, heuristic, heuristic + dive, heuristic + weighted repair, and the last three with the objective step.
Kernel: device time of wrepair_steps and of fixprop_dive on the same points at 256 x 128, for one point and for 512.

    python scripts/weighted_repair_profile.py [--limit 20] [--seeds 4] [--big-seeds 2] [--skip-kernel]
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
from fix_propagate_profile import lp_points, mixed                            # noqa: E402

CONFIGS = [('plain', dict()),
           ('heuristic', dict(heuristic=True)),
           ('heuristic + dive', dict(heuristic=True, fix_propagate=True)),
           ('heuristic + weighted', dict(heuristic=True, weighted_repair=True)),
           ('heuristic + step', dict(heuristic=True, step=1.0)),
           ('heuristic + dive + step', dict(heuristic=True, fix_propagate=True, step=1.0)),
           ('heuristic + weighted + step', dict(heuristic=True, weighted_repair=True, step=1.0))]


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


def lifted(p, out, l, u, ints):
    """Objectives of the feasible points of `out` after the heuristic's lift, as the engine lifts them."""
    ok = out['status'] == 0
    if not ok.any():
        return np.zeros(0)
    h = p.round_repair_batch(out['x'][ok], l, u, ints)
    return h['obj'][h['status'] == 0]


def run_points(ctx, name, arrays, count, seed):
    A, b, c, l, u, ints = arrays
    p = _ffi.Problem(ctx, A, b, c)
    X = lp_points(p, l, u, ints, count, seed)
    h, h_ms = timed(ctx, lambda: p.round_repair_batch(X, l, u, ints))
    d, d_ms = timed(ctx, lambda: p.fix_propagate_batch(X, l, u, ints))
    w, w_ms = timed(ctx, lambda: p.weighted_repair_batch(X, l, u, ints))
    dl, wl = lifted(p, d, l, u, ints), lifted(p, w, l, u, ints)
    p.close()
    hf, df, wf = h['status'] == 0, d['status'] == 0, w['status'] == 0
    return dict(instance=name, what='points', points=len(X), rounding_feasible=int(hf.sum()), dive_feasible=int(df.sum()),
                weighted_feasible=int(wf.sum()), weighted_where_rounding_is_not=int((wf & ~hf).sum()),
                dive_tries_mean=float(d['counts'][:, 1].mean()), weighted_moves_mean=float(w['counts'][:, 0].mean()),
                weighted_bumps_mean=float(w['counts'][:, 1].mean()), weighted_steps_max=int(w['counts'].sum(axis=1).max()),
                rounding_launch_us_per_point=1000.0 * h_ms / len(X), dive_launch_us_per_point=1000.0 * d_ms / len(X),
                weighted_launch_us_per_point=1000.0 * w_ms / len(X),
                dive_best_lifted=float(dl.min()) if dl.size else None, weighted_best_lifted=float(wl.min()) if wl.size else None,
                dive_median_lifted=float(np.median(dl)) if dl.size else None,
                weighted_median_lifted=float(np.median(wl)) if wl.size else None)


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
    if opts.get('weighted_repair'):
        t.set_weighted_repair(True)
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
    if opts.get('weighted_repair'):
        f = t.weighted_repair_stats()
        out['weighted_repair'] = dict(f, kernel_us_per_point=f['kernel_us'] / f['points'] if f['points'] else None)
    if opts.get('step'):
        out['objective_step'] = {k: v for k, v in t.objective_step_stats().items() if not k.startswith('reserved')}
    t.close()
    p.close()
    return out


def run_kernel(ctx, n, m, k):
    """LP points of mixed(n, m - k, k, 0), the first alone and 512 copies' worth of them: both kernels on the same."""
    A, b, c, l, u, ints = mixed(n, m - k, k, 0)
    p = _ffi.Problem(ctx, A, b, c)
    X = lp_points(p, l, u, ints, 64, 0)
    for batch in (1, 512):
        Xb = np.tile(X, (batch // len(X) + 1, 1))[:batch]
        d, d_ms = timed(ctx, lambda: p.fix_propagate_batch(Xb, l, u, ints), repeats=3)
        w, w_ms = timed(ctx, lambda: p.weighted_repair_batch(Xb, l, u, ints), repeats=3)
        yield dict(what='kernel', n=n, m=m, batch=batch, dive_launch_ms=d_ms, weighted_launch_ms=w_ms,
                   dive_us_per_point=1000.0 * d_ms / batch, weighted_us_per_point=1000.0 * w_ms / batch,
                   dive_status=np.bincount(d['status'], minlength=6).tolist(), weighted_status=np.bincount(w['status'], minlength=4).tolist(),
                   dive_tries_mean=float(d['counts'][:, 1].mean()), weighted_steps_mean=float(w['counts'].sum(axis=1).mean()),
                   weighted_steps_max=int(w['counts'].sum(axis=1).max()))
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
    if not args.skip_kernel:
        for line in run_kernel(ctx, 256, 128, 32):
            print(json.dumps(line), flush=True)
    for name, arrays, batch, pool_log2, count, seed in families:
        for what, opts in CONFIGS:
            print(json.dumps(run_search(ctx, name, arrays, batch, pool_log2, what, opts, args.limit)), flush=True)


if __name__ == '__main__':
    main()
