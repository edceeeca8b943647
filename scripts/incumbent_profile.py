"""What the objective-step cutoff (include/mipx_objstep.h) and the pair-move local search (include/mipx_lsearch.h)
cost and buy, one JSON line per run: nodes evaluated to the proven optimum (or the time limit),
seconds, the counters of the options and the kernels' device time per point and per step -- for five configurations:
plain, primal heuristic, heuristic + step, heuristic + step + pair search, and all of those with the reduced-cost
tightening -- on 40 x 20 instances of the generator, 144 x 72 instances, and the bench's 256 x 128 instance, which
does not close: there the line holds the incumbent and the gap after the bench's two phases (the ramp-up to 8192 open
nodes, then steps of 8192 nodes).

    python scripts/incumbent_profile.py [--limit 20] [--seeds 4] [--big-seeds 2] [--bench-steps 30]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from simple_mip_solver_amd import _ffi                                        # noqa: E402
from simple_mip_solver_amd.generators import random_dense_milp_arrays         # noqa: E402

CONFIGS = [('plain', dict()),
           ('heuristic', dict(heuristic=True)),
           ('heuristic + step', dict(heuristic=True, step=1.0)),
           ('heuristic + step + pair search', dict(heuristic=True, step=1.0, local_search=True)),
           ('all + reduced cost', dict(heuristic=True, step=1.0, local_search=True, reduced_cost=True))]


def make_tree(ctx, arrays, batch, pool, dive=True, heuristic=False, step=None, local_search=False, reduced_cost=False):
    A, b, c, l, u, ints = arrays
    p = _ffi.Problem(ctx, A, b, c)
    t = _ffi.Tree(p, ints, l, u, branch_rule='pseudo cost', max_batch=batch, pool_capacity=pool)
    t.set_anchor_mode(True)
    t.set_dive(dive)
    if heuristic:
        t.set_heuristic(True)
    if local_search:
        t.set_local_search(True)
    if step:
        t.set_objective_step(step)
    if reduced_cost:
        t.set_reduced_cost(True)
    return p, t


def report(t, s, seconds, opts):
    out = dict(status=_ffi.TREE_STATUS[s['status']], seconds=seconds, steps=s['steps'], nodes=s['evaluated_nodes'],
               lps=s['lp_solved'], primal=s['primal_bound'], dual=s['dual_bound'],
               gap=None if s['primal_bound'] == float('inf') or s['primal_bound'] == 0 else
               abs(s['primal_bound'] - s['dual_bound']) / abs(s['primal_bound']),
               node_lp_ms_per_step=s['kernel_ms'] / s['steps'] if s['steps'] else None)
    if opts.get('heuristic'):
        h = t.heuristic_stats()
        out['heuristic'] = dict(h, kernel_us_per_point=h['kernel_us'] / h['points'] if h['points'] else None,
                                kernel_us_per_step=h['kernel_us'] / s['steps'] if s['steps'] else None)
    if opts.get('local_search'):
        ls = t.local_search_stats()
        out['local_search'] = dict(ls, kernel_us_per_point=ls['kernel_us'] / ls['points'] if ls['points'] else None,
                                   kernel_us_per_step=ls['kernel_us'] / s['steps'] if s['steps'] else None)
    if opts.get('step'):
        out['objective_step'] = {k: v for k, v in t.objective_step_stats().items() if not k.startswith('reserved')}
    if opts.get('reduced_cost'):
        out['reduced_cost'] = t.reduced_cost_stats()
    return out


def run(ctx, arrays, batch, pool_log2, opts, limit):
    p, t = make_tree(ctx, arrays, batch, 1 << pool_log2, **opts)
    t0 = time.perf_counter()
    s = t.solve(mip_gap=0.0, frontier_batch=batch, max_seconds=limit)
    out = report(t, s, time.perf_counter() - t0, opts)
    t.close()
    p.close()
    return out


def run_bench_phases(ctx, arrays, opts, steps):
    """The bench's two phases on its instance (bench.py: 256 x 128, seed 0, plunges of 8): steps of at most 1024 nodes
    until 8192 are open, every open node re-anchored, then `steps` steps of 8192 nodes."""
    B = 8192
    p, t = make_tree(ctx, arrays, B, 18 * B * (steps + 8) + 4 * B, dive=8, **opts)
    t0 = time.perf_counter()
    s = t.solve(mip_gap=0.0, frontier_batch=1024, max_steps=1)
    while s['open_nodes'] < B and s['status'] == 4:
        s = t.solve(mip_gap=0.0, frontier_batch=1024, max_steps=1)
    ramp = s['steps']
    t.reanchor(t.stats()['open_nodes'])
    s = t.solve(mip_gap=0.0, frontier_batch=B, max_steps=steps)
    out = dict(report(t, s, time.perf_counter() - t0, opts), ramp_steps=ramp, open_nodes=s['open_nodes'])
    t.close()
    p.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--limit', type=float, default=20.0)
    ap.add_argument('--seeds', type=int, default=4)
    ap.add_argument('--big-seeds', type=int, default=2)
    ap.add_argument('--bench-steps', type=int, default=30)
    args = ap.parse_args()
    ctx = _ffi.default_context()
    families = [('40 x 20 seed %d' % s, random_dense_milp_arrays(40, 20, seed=s), 64, 16) for s in range(args.seeds)]
    families += [('144 x 72 seed %d' % s, random_dense_milp_arrays(144, 72, seed=s), 1024, 21) for s in range(args.big_seeds)]
    for name, arrays, batch, pool_log2 in families:
        for what, opts in CONFIGS:
            out = run(ctx, arrays, batch, pool_log2, opts, args.limit)
            print(json.dumps(dict(out, instance=name, configuration=what)), flush=True)
    bench = random_dense_milp_arrays(256, 128, seed=0)
    for what, opts in CONFIGS:
        out = run_bench_phases(ctx, bench, opts, args.bench_steps)
        print(json.dumps(dict(out, instance='256 x 128 seed 0 (bench)', configuration=what)), flush=True)


if __name__ == '__main__':
    main()
