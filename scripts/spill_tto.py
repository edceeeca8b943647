"""Host spill on the metric's instance (C3: 256 x 128, seed 0): the best-first phase of bench.py's time-to-gap
leg with a 2^22-row device pool and the host spill on, against the 2^24-row pool without it.

Phase 1 (depth first, as bench.two_phase) runs once; its incumbent seeds both best-first runs, which then
take steps of 8192 nodes with the in-place dive until the gap closes, the pool is full or --seconds pass.
Printed as one JSON document (and written to --out): per run the allocation seconds, nodes/s before and
after the first spill event, spill and reload milliseconds per step, host bytes, and the gap reached at
fixed search-time marks.  Run it alone on the GPU; for where the time goes, under
`rocprofv3 --kernel-trace --stats -- python scripts/spill_tto.py ...`."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simple_mip_solver_amd import _ffi   # noqa: E402
from simple_mip_solver_amd.generators import random_dense_milp_arrays   # noqa: E402

INF = float('inf')


def depth_first(ctx, p, inst, dive, seconds):
    A, b, c, l, u, ints = inst
    t = _ffi.Tree(p, ints, l, u, branch_rule='pseudo cost', search_rule='depth first', max_batch=1024,
                  pool_capacity=1 << 21)
    t.set_anchor_mode(True)
    t.set_dive(max(1, dive))
    t0 = time.perf_counter()
    s = None
    while s is None or time.perf_counter() - t0 < seconds:
        s = t.solve(mip_gap=1e-4, frontier_batch=1024, max_steps=20)
        if s['status'] != 4:
            break
    t.close()
    return s


def best_first(ctx, p, inst, dive, pool_log2, spill, incumbent, seconds, marks, batch=8192):
    A, b, c, l, u, ints = inst
    a0 = time.perf_counter()
    t = _ffi.Tree(p, ints, l, u, branch_rule='pseudo cost', max_batch=batch, pool_capacity=1 << pool_log2)
    t.set_anchor_mode(True)
    t.set_dive(max(1, dive))
    if spill:
        t.set_host_spill(spill)
    alloc = time.perf_counter() - a0
    if incumbent < INF:
        t.set_primal_bound(incumbent)
    t0 = time.perf_counter()
    timeline = []   # (search seconds, evaluated, steps, gap, spill stats)
    s = None
    while s is None or time.perf_counter() - t0 < seconds:
        s = t.solve(mip_gap=1e-4, frontier_batch=batch, max_steps=10)
        timeline.append((time.perf_counter() - t0, s['evaluated_nodes'], s['steps'], s['gap'], t.spill_stats()))
        if s['status'] != 4 or s['pool_exhausted']:
            break
    a1 = time.perf_counter()
    t.close()
    alloc += time.perf_counter() - a1
    first = next((k for k, e in enumerate(timeline) if e[4]['events'] > 0), None)

    def rate(a, z):
        if a is None or z is None or z <= a:
            return None
        return (timeline[z][1] - timeline[a][1]) / (timeline[z][0] - timeline[a][0])
    last = len(timeline) - 1
    sp = timeline[-1][4]
    # steps since the last snapshot before the first event: every spill event of the run falls into them
    base = timeline[first - 1][2] if first else 0
    steps = max(1, timeline[-1][2] - base)
    # bytes per record at one moment: the host bytes and the nodes on the host of the same snapshot (segments
    # are freed only when empty, so with reloads this is an upper bound), and the peak snapshot's
    peak = max(timeline, key=lambda e: e[4]['host_bytes'])[4]
    out = {
        'pool_rows': 1 << pool_log2, 'host_spill_bytes': spill or 0, 'allocation_seconds': alloc,
        'status': _ffi.TREE_STATUS[s['status']], 'pool_exhausted': bool(s['pool_exhausted']),
        'search_seconds': timeline[-1][0], 'nodes': s['evaluated_nodes'], 'steps': s['steps'],
        'gap': None if s['gap'] < 0 else s['gap'], 'primal_bound': s['primal_bound'], 'dual_bound': s['dual_bound'],
        'nodes_per_s_before_first_spill': rate(0, first if first is not None else last),
        'nodes_per_s_after_first_spill': rate(first, last) if first is not None else None,
        'first_spill': None if first is None else {'seconds': timeline[first][0], 'nodes': timeline[first][1]},
        'spill': sp, 'spill_ms_per_step_since_first': sp['spill_ms'] / steps,
        'reload_ms_per_step_since_first': sp['reload_ms'] / steps,
        'spill_ms_per_event': sp['spill_ms'] / sp['events'] if sp['events'] else None,
        'nodes_per_event': sp['spilled'] / sp['events'] if sp['events'] else None,
        'host_bytes_per_node_on_host': peak['host_bytes'] / peak['on_host'] if peak['on_host'] else None,
        'gap_at_seconds': {f'{mk:g}': next(((None if e[3] < 0 else e[3]), e[1]) for e in timeline if e[0] >= mk)
                           if timeline[-1][0] >= mk else None for mk in marks},
    }
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--seconds', type=float, default=60.0, help='search-time limit of each best-first run')
    ap.add_argument('--dfs-seconds', type=float, default=2.0, help='depth-first phase for the incumbent')
    ap.add_argument('--dive', type=int, default=8)
    ap.add_argument('--spill-bytes', type=int, default=64 << 30, help='host cap of the spill run')
    ap.add_argument('--marks', type=float, nargs='*', default=[10, 20, 30, 40, 50, 60])
    ap.add_argument('--only', choices=['big', 'spill'], default=None, help='one of the two runs (e.g. for a profile)')
    ap.add_argument('--out', default=None, help='also write the JSON document to this file')
    args = ap.parse_args()
    ctx = _ffi.default_context()
    inst = random_dense_milp_arrays(256, 128, seed=0)
    A, b, c = inst[:3]
    p = _ffi.Problem(ctx, A, b, c)
    s1 = depth_first(ctx, p, inst, args.dive, args.dfs_seconds)
    res = {'instance': 'C3: 256 vars x 128 rows random dense MILP, seed 0',
           'phase_1_depth_first': {'nodes': s1['evaluated_nodes'], 'primal_bound': s1['primal_bound']}}
    runs = [('big_pool_no_spill', 24, 0), ('small_pool_spill', 22, args.spill_bytes)]
    for name, log2, spill in runs:
        if args.only and (args.only == 'big') != (spill == 0):
            continue
        res[name] = best_first(ctx, p, inst, args.dive, log2, spill, s1['primal_bound'], args.seconds, args.marks)
        print(json.dumps({name: res[name]}), flush=True)
    p.close()
    if args.out:
        os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
