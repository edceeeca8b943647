"""Disjunctive separation (include/mipx_cglp.h, DisjunctiveSeparator) on the tree of DESIGN.md 4f: 256 x 128,
seed 0, B = 8 192, plunge of depth 8, ten steps after the ramp-up.  For T = 10^3, 10^4, 10^5 childless
not-infeasible nodes (the first T below the root, in id order) it runs the row generation to convergence and
reports rounds, leaf LPs per second in round one and in the later rounds (device time of the node-LP launches),
pivots per leaf LP, the selection kernels' time and the share of a round spent in the master; then
mipx_tree_node_solve on the same leaves, the yardstick of a separation round.  Prints one JSON line.

    python3 scripts/cglp_separation_profile.py [n m B dive steps max_rounds]    (default: 256 128 8192 8 10 40)

The measurement runs in a child process under a time limit.
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = (1000, 10000, 100000)


def child(n, m, B, dive, steps, max_rounds):
    import numpy as np
    from simple_mip_solver_amd import _ffi
    from simple_mip_solver_amd.generators import random_dense_milp_arrays
    from simple_mip_solver_amd.utils.disjunctive_separation import DisjunctiveSeparator
    from simple_mip_solver_amd.lp import CyLPArray
    ctx = _ffi.default_context()
    A, b, c, l, u, ints = random_dense_milp_arrays(n, m, seed=0)
    pool = max(1 << 16, 3 * B * (2 * (1 + dive) + 1) * 8)
    p = _ffi.Problem(ctx, A, b, c)
    t = _ffi.Tree(p, ints, l, u, branch_rule='pseudo cost', max_batch=B, pool_capacity=pool)
    t.set_anchor_mode(True)
    t.set_dive(dive)
    t.set_tree_record(True)
    st = t.stats()
    while st['open_nodes'] < B and st['status'] in (0, 4):
        st = t.solve(mip_gap=0.0, frontier_batch=min(B, 256), max_steps=1)
    t.solve(mip_gap=0.0, frontier_batch=B, max_steps=steps)
    rec = t.tree_records()
    leaves = np.flatnonzero(((rec['flags'] & _ffi.TR_HAS_CHILDREN) == 0) & (rec['lp_status'] != 1))
    x_root = t.node_solve([0])['x'][0]
    out = dict(tree_nodes=int(len(rec['parent'])), childless_not_infeasible=int(len(leaves)), runs=[])
    for T in SIZES:
        ids = leaves[:T]
        if len(ids) < T:
            break
        s0 = t.tree_record_stats()
        g0 = time.perf_counter()
        res = t.node_solve(ids, want_x=False, want_vstat=False)
        g1 = time.perf_counter()
        s1 = t.tree_record_stats()
        yard = dict(wall_ms=1e3 * (g1 - g0), device_ms=s1['query_ms'] - s0['query_ms'],
                    nodes_per_s_device=T / max(1e-9, 1e-3 * (s1['query_ms'] - s0['query_ms'])),
                    optimal=int((res['status'] == 0).sum()))
        ses = t.support_open(ids)
        sep = DisjunctiveSeparator.on_session(ses, l, u, max_rounds=max_rounds)
        # round by round: the session's counters after each evaluation
        per_round = []
        inner = ses.eval

        def eval_and_note(*a, **k):
            r = inner(*a, **k)
            per_round.append(ses.stats())
            return r
        ses.eval = eval_and_note
        g0 = time.perf_counter()
        pi, pi0 = sep.solve(CyLPArray(x_root))
        wall = time.perf_counter() - g0
        first, last = per_round[0], per_round[-1]
        later_lps = last['leaf_lps'] - first['leaf_lps']
        later_ms = (last['kernel_ms'] - last['select_ms']) - (first['kernel_ms'] - first['select_ms'])
        out['runs'].append(dict(
            T=T, node_solve=yard, stats=sep.stats, wall_s=wall, timing=sep.timing,
            master_share=sep.timing['master'] / max(1e-9, sep.timing['master'] + sep.timing['separation']),
            round_one=dict(leaf_lps=first['leaf_lps'], lp_ms=first['kernel_ms'] - first['select_ms'], pivots=first['pivots'],
                           iterations=first['iterations']),
            later=dict(leaf_lps=later_lps, lp_ms=later_ms, leaf_lps_per_s=later_lps / max(1e-9, 1e-3 * later_ms),
                       pivots_per_lp=(last['pivots'] - first['pivots']) / max(1, later_lps),
                       iterations_per_lp=(last['iterations'] - first['iterations']) / max(1, later_lps)),
            select_ms_per_round=last['select_ms'] / max(1, last['evaluations']), device_bytes=last['device_bytes'],
            cut_found=pi is not None))
        ses.close()
    print(json.dumps(out))
    t.close()
    p.close()


def main():
    args = sys.argv[1:7] + ['256', '128', '8192', '8', '10', '40'][len(sys.argv[1:7]):]
    run = subprocess.run([sys.executable, os.path.abspath(__file__), '--child'] + args, capture_output=True, text=True, timeout=900)
    if run.returncode != 0:
        sys.stderr.write(run.stderr[-4000:])
        sys.exit(f'exit status {run.returncode}')
    print(run.stdout.strip().splitlines()[-1])


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == '--child':
        child(*(int(a) for a in sys.argv[2:8]))
    else:
        main()
