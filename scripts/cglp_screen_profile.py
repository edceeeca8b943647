"""The options of DisjunctiveSeparator (screen, stabilisation, retry_cold; include/mipx_cglp_screen.h) on the tree and
settings of DESIGN.md 4g's table: 256 x 128, seed 0, B = 8 192, plunge of depth 8, ten steps after the ramp-up, the first
T = 10^3, 10^4, 10^5 childless not-infeasible nodes in id order, x* the root's solution, P = 32.  Every variant runs on
a session of its own and prints one JSON line when it is done:

    rounds, leaf LPs, pivots and iterations per leaf LP in the rounds after the first, the share of the leaf
    evaluations that the screen answered, device time per round (HIP events: node LPs, screen, selection), the screen
    kernels' own time per round, the master's share of the wall time, and what ended the run.

    python3 scripts/cglp_screen_profile.py [sizes variants max_rounds n m B dive steps]
        sizes     comma list, default 1000,10000,100000
        variants  comma list of default, screen, in-out-0.3, in-out-0.5, screen+in-out-0.3, screen+in-out-0.5,
                  screen+in-out-0.3+retry, screen+in-out-0.5+retry (default: all of them)
        the rest  default 40 256 128 8192 8 10

Device times come from the session's events and end in a synchronise; the first evaluation of a session is the warm-up
of its shapes and is reported apart (round one).  The measurement runs in a child process under a time limit.
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VARIANTS = {
    'default': dict(),
    'screen': dict(screen=True),
    'in-out-0.3': dict(stabilisation=0.3),
    'in-out-0.5': dict(stabilisation=0.5),
    'screen+in-out-0.3': dict(screen=True, stabilisation=0.3),
    'screen+in-out-0.5': dict(screen=True, stabilisation=0.5),
    'screen+in-out-0.3+retry': dict(screen=True, stabilisation=0.3, retry_cold=True),
    'screen+in-out-0.5+retry': dict(screen=True, stabilisation=0.5, retry_cold=True),
}


def ended_by(stats, max_rounds):
    if stats['converged']:
        return 'converged'
    if stats['leaf_lps_not_optimal']:
        return '%d leaf LP(s) not optimal' % stats['leaf_lps_not_optimal']
    if stats['master_failed']:
        return 'the master: not solved'
    if stats['rounds'] >= max_rounds:
        return 'max_rounds'
    return 'no new point'


def child(sizes, variants, max_rounds, n, m, B, dive, steps):
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
    print(json.dumps(dict(tree_nodes=int(len(rec['parent'])), childless_not_infeasible=int(len(leaves)))), flush=True)
    for T in sizes:
        ids = leaves[:T]
        if len(ids) < T:
            break
        for name in variants:
            options = VARIANTS[name]
            ses = t.support_open(ids, duals=bool(options.get('screen') or options.get('retry_cold')))
            sep = DisjunctiveSeparator.on_session(ses, l, u, max_rounds=max_rounds, **options)
            per_round, screen_us = [], []
            inner = ses.eval

            def eval_and_note(*a, **k):
                r = inner(*a, **k)
                per_round.append(ses.stats())
                screen_us.append(r.get('screen_us', 0.0))
                return r
            ses.eval = eval_and_note
            g0 = time.perf_counter()
            pi, pi0 = sep.solve(CyLPArray(x_root))
            wall = time.perf_counter() - g0
            first, last = per_round[0], per_round[-1]
            later_lps = last['leaf_lps'] - first['leaf_lps']
            later_rounds = max(1, len(per_round) - 1)
            stats = sep.stats
            print(json.dumps(dict(
                T=T, variant=name, rounds=stats['rounds'], leaf_lps=stats['leaf_lps'], leaves=stats['leaves'],
                screened=stats.get('screened', 0),
                screened_share=stats.get('screened', 0) / max(1, stats.get('screened', 0) + stats['leaf_lps']),
                in_moves=stats.get('in_moves', 0), retried=stats.get('retried', 0), retried_optimal=stats.get('retried_optimal', 0),
                pivots_per_lp_round_one=first['pivots'] / max(1, first['leaf_lps']),
                pivots_per_lp_later=(last['pivots'] - first['pivots']) / max(1, later_lps),
                iterations_per_lp_later=(last['iterations'] - first['iterations']) / max(1, later_lps),
                device_ms_round_one=first['kernel_ms'],
                device_ms_per_later_round=(last['kernel_ms'] - first['kernel_ms']) / later_rounds,
                screen_ms_per_later_round=1e-3 * sum(screen_us[1:]) / later_rounds,
                select_ms_per_round=last['select_ms'] / max(1, last['evaluations']),
                master_share=sep.timing['master'] / max(1e-9, sep.timing['master'] + sep.timing['separation']),
                wall_s=wall, device_bytes=last['device_bytes'], violation=stats['violation'],
                final_min_margin=stats['final_min_margin'], master_rows=stats['master_rows'],
                ended_by=ended_by(stats, max_rounds), cut_found=pi is not None)), flush=True)
            ses.close()
    t.close()
    p.close()


def main():
    args = sys.argv[1:9] + ['1000,10000,100000', ','.join(VARIANTS), '40', '256', '128', '8192', '8', '10'][len(sys.argv[1:9]):]
    unknown = [v for v in args[1].split(',') if v not in VARIANTS]
    if unknown:
        sys.exit(f'unknown variant(s) {unknown}: choose from {list(VARIANTS)}')
    run = subprocess.run([sys.executable, os.path.abspath(__file__), '--child'] + args, stderr=subprocess.PIPE, text=True, timeout=1100)
    if run.returncode != 0:
        sys.stderr.write(run.stderr[-4000:])
        sys.exit(f'exit status {run.returncode}')


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == '--child':
        a = sys.argv[2:10]
        child([int(v) for v in a[0].split(',')], a[1].split(','), *(int(v) for v in a[2:8]))
    else:
        main()
