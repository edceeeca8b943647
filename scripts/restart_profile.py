"""A restart from the leaves of a recorded search (include/mipx_restart.h) against a cold solve at the same
right-hand side, on generator instances the engine closes: nodes evaluated and wall seconds of both (the cold
solve with the record off, so with the device finish, and with the record on, as the restart runs), and the
seeding kernel's device time beside the wall time of mipx_tree_node_bounds for the same ids.  Prints one JSON
line per size.

    python3 scripts/restart_profile.py [B dive seed]     (default: 1024 2 0; sizes 60x30, 80x40, 100x50)

Every size runs in a child process of its own under a time limit; the first one that fails ends the script.
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = ((60, 30), (80, 40), (100, 50))
LIMIT = 60.0   # seconds per solve


def tree(_ffi, p, ints, l, u, B, dive, record):
    t = _ffi.Tree(p, ints, l, u, branch_rule='pseudo cost', max_batch=B, pool_capacity=1 << 21)
    t.set_anchor_mode(True)
    t.set_dive(dive)
    if record:
        t.set_tree_record(True)
    return t


def timed_solve(ctx, t, B):
    ctx.sync()
    t0 = time.perf_counter()
    st = t.solve(mip_gap=1e-9, frontier_batch=B, max_seconds=LIMIT)
    ctx.sync()
    return st, time.perf_counter() - t0


def child(n, m, B, dive, seed):
    import numpy as np
    from simple_mip_solver_amd import _ffi
    from simple_mip_solver_amd.generators import random_dense_milp_arrays
    ctx = _ffi.default_context()
    A, b, c, l, u, ints = random_dense_milp_arrays(n, m, seed=seed)
    p = _ffi.Problem(ctx, A, b, c)
    src = tree(_ffi, p, ints, l, u, B, dive, True)
    st, dt = timed_solve(ctx, src, B)
    out = dict(n=n, m=m, B=B, dive=dive, source=dict(status=st['status'], evaluated=st['evaluated_nodes'],
                                                       created=st['created_nodes'], seconds=dt), rhs=[])
    rng = np.random.default_rng(seed + 1)
    for kind, b2 in (('noise', b + rng.uniform(-1, 1, m)), ('tighter', b + rng.uniform(0, 2, m)), ('relaxed', b - rng.uniform(0, 2, m))):
        p2 = _ffi.Problem(ctx, A, b2, c)
        ctx.sync()
        t0 = time.perf_counter()
        t = _ffi.Tree.restart(src, p2)
        t.set_anchor_mode(True)
        t.set_dive(dive)
        ctx.sync()
        made = time.perf_counter() - t0
        rst, rdt = timed_solve(ctx, t, B)
        stats = t.restart_stats()
        seeds = t.restart_seeds()
        t.close()
        g0 = time.perf_counter()
        src.node_bounds(seeds)
        bounds_wall = time.perf_counter() - g0
        row = dict(kind=kind, seeds=int(len(seeds)),
                   restart=dict(status=rst['status'], evaluated=rst['evaluated_nodes'], primal=rst['primal_bound'],
                                create_seconds=made, solve_seconds=rdt, seconds=made + rdt),
                   seeding=dict(device_ms=stats['seed_ms'], device_bytes=stats['device_bytes'],
                                node_bounds_wall_ms=1e3 * bounds_wall))
        for name, record in (('cold', False), ('cold_recorded', True)):
            ct = tree(_ffi, p2, ints, l, u, B, dive, record)
            cst, cdt = timed_solve(ctx, ct, B)
            row[name] = dict(status=cst['status'], evaluated=cst['evaluated_nodes'], primal=cst['primal_bound'], seconds=cdt)
            ct.close()
        row['restart_over_cold_seconds'] = row['restart']['seconds'] / row['cold']['seconds']
        row['restart_over_cold_nodes'] = row['restart']['evaluated'] / max(1, row['cold']['evaluated'])
        out['rhs'].append(row)
        p2.close()
    print(json.dumps(out))
    src.close()
    p.close()


def main():
    args = sys.argv[1:4] + ['1024', '2', '0'][len(sys.argv[1:4]):]
    for n, m in SIZES:
        run = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', str(n), str(m)] + args,
                             capture_output=True, text=True, timeout=600)
        if run.returncode != 0:   # (a failed size ends the script: nothing more is started on the GPU)
            sys.stderr.write(run.stderr[-4000:])
            sys.exit(f'{n}x{m}: exit status {run.returncode}')
        print(run.stdout.strip().splitlines()[-1], flush=True)


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--child':
        child(*(int(a) for a in sys.argv[2:7]))
    else:
        main()
