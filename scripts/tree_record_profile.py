"""Cost of the tree record (include/mipx_treerec.h) on a frontier-engine search, on the bench's instance:
ms per step with recording off (device finish), with MIPX_HOST_FINISH=1 and recording off, and with recording
on; then the two queries for all leaves of the recorded tree (nodes per second, device time from the stats).
The comparison that matters is recording on against the host finish with recording off: the record forces the
host finish, and should cost little beyond it.  Prints one JSON line.

    python3 scripts/tree_record_profile.py [n m B dive steps]     (default: 256 128 8192 8 10)

Every measurement runs in a child process of its own under a time limit; the first one that fails ends the
script.
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = (('off_device_finish', {}, 300), ('off_host_finish', {'MIPX_HOST_FINISH': '1'}, 300), ('on', {}, 600))


def child(mode, n, m, B, dive, steps):
    import numpy as np
    from simple_mip_solver_amd import _ffi
    from simple_mip_solver_amd.generators import random_dense_milp_arrays
    ctx = _ffi.default_context()
    A, b, c, l, u, ints = random_dense_milp_arrays(n, m, seed=0)
    pool = max(1 << 16, 3 * B * (2 * (1 + dive) + 1) * 8)
    p = _ffi.Problem(ctx, A, b, c)
    t = _ffi.Tree(p, ints, l, u, branch_rule='pseudo cost', max_batch=B, pool_capacity=pool)
    t.set_anchor_mode(True)
    t.set_dive(dive)
    if mode == 'on':
        t.set_tree_record(True)
    st = t.stats()
    while st['open_nodes'] < B and st['status'] in (0, 4):   # ramp-up as the bench's: up to a full batch
        st = t.solve(mip_gap=0.0, frontier_batch=min(B, 256), max_steps=1)
    ctx.sync()
    t0 = time.perf_counter()
    st2 = t.solve(mip_gap=0.0, frontier_batch=B, max_steps=steps)
    ctx.sync()
    dt = time.perf_counter() - t0
    out = dict(ms_per_step=1e3 * dt / steps, lps=st2['lp_solved'] - st['lp_solved'], created_nodes=st2['created_nodes'])
    if mode == 'on':
        rec = t.tree_records()
        leaves = np.flatnonzero((rec['flags'] & _ffi.TR_HAS_CHILDREN) == 0)
        s0 = t.tree_record_stats()
        g0 = time.perf_counter()
        t.node_bounds(leaves)
        g1 = time.perf_counter()
        s1 = t.tree_record_stats()
        res = t.node_solve(leaves, want_x=False, want_vstat=False)
        g2 = time.perf_counter()
        s2 = t.tree_record_stats()
        out['record'] = s2
        out['leaves'] = int(len(leaves))
        out['bounds'] = dict(wall_ms=1e3 * (g1 - g0), device_ms=s1['query_ms'] - s0['query_ms'],
                             nodes_per_s_wall=len(leaves) / (g1 - g0),
                             nodes_per_s_device=len(leaves) / max(1e-9, 1e-3 * (s1['query_ms'] - s0['query_ms'])))
        out['solve'] = dict(wall_ms=1e3 * (g2 - g1), device_ms=s2['query_ms'] - s1['query_ms'],
                            nodes_per_s_wall=len(leaves) / (g2 - g1),
                            nodes_per_s_device=len(leaves) / max(1e-9, 1e-3 * (s2['query_ms'] - s1['query_ms'])),
                            optimal=int((res['status'] == 0).sum()), infeasible=int((res['status'] == 1).sum()))
    print(json.dumps(out))
    t.close()
    p.close()


def main():
    args = sys.argv[1:6] + ['256', '128', '8192', '8', '10'][len(sys.argv[1:6]):]
    out = dict(zip(('n', 'm', 'B', 'dive', 'steps'), (int(a) for a in args)))
    for name, env, limit in STEPS:
        run = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', name] + args, env=dict(os.environ, **env),
                             capture_output=True, text=True, timeout=limit)
        if run.returncode != 0:   # (a failed step ends the script: nothing more is started on the GPU)
            sys.stderr.write(run.stderr[-4000:])
            sys.exit(f'{name}: exit status {run.returncode}')
        out[name] = json.loads(run.stdout.strip().splitlines()[-1])
    out['record_over_host_finish_pct'] = 100.0 * (out['on']['ms_per_step'] / out['off_host_finish']['ms_per_step'] - 1.0)
    out['record_over_device_finish_pct'] = 100.0 * (out['on']['ms_per_step'] / out['off_device_finish']['ms_per_step'] - 1.0)
    print(json.dumps(out))


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--child':
        child(sys.argv[2], *(int(a) for a in sys.argv[3:8]))
    else:
        main()
