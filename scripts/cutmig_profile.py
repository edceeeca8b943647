"""One donation of open nodes with cut rows through mipx_tree_migrate_self (include/mipx_cutmig.h).

Grows a tree with cut rounds on an unboxed random instance (default 256 x 128, seed 1, where a few open nodes
carry cut rows; 64 32 5 gives more), then moves up to 4096 nodes to its own rank and back over the custom transport (a device copy).  The
share of open nodes that carry cut rows peaks early and falls as the tree grows, so a first pass records it
per step and a second pass, the same deterministic search, stops at the step where most open nodes carry
rows.  Run it under `rocprofv3 --kernel-trace --stats -- python3 scripts/cutmig_profile.py` for the times of
cutmig_lists / pack_nodes / cutmig_gather / unpack_nodes / cutmig_unpack_lists / cutmig_scatter.  Prints the
planned message size per donation and what moved.

usage: python3 scripts/cutmig_profile.py [n m seed (256 128 1)] [frontier batch (512)] [region rows (65536)]
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simple_mip_solver_amd import _ffi  # noqa: E402
from simple_mip_solver_amd.generators import random_dense_milp_arrays  # noqa: E402


def message_bytes(n, m, kc, amount, ctab):
    """The planned size of one cut-mode donation (the layout in tree_engine.hip.h, mig_layout)."""
    pad8 = lambda b: (b + 7) // 8 * 8
    rowbytes = 16 * n + pad8(n + m + kc)
    return amount * rowbytes + pad8(amount * (1 + kc) * 4) + ctab * (n + 1) * 8 + (1 + 6 * amount + 1) * 8


def main():
    a = [int(v) for v in sys.argv[1:]]
    n, m, seed = a[:3] if len(a) >= 3 else (256, 128, 1)
    B = a[3] if len(a) > 3 else 512
    rows = a[4] if len(a) > 4 else 1 << 16
    amount, cap = 4096, 1 << 16
    ctx = _ffi.default_context()
    A, b, c, l, u, ints = random_dense_milp_arrays(n, m, density=1.0, seed=seed)
    u = np.full(n, np.inf)
    prob = _ffi.Problem(ctx, A, b, c)

    def grow(stop_at=None):
        t = _ffi.Tree(prob, ints, l, u, branch_rule='pseudo cost', max_batch=B, pool_capacity=1 << 17,
                      cut_params=dict(max_abs_coef=1000.0 * float(np.max(np.abs(A)))))
        t.set_cut_migration(rows)
        st, seen, t0 = t.stats(), [], time.time()
        while st['open_nodes'] < cap and time.time() - t0 < 60 and len(seen) != stop_at:
            st = t.solve(mip_gap=0.0, frontier_batch=B, max_steps=1)
            if st['status'] != 4:
                break
            seen.append(int(np.sum(t.peek_cuts(st['open_nodes'])[1] > 0)))
        return t, st, seen
    t, _, seen = grow()
    t.close()
    best = int(np.argmax(seen)) + 1
    t, st, seen2 = grow(best)
    assert seen2 == seen[:best], (seen2, seen[:best])   # the same search
    kc = _ffi.lib().mipx_tree_cut_rows_per_node(t._h)
    comm = _ffi.Comm(ctx, 0, 1, allgather=lambda x: [x], send=lambda p, d: None, recv=lambda p, k: b'')
    t.keep_shard(0, 1)
    t.set_comm(comm, 3)
    ctab = min(rows, 1 << 14, amount * kc)
    t1 = time.perf_counter()
    moved = t.migrate_self(amount)
    wall = time.perf_counter() - t1
    s = t.cut_migration_stats()
    print(json.dumps(dict(shape=[n, m, seed], batch=B, carrying_per_step=seen, steps=best, open_nodes=st['open_nodes'],
                          open_with_cut_rows=seen[best - 1], kc=kc, moved=moved, **s, planned_table_rows=ctab,
                          message_bytes=message_bytes(n, m, kc, amount, ctab), migrate_self_ms=round(wall * 1e3, 3))))
    t.set_comm(None)
    t.close()
    comm.close()
    prob.close()


if __name__ == '__main__':
    main()
