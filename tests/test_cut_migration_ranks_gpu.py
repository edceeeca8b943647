"""Two ranks with cut rounds and cut migration (include/mipx_cutmig.h): two PROCESSES sharing the one GPU,
the exchange protocol over the custom transport (gloo underneath, tests/support/gloo_comm.py), as in
tests/test_parallel_gpu.py -- a rehearsal on one GPU, never a measurement.

On an instance whose open nodes carry cut rows, a rank that starts without open nodes is fed by the other:
nodes arrive with their cut rows, and both ranks end with the same incumbent and solution, bit for bit.  The
objective is never better than the cut-free optimum (cut rounds can lose it: DESIGN.md section 7) and the
solution is integral and feasible.  The same through BranchAndBound(comm=..., cut_migration=True).  A rank
with cut migration off beside a peer with it on: no node moves, and the ranks still agree."""
import textwrap

import pytest

from tests.test_parallel_cpu import ROOT, run_two_ranks

pytestmark = pytest.mark.gpu

WORKER = textwrap.dedent('''
    import os, sys
    sys.path.insert(0, {root!r})
    import numpy as np
    import torch.distributed as dist
    dist.init_process_group('gloo')
    os.environ['LOCAL_RANK'] = '0'                 # (one GPU on the box: both ranks use device 0)
    from simple_mip_solver_amd import _ffi, BranchAndBound, PseudoCostBranchNode, MILPInstance
    from simple_mip_solver_amd.generators import random_dense_milp_arrays
    from tests.support.gloo_comm import make_comm
    rank = dist.get_rank()
    ctx = _ffi.Context(0)                          # both ranks on the one GPU: a rehearsal
    comm = make_comm(ctx)
    n, m, B = 40, 16, 16
    A, b, c, l, u, ints = random_dense_milp_arrays(n, m, seed=3)
    u = np.full(n, np.inf)                         # unboxed: most open nodes carry cut rows
    prob = _ffi.Problem(ctx, A, b, c)
    mac = 1000.0 * float(np.max(np.abs(A)))
    plain = _ffi.Tree(prob, ints, l, u, branch_rule='pseudo cost', max_batch=B, pool_capacity=1 << 15)
    ref = plain.solve(mip_gap=1e-4, frontier_batch=B)
    assert ref['status'] == 1
    plain.close()

    def check_answer(value, x):
        assert value >= ref['primal_bound'] - 1e-9, (value, ref['primal_bound'])   # never better than the optimum
        assert np.max(np.abs(x[ints] - np.round(x[ints]))) <= 1e-4
        assert np.all(A @ x >= b - 1e-6) and np.all(x >= l - 1e-9)
        assert abs(float(c @ x) - value) < 1e-6

    def dry_rank_fed(on):
        t = _ffi.Tree(prob, ints, l, u, branch_rule='pseudo cost', max_batch=B, pool_capacity=1 << 15,
                      cut_params=dict(max_abs_coef=mac))
        if on:
            t.set_cut_migration(True)
        stx = t.stats()
        while stx['open_nodes'] < 4 * B:
            stx = t.solve(mip_gap=0.0, frontier_batch=B, max_steps=1)
        held = t.peek_cuts(stx['open_nodes'])[1]
        assert np.sum(held > 0) > 0                # the nodes rank 0 will hand out carry cut rows
        if rank == 0:
            t.keep_shard(0, 1)                      # everything
        else:
            t.keep_shard(999983, 1000003)           # nothing
            assert t.stats()['open_nodes'] == 0
        t.set_comm(comm, 3)
        st = t.solve(mip_gap=1e-4, frontier_batch=B)
        g, cm, x = t.global_stats(), t.cut_migration_stats(), t.solution()
        t.set_comm(None)
        t.close()
        return st, g, cm, x

    # --- both ranks with cut migration: the dry rank is fed, nodes arrive with their cut rows ----------
    st, g, cm, x = dry_rank_fed(True)
    assert st['status'] == 1, st
    check_answer(st['primal_bound'], x)
    both = comm.allgather(np.concatenate([[st['primal_bound'], st['dual_bound'], g['evaluated_nodes'], g['incumbent_rank'],
                                           st['status']], x]))
    assert np.array_equal(both[0], both[1]), both   # the same answer, bit for bit, on both ranks
    moved = comm.allgather(np.array([g['nodes_sent'], g['nodes_received'], cm['nodes_sent_with_cuts'],
                                     cm['cut_rows_sent'], cm['cut_rows_received'], cm['region_rows_used']], float))
    assert moved[1, 1] > 0 and moved[1, 4] > 0, moved        # the dry rank got nodes, and cut rows with them
    assert moved[:, 0].sum() == moved[:, 1].sum() and moved[:, 3].sum() == moved[:, 4].sum(), moved
    assert np.array_equal(moved[:, 4], moved[:, 5]) and moved[:, 2].sum() > 0
    sys.stdout.write('rank%d fed: %s\\n' % (rank, moved[rank].tolist()))

    # --- a rank with cut migration off beside one with it on: nothing moves, the ranks still agree -------
    st, g, cm, x = dry_rank_fed(rank == 0)
    assert st['status'] == 1, st
    check_answer(st['primal_bound'], x)
    both = comm.allgather(np.concatenate([[st['primal_bound'], st['status'], g['nodes_sent'], g['nodes_received'],
                                           cm['cut_rows_received']], x]))
    assert np.array_equal(both[0], both[1]), both
    assert both[0][2] == both[0][3] == 0             # no node moved in either direction

    # --- through the driver -----------------------------------------------------------------------
    make = lambda: MILPInstance(A=A, b=b, c=c, l=l, u=u, sense=['Min', '>='], integerIndices=ints, numVars=n)
    bb = BranchAndBound(make(), PseudoCostBranchNode, pseudo_costs={{}}, frontier_batch=B,
                        comm=make_comm(_ffi.default_context()), exchange_every=3, cut_migration=True)
    bb.solve()
    assert bb.status == 'optimal' and bb.solution is not None
    check_answer(bb.objective_value, bb.solution)
    agree = comm.allgather(np.concatenate([[bb.objective_value, bb.evaluated_nodes], bb.solution]))
    assert np.array_equal(agree[0], agree[1]) and bb._native_global['world'] == 2
    s = bb.cut_migration_stats
    assert set(s) == {{'nodes_sent_with_cuts', 'cut_rows_sent', 'cut_rows_received', 'region_rows_used'}}
    totals = comm.allgather(np.array([s['cut_rows_sent'], s['cut_rows_received']], float))
    assert totals[:, 0].sum() == totals[:, 1].sum()
    comm.barrier()
    dist.destroy_process_group()
    sys.stdout.write('rank%dok\\n' % rank)
    sys.stdout.flush()
''')


def test_two_ranks_migrate_cut_rows_rehearsal(tmp_path):
    script = tmp_path / 'worker.py'
    script.write_text(WORKER.format(root=ROOT))
    res = run_two_ranks(script, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-6000:]
    assert 'rank0ok' in res.stdout and 'rank1ok' in res.stdout
