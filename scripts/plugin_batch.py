"""A user's Node subclass on C3's instance (256 x 128, seed 0, the bench's generator), gomory_cuts=False:
node LPs per second per-node and with BranchAndBound(lp_batch=B), plus launches, prefetch hit rate
and a host profile of one lp_batch run by phase (pop, pack + launch, bound, branch, put).

usage: python scripts/plugin_batch.py [node_limit] [B ...]"""
import cProfile
import json
import os
import pstats
import sys
import time
from math import ceil, floor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from simple_mip_solver_amd import BaseNode, BranchAndBound, MILPInstance
from simple_mip_solver_amd import lp as lpmod
from simple_mip_solver_amd.generators import random_dense_milp_arrays


class LeastFractionalNode(BaseNode):
    def branch(self, **kwargs):
        frac = self._fractional_indices()
        x = self.solution
        dist = [min(x[i] - floor(x[i]), ceil(x[i]) - x[i]) for i in frac]
        return self._base_branch(frac[int(np.argmin(dist))], **kwargs)

    def __lt__(self, other):
        return (self.dual_bound, -self.depth) < (other.dual_bound, -other.depth)


class Counting(lpmod.HipBackend):
    calls = lps = 0

    def solve(self, A, b, c, l, u, vstat, max_iter, cache_key):
        Counting.calls += 1
        Counting.lps += len(l)
        return super().solve(A, b, c, l, u, vstat, max_iter, cache_key)


def main():
    limit = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
    batches = [int(a) for a in sys.argv[2:]] or [64, 1024, 8192]
    lpmod.set_backend(Counting())
    A, b, c, l, u, ints = random_dense_milp_arrays(256, 128, seed=0)
    model = MILPInstance(A=A, b=b, c=c, l=l, u=u, sense=['Min', '>='], integerIndices=list(ints), numVars=256)
    # context, library load and first launches stay out of the timing
    BranchAndBound(model, LeastFractionalNode, gomory_cuts=False, node_limit=5, lp_batch=4).solve()
    rows = []
    for B in [None] + batches:
        bb = BranchAndBound(model, LeastFractionalNode, gomory_cuts=False, node_limit=limit, lp_batch=B)
        c0, l0 = Counting.calls, Counting.lps
        t0 = time.perf_counter()
        bb.solve()
        dt = time.perf_counter() - t0
        st = bb.lp_batch_stats or {}
        row = dict(lp_batch=B, nodes=bb.evaluated_nodes, lps=Counting.lps - l0, launches=Counting.calls - c0,
                   seconds=round(dt, 3), node_lps_per_s=round((Counting.lps - l0) / dt, 1),
                   hit_rate=round(st['consumed'] / st['prefetched'], 4) if st.get('prefetched') else None,
                   stats=st, status=bb.status, dual_bound=bb.dual_bound, primal_bound=bb.primal_bound)
        rows.append(row)
        print(json.dumps(row), flush=True)
    # where the host time goes in an lp_batch run (cumulative seconds of the driver's phases)
    B = max(batches)
    bb = BranchAndBound(model, LeastFractionalNode, gomory_cuts=False, node_limit=limit, lp_batch=B)
    prof = cProfile.Profile()
    t0 = time.perf_counter()
    prof.enable()
    bb.solve()
    prof.disable()
    dt = time.perf_counter() - t0
    ps = pstats.Stats(prof)
    phase = {}
    for (file, _, fn), (_, _, tt, ct, _) in ps.stats.items():
        key = {('branch_and_bound.py', '_prefetch'): 'pack+launch (prefetch)', ('lp.py', 'solve'): 'launch (engine)',
               ('base_node.py', 'bound'): 'bound', ('branch_and_bound.py', '_process_branch_rtn'): 'branch: put + tree',
               ('plugin_batch.py', 'branch'): 'branch (user)',
               ('queue.py', 'get'): 'pop', ('queue.py', 'put'): 'put', ('lp.py', 'dual'): 'dual (consume)',
               ('lp.py', '_store'): '_store', ('lp.py', '_warm_start'): '_warm_start',
               ('base_node.py', '_base_branch'): '_base_branch (children)'}.get((os.path.basename(file), fn))
        if key:
            phase[key] = round(phase.get(key, 0) + ct, 3)
    print(json.dumps(dict(profile_lp_batch=B, seconds_under_profiler=round(dt, 3), nodes=bb.evaluated_nodes,
                          cumulative_seconds=phase)), flush=True)


if __name__ == '__main__':
    main()
