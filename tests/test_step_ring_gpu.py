"""The grow path of the step options' buffers (StepRing::grow in csrc/tree_engine.hip.h, behind every
mipx_tree_set_*): a tree whose heuristic was first set for one point and then for three, with or without a dependent
option that was laid out for the one point in between, searches exactly as a tree set up for three points at once --
the same optimum, the same nodes, the same counters of the option (all but kernel_us, which is a time).  One small
instance of the generator, 12 x 8 at a batch of 4: the search takes several steps and the heuristic's points are capped
by the batch.  That growing the heuristic past an option that is still on is refused is pinned per option in the
options' own test files (their refusal tests)."""
import functools

import pytest

from simple_mip_solver_amd import _ffi
from simple_mip_solver_amd.generators import random_dense_milp_arrays
from tests.support import completion_reference as comp

gpu = pytest.mark.gpu
N, M, SEED, BATCH = 12, 8, 0, 4

# name: (switch the option on, switch it off, its counters, the instance's family)
OPTIONS = {
    'local_search': (lambda t: t.set_local_search(True), lambda t: t.set_local_search(0), lambda t: t.local_search_stats(), 'integer'),
    'fix_propagate': (lambda t: t.set_fix_propagate(True), lambda t: t.set_fix_propagate(0), lambda t: t.fix_propagate_stats(), 'integer'),
    'weighted_repair': (lambda t: t.set_weighted_repair(True), lambda t: t.set_weighted_repair(0), lambda t: t.weighted_repair_stats(), 'integer'),
    'cube_search': (lambda t: t.set_cube_search(True), lambda t: t.set_cube_search(0), lambda t: t.cube_search_stats(), 'integer'),
    'completion': (lambda t: t.set_completion(True), lambda t: t.set_completion(False), lambda t: t.completion_stats(), 'mixed'),
    'lp_dive': (lambda t: t.set_lpdive(8, 1), lambda t: t.set_lpdive(0), lambda t: t.lpdive_stats(), 'integer'),
}


@functools.lru_cache(maxsize=None)
def instance(family):
    """The generator's instance with every column integer, or the completion's mixed family (even columns integer)."""
    if family == 'mixed':
        return comp.mixed(N, M, SEED)
    return random_dense_milp_arrays(N, M, seed=SEED)


def search(ctx, family, setup, stats):
    """One search to the end on a fresh tree that `setup` switched the options of: what it ended with, and `stats`
    without the device time."""
    A, b, c, l, u, ints = instance(family)
    t = _ffi.Tree(_ffi.Problem(ctx, A, b, c), [int(j) for j in ints], l, u, max_batch=BATCH, pool_capacity=1 << 14)
    setup(t)
    st = t.solve(mip_gap=0.0, frontier_batch=BATCH)
    counters = stats(t)
    ran = counters.pop('kernel_us') > 0   # (the option's event pair bracketed launches; the time itself is not compared)
    heur = {k: v for k, v in t.heuristic_stats().items() if k != 'kernel_us'}
    print(family, 'status', st['status'], 'optimum', st['primal_bound'], 'nodes', st['evaluated_nodes'], 'steps', st['steps'],
          'heuristic', heur, 'option', counters)
    return dict(status=st['status'], has_solution=st['has_solution'], optimum=st['primal_bound'], nodes=st['evaluated_nodes'],
                steps=st['steps'], solution=t.solution().tolist() if st['has_solution'] else None, heuristic=heur, option=counters,
                ran=ran)


@gpu
def test_a_heuristic_grown_from_one_point_to_three_searches_as_one_set_for_three(gpu_ctx):
    def grown(t):
        t.set_heuristic(1)
        t.set_heuristic(3)
    fresh = search(gpu_ctx, 'integer', lambda t: t.set_heuristic(3), lambda t: t.heuristic_stats())
    again = search(gpu_ctx, 'integer', grown, lambda t: t.heuristic_stats())
    assert fresh['status'] == 1 and fresh['has_solution'] and fresh['steps'] >= 3   # (solved to the end, over several steps)
    assert fresh['heuristic']['points'] > fresh['steps']                         # (more than one point a step: the three are used)
    assert again == fresh


@gpu
@pytest.mark.parametrize('name', list(OPTIONS))
def test_an_option_laid_out_for_one_point_grows_behind_the_heuristic(name, gpu_ctx):
    on, off, stats, family = OPTIONS[name]

    def direct(t):
        t.set_heuristic(3)
        on(t)

    def grown(t):
        t.set_heuristic(1)
        on(t)    # (the option's buffers: for one point)
        off(t)   # (the buffers stay)
        t.set_heuristic(3)
        on(t)    # (... and grow here, behind the heuristic's)
    fresh = search(gpu_ctx, family, direct, stats)
    again = search(gpu_ctx, family, grown, stats)
    assert fresh['status'] == 1 and fresh['has_solution'] and fresh['steps'] >= 3
    # (the option's kernels ran; the dive and the weighted repair take the points the rounding fails on, which this family
    # has none of: their launches go over the grown buffers all the same, every point SKIPPED)
    assert fresh['ran'] and (fresh['option']['points'] > 0 or name in ('fix_propagate', 'weighted_repair'))
    assert again == fresh


@gpu
def test_propagation_set_twice_searches_as_set_once(gpu_ctx):
    def twice(t):
        t.set_propagation(True)
        t.set_propagation(True)
    fresh = search(gpu_ctx, 'integer', lambda t: t.set_propagation(True), lambda t: t.propagation_stats())
    again = search(gpu_ctx, 'integer', twice, lambda t: t.propagation_stats())
    assert fresh['status'] == 1 and fresh['has_solution'] and fresh['steps'] >= 3
    assert fresh['ran'] and fresh['option']['nodes'] > 0   # (the option ran)
    assert again == fresh
