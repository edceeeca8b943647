"""Stand-alone use of the GPU fix-and-propagate dive (include/mipx_fixprop.h) for users of lp_batch or of a loop of
their own: make integer-feasible points out of LP points of a model, without an LP."""
import numpy as np

from simple_mip_solver_amd.milp_instance import MILPInstance


def fix_and_propagate(bb_or_model, X, cutoff=np.inf, tol=1e-9, max_rounds=8, max_tries=256):
    """Dive from the points X ((batch, n) or (n,)) of a BranchAndBound's root problem or of a MILPInstance, one GPU
    workgroup per point (mipx_fix_propagate_batch): the integer columns are fixed one after the other, the most
    integral first, each to the value nearest the point that bound propagation over the rows does not refuse; cutoff
    is an objective value (in the minimisation form the solver works on) above which no point is of interest.

    Returns (X', obj, status, counts): the points (batch, n); their objectives c . x' with c = lp.objective; status
    per point 0 feasible (every row within tol, the integer columns integral and inside their bounds), 1 stuck (a
    column none of whose values the propagation accepts), 2 capped (max_tries propagation calls made), 4 the box holds
    no integer point within the cutoff, 5 every integer column is fixed and a row is violated all the same (continuous
    columns stay at their clamped value); counts (batch, 2): fixings and tries.  Only status 0 and 5 change the point."""
    from simple_mip_solver_amd.lp import get_backend, HipBackend
    if isinstance(bb_or_model, MILPInstance):
        lp, ints = bb_or_model.lp, bb_or_model.integerIndices
    else:
        assert hasattr(bb_or_model, 'root_node') and hasattr(bb_or_model, 'model'), \
            'fix_and_propagate takes a BranchAndBound or a MILPInstance'
        lp, ints = bb_or_model.root_node.lp, bb_or_model.model.integerIndices
    backend = get_backend()
    assert isinstance(backend, HipBackend), 'fix_and_propagate needs the HIP backend'
    assert tol >= 0, 'tol is not negative'
    assert isinstance(max_rounds, int) and not isinstance(max_rounds, bool) and max_rounds >= 1, 'max_rounds is a positive count of rounds'
    assert isinstance(max_tries, int) and not isinstance(max_tries, bool) and max_tries >= 0, 'max_tries is a count of tries'
    assert not np.isnan(cutoff), 'cutoff is a number'
    rs = lp._engine_form()
    X = np.asarray(X, dtype=np.float64)
    assert X.ndim in (1, 2) and X.shape[-1] == rs.A.shape[1], 'X holds one point of n columns per row'
    problem = backend._problem(rs.A, rs.b, rs.c, rs.key)
    l, u = lp._bounds()
    out = problem.fix_propagate_batch(X.reshape(-1, rs.A.shape[1]), l, u, sorted(set(int(j) for j in ints)), cutoff=cutoff,
                                      tol=tol, max_rounds=max_rounds, max_tries=max_tries)
    return out['x'], out['obj'], out['status'], out['counts']
