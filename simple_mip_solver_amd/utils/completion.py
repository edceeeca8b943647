"""Stand-alone use of the GPU completion (include/mipx_complete.h) for users of lp_batch or of a loop of their own:
hold the integer columns of points of a model where they are and solve the LP over the continuous columns, a batch of
points in one launch."""
import numpy as np

from simple_mip_solver_amd.milp_instance import MILPInstance


def complete_continuous(bb_or_model, X, vstat=None, ctol=1e-6):
    """Complete the points X ((batch, n) or (n,)) of a BranchAndBound's root problem or of a MILPInstance on the GPU
    (mipx_complete_batch): every integer column of a point is fixed at its value, the other columns get the root's
    bounds, and the LP over them is solved by the node-LP kernel -- warm from the basis codes vstat ((batch, n + m),
    e.g. those of the node LP a point was rounded from) where given, cold otherwise.

    Returns (X', obj, status, pivots): the points (batch, n); their objectives c . x' with c = lp.objective (in the
    minimisation form the solver works on); status per point 0 completed (every row and every bound of a continuous
    column within ctol, the integer columns as they came, obj the LP's optimum for them), 1 the LP is infeasible,
    2 it hit its iteration limit or is unbounded, 3 skipped (an integer column is fractional or outside its bounds),
    4 rejected (the LP said optimal, the recomputed point does not hold); a point that is not completed comes back
    unchanged with obj 0; pivots: the tableau pivots of each LP."""
    from simple_mip_solver_amd.lp import get_backend, HipBackend
    if isinstance(bb_or_model, MILPInstance):
        lp, ints = bb_or_model.lp, bb_or_model.integerIndices
    else:
        assert hasattr(bb_or_model, 'root_node') and hasattr(bb_or_model, 'model'), \
            'complete_continuous takes a BranchAndBound or a MILPInstance'
        lp, ints = bb_or_model.root_node.lp, bb_or_model.model.integerIndices
    backend = get_backend()
    assert isinstance(backend, HipBackend), 'complete_continuous needs the HIP backend'
    assert ctol >= 0, 'ctol is not negative'
    rs = lp._engine_form()
    X = np.asarray(X, dtype=np.float64)
    assert X.ndim in (1, 2) and X.shape[-1] == rs.A.shape[1], 'X holds one point of n columns per row'
    problem = backend._problem(rs.A, rs.b, rs.c, rs.key)
    l, u = lp._bounds()
    out = problem.complete_batch(X.reshape(-1, rs.A.shape[1]), l, u, sorted(set(int(j) for j in ints)), vstat=vstat, ctol=ctol)
    return out['x'], out['obj'], out['status'], out['pivots']
