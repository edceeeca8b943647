"""Stand-alone use of the GPU weighted row repair (include/mipx_wrepair.h) for users of lp_batch or of a loop of their
own: make integer-feasible points out of LP points of a model, without an LP."""
import numpy as np

from simple_mip_solver_amd.milp_instance import MILPInstance


def weighted_repair(bb_or_model, X, max_steps=256, tol=1e-9):
    """Repair the points X ((batch, n) or (n,)) of a BranchAndBound's root problem or of a MILPInstance, one GPU
    workgroup per point (mipx_weighted_repair_batch): the integer columns are rounded, then unit moves of one integer
    column lower the violation of the rows, each row weighted; where no move lowers it, the weights of the violated
    rows go up by one.  At most max_steps moves and bumps per point.

    Returns (X', obj, status, counts): the points (batch, n); their objectives c . x' with c = lp.objective (in the
    minimisation form the solver works on); status per point 0 feasible (every row within tol, the integer columns
    integral and inside their bounds, the others unchanged) or 2 capped (the point comes back unchanged, obj 0);
    counts (batch, 2): moves and bumps."""
    from simple_mip_solver_amd.lp import get_backend, HipBackend
    if isinstance(bb_or_model, MILPInstance):
        lp, ints = bb_or_model.lp, bb_or_model.integerIndices
    else:
        assert hasattr(bb_or_model, 'root_node') and hasattr(bb_or_model, 'model'), \
            'weighted_repair takes a BranchAndBound or a MILPInstance'
        lp, ints = bb_or_model.root_node.lp, bb_or_model.model.integerIndices
    backend = get_backend()
    assert isinstance(backend, HipBackend), 'weighted_repair needs the HIP backend'
    assert tol >= 0, 'tol is not negative'
    assert isinstance(max_steps, int) and not isinstance(max_steps, bool) and max_steps >= 0, 'max_steps is a count of steps'
    rs = lp._engine_form()
    X = np.asarray(X, dtype=np.float64)
    assert X.ndim in (1, 2) and X.shape[-1] == rs.A.shape[1], 'X holds one point of n columns per row'
    problem = backend._problem(rs.A, rs.b, rs.c, rs.key)
    l, u = lp._bounds()
    out = problem.weighted_repair_batch(X.reshape(-1, rs.A.shape[1]), l, u, sorted(set(int(j) for j in ints)), tol=tol,
                                        max_steps=max_steps)
    return out['x'], out['obj'], out['status'], out['counts']
