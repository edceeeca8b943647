"""Stand-alone use of the GPU primal heuristic (include/mipx_heur.h) for users of lp_batch or of a loop of their
own: round LP points of a model, repair the rows the rounding broke, lift the objective."""
import numpy as np

from simple_mip_solver_amd.milp_instance import MILPInstance


def round_repair_lift(bb_or_model, X, tol=1e-9, max_moves=None):
    """Round, repair and lift the points X ((batch, n) or (n,)) of a BranchAndBound's root problem or of a
    MILPInstance, one GPU workgroup per point (mipx_round_repair_batch).

    Returns (X~, obj, status, moves): the points (batch, n); their objectives in the minimisation form the solver
    works on (c . x~ with c = lp.objective); status per point 0 feasible (every row within tol, integer columns
    integral and inside their bounds), 1 stuck (no unit move lowers the violation), 2 capped (max_moves reached
    with a row still violated); moves (batch, 2): repair and lift moves.  max_moves None: rows + columns."""
    from simple_mip_solver_amd.lp import get_backend, HipBackend
    if isinstance(bb_or_model, MILPInstance):
        lp, ints = bb_or_model.lp, bb_or_model.integerIndices
    else:
        assert hasattr(bb_or_model, 'root_node') and hasattr(bb_or_model, 'model'), \
            'round_repair_lift takes a BranchAndBound or a MILPInstance'
        lp, ints = bb_or_model.root_node.lp, bb_or_model.model.integerIndices
    backend = get_backend()
    assert isinstance(backend, HipBackend), 'round_repair_lift needs the HIP backend'
    assert tol >= 0, 'tol is not negative'
    assert max_moves is None or (isinstance(max_moves, int) and max_moves >= 0), 'max_moves is None or a count of moves'
    rs = lp._engine_form()
    X = np.asarray(X, dtype=np.float64)
    assert X.ndim in (1, 2) and X.shape[-1] == rs.A.shape[1], 'X holds one point of n columns per row'
    problem = backend._problem(rs.A, rs.b, rs.c, rs.key)
    l, u = lp._bounds()
    out = problem.round_repair_batch(X.reshape(-1, rs.A.shape[1]), l, u, sorted(set(int(j) for j in ints)), tol=tol,
                                     max_moves=max_moves)
    return out['x'], out['obj'], out['status'], out['moves']
