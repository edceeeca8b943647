"""Stand-alone use of the GPU pair-move local search (include/mipx_lsearch.h) for users of lp_batch or of a loop of
their own: improve feasible integral points of a model by unit moves of one or two integer columns."""
import numpy as np

from simple_mip_solver_amd.milp_instance import MILPInstance


def pair_search(bb_or_model, X, tol=1e-9, max_moves=64):
    """Improve the points X ((batch, n) or (n,)) of a BranchAndBound's root problem or of a MILPInstance, one GPU
    workgroup per point (mipx_pair_search_batch).

    Returns (X', obj, status, moves): the points (batch, n); their objectives in the minimisation form the solver
    works on (c . x' with c = lp.objective); status per point 0 local optimum (no move of one integer column or of
    two by one unit lowers the objective and keeps every row), 1 capped (max_moves made and a move remains), 2 not
    feasible (a row violated by more than tol, or an integer column fractional or outside its bounds: the point
    comes back as it went in); moves (batch, 2): single and pair moves.  Only integer columns move."""
    from simple_mip_solver_amd.lp import get_backend, HipBackend
    if isinstance(bb_or_model, MILPInstance):
        lp, ints = bb_or_model.lp, bb_or_model.integerIndices
    else:
        assert hasattr(bb_or_model, 'root_node') and hasattr(bb_or_model, 'model'), \
            'pair_search takes a BranchAndBound or a MILPInstance'
        lp, ints = bb_or_model.root_node.lp, bb_or_model.model.integerIndices
    backend = get_backend()
    assert isinstance(backend, HipBackend), 'pair_search needs the HIP backend'
    assert tol >= 0, 'tol is not negative'
    assert isinstance(max_moves, int) and not isinstance(max_moves, bool) and max_moves >= 0, 'max_moves is a count of moves'
    rs = lp._engine_form()
    X = np.asarray(X, dtype=np.float64)
    assert X.ndim in (1, 2) and X.shape[-1] == rs.A.shape[1], 'X holds one point of n columns per row'
    problem = backend._problem(rs.A, rs.b, rs.c, rs.key)
    l, u = lp._bounds()
    out = problem.pair_search_batch(X.reshape(-1, rs.A.shape[1]), l, u, sorted(set(int(j) for j in ints)), tol=tol,
                                    max_moves=max_moves)
    return out['x'], out['obj'], out['status'], out['moves']
