"""Stand-alone use of the GPU cube search (include/mipx_cube.h) for users of lp_batch or of a loop of their own: try
every rounding of the most fractional columns of LP points of a model, without an LP."""
import numpy as np

from simple_mip_solver_amd.milp_instance import MILPInstance


def cube_search(bb_or_model, X, cutoff=np.inf, max_columns=16, tol=1e-9, ftol=1e-4):
    """Search the cubes of the points X ((batch, n) or (n,)) of a BranchAndBound's root problem or of a MILPInstance
    on the GPU (mipx_cube_search_batch): the at most max_columns (1..20) integer columns of a point that lie farthest
    from an integer (farther than ftol) are rounded down and up in every combination, every other integer column
    is rounded to the nearest integer inside its bounds, and the combination of the smallest objective that
    satisfies every row within tol and lies below cutoff is the point's result.

    Returns (X', obj, status, counts): the points (batch, n); their objectives c . x' with c = lp.objective (in the
    minimisation form the solver works on); status per point 0 found (every row within tol, the integer columns
    integral and inside their bounds, the others unchanged, obj < cutoff) or 1 none (the point comes back
    unchanged, obj 0); counts (batch, 2): the number of columns enumerated and the code picked (bit t raises the
    t-th of them, in ascending column order; -1 for none)."""
    from simple_mip_solver_amd.lp import get_backend, HipBackend
    if isinstance(bb_or_model, MILPInstance):
        lp, ints = bb_or_model.lp, bb_or_model.integerIndices
    else:
        assert hasattr(bb_or_model, 'root_node') and hasattr(bb_or_model, 'model'), \
            'cube_search takes a BranchAndBound or a MILPInstance'
        lp, ints = bb_or_model.root_node.lp, bb_or_model.model.integerIndices
    backend = get_backend()
    assert isinstance(backend, HipBackend), 'cube_search needs the HIP backend'
    assert tol >= 0 and ftol >= 0, 'tol and ftol are not negative'
    assert isinstance(max_columns, int) and not isinstance(max_columns, bool) and 1 <= max_columns <= 20, \
        'max_columns is a number of columns from 1 to 20'
    assert not np.isnan(cutoff), 'cutoff is a number (inf for none)'
    rs = lp._engine_form()
    X = np.asarray(X, dtype=np.float64)
    assert X.ndim in (1, 2) and X.shape[-1] == rs.A.shape[1], 'X holds one point of n columns per row'
    problem = backend._problem(rs.A, rs.b, rs.c, rs.key)
    l, u = lp._bounds()
    out = problem.cube_search_batch(X.reshape(-1, rs.A.shape[1]), l, u, sorted(set(int(j) for j in ints)), cutoff=cutoff,
                                    tol=tol, ftol=ftol, max_columns=max_columns)
    return out['x'], out['obj'], out['status'], out['counts']
