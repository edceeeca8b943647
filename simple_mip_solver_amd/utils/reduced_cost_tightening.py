"""Stand-alone use of the GPU reduced-cost bound tightening (include/mipx_rcfix.h) for users of lp_batch or of a loop
of their own: tighten the bounds of node boxes of a model from the row duals of their LPs and an incumbent."""
import numpy as np

from simple_mip_solver_amd.milp_instance import MILPInstance


def tighten_by_reduced_costs(bb_or_model, L, U, Y, cutoff):
    """Tighten the boxes L <= x <= U ((batch, n) or (n,) each) of a BranchAndBound's root problem or of a
    MILPInstance from the row duals Y ((batch, m) or (m,)) of their LPs, one GPU workgroup per box
    (mipx_reduced_cost_tighten_batch).

    Returns (L', U', z, status, changed): the tightened boxes (batch, n); the bound z the duals give on c . x over
    each box; status per box 0 unchanged, 1 tightened, 2 cut off (no point of the box satisfies the rows with an
    objective of at most `cutoff`; its bounds come back as they went in), 3 no bound (an infinite cutoff, or duals
    that give none); the number of bounds changed.  Only the bounds of integer columns are tightened.  Y are duals of
    the rows in the form the solver works on (A x >= b, minimisation: what lp_solve_batch returns), and any vectors
    are safe: negative and NaN entries count as 0.  cutoff is an objective value in that form (c . x with
    c = lp.objective), typically the incumbent's."""
    from simple_mip_solver_amd.lp import get_backend, HipBackend
    if isinstance(bb_or_model, MILPInstance):
        lp, ints = bb_or_model.lp, bb_or_model.integerIndices
    else:
        assert hasattr(bb_or_model, 'root_node') and hasattr(bb_or_model, 'model'), \
            'tighten_by_reduced_costs takes a BranchAndBound or a MILPInstance'
        lp, ints = bb_or_model.root_node.lp, bb_or_model.model.integerIndices
    backend = get_backend()
    assert isinstance(backend, HipBackend), 'tighten_by_reduced_costs needs the HIP backend'
    assert cutoff is not None and not np.isnan(cutoff), 'cutoff is an objective value'
    rs = lp._engine_form()
    m, n = rs.A.shape
    L, U, Y = np.asarray(L, dtype=np.float64), np.asarray(U, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    assert L.shape == U.shape and L.ndim in (1, 2) and L.shape[-1] == n, 'L and U hold one box of n columns per row'
    assert Y.ndim == L.ndim and Y.shape[-1] == m and Y.shape[:-1] == L.shape[:-1], 'Y holds one vector of m duals per box'
    problem = backend._problem(rs.A, rs.b, rs.c, rs.key)
    out = problem.reduced_cost_tighten_batch(L.reshape(-1, n), U.reshape(-1, n), Y.reshape(-1, m),
                                             sorted(set(int(j) for j in ints)), cutoff)
    return out['l'], out['u'], out['z'], out['status'], out['changed']
