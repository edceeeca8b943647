"""Stand-alone use of the GPU bound propagation (include/mipx_prop.h) for users of lp_batch or of a loop of their
own: tighten the bounds of node boxes of a model from its rows before their LPs are solved."""
import numpy as np

from simple_mip_solver_amd.milp_instance import MILPInstance


def propagate_bounds(bb_or_model, L, U, cutoff=None, max_rounds=8):
    """Propagate the boxes L <= x <= U ((batch, n) or (n,) each) of a BranchAndBound's root problem or of a
    MILPInstance over its rows, one GPU workgroup per box (mipx_propagate_batch).

    Returns (L', U', status, changed, rounds): the tightened boxes (batch, n); status per box 0 unchanged,
    1 tightened, 2 infeasible (no integer-feasible point in the box, or none with an objective of at most
    `cutoff`; its bounds come back as they went in); the number of bounds changed; the rounds run.  Only the
    bounds of integer columns are tightened.  cutoff is an objective value in the minimisation form the solver
    works on (c . x with c = lp.objective), None for none; max_rounds caps the rounds per box."""
    from simple_mip_solver_amd.lp import get_backend, HipBackend
    if isinstance(bb_or_model, MILPInstance):
        lp, ints = bb_or_model.lp, bb_or_model.integerIndices
    else:
        assert hasattr(bb_or_model, 'root_node') and hasattr(bb_or_model, 'model'), \
            'propagate_bounds takes a BranchAndBound or a MILPInstance'
        lp, ints = bb_or_model.root_node.lp, bb_or_model.model.integerIndices
    backend = get_backend()
    assert isinstance(backend, HipBackend), 'propagate_bounds needs the HIP backend'
    assert isinstance(max_rounds, int) and not isinstance(max_rounds, bool) and max_rounds >= 1, \
        'max_rounds is a positive number of rounds'
    assert cutoff is None or not np.isnan(cutoff), 'cutoff is None or an objective value'
    rs = lp._engine_form()
    n = rs.A.shape[1]
    L, U = np.asarray(L, dtype=np.float64), np.asarray(U, dtype=np.float64)
    assert L.shape == U.shape and L.ndim in (1, 2) and L.shape[-1] == n, 'L and U hold one box of n columns per row'
    problem = backend._problem(rs.A, rs.b, rs.c, rs.key)
    out = problem.propagate_batch(L.reshape(-1, n), U.reshape(-1, n), sorted(set(int(j) for j in ints)), cutoff=cutoff,
                                  max_rounds=max_rounds)
    return out['l'], out['u'], out['status'], out['changed'], out['rounds']
