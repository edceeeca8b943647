"""Stand-alone use of the GPU LP dive (include/mipx_lpdive.h) for users of lp_batch or of a loop of their own: from LP
points of a model, fix one integer column per point, re-solve all the points' LPs in one launch, and repeat until every
integer column is integral."""
import numpy as np

from simple_mip_solver_amd.milp_instance import MILPInstance


def lp_dive(bb_or_model, X, L=None, U=None, vstat=None, cutoff=np.inf, max_rounds=64, rule='fractional'):
    """Dive from the LP points X ((batch, n) or (n,)) of a BranchAndBound's root problem or of a MILPInstance on the
    GPU (mipx_lpdive_batch).  L, U: the boxes the points are LP optima over ((batch, n), or (n,) for all of them;
    None: the root's bounds); vstat: the basis codes of those LPs ((batch, n + m)) where known -- the first re-solve
    is then warm; cutoff: a dive whose LP objective is not below it is given up; max_rounds: 1..1024 LPs per point;
    rule: 'fractional' (fix the least fractional column at its nearest integer) or 'coefficient' (fix the column with
    the fewest rows against its cheaper direction, in that direction).

    Returns (X', obj, status, rounds, fixings, flips, pivots): the points (batch, n); their objectives c . x' with
    c = lp.objective (in the minimisation form the solver works on); status per point 0 feasible (integral, every row
    and bound within 1e-6, obj the LP's optimum for its integers), 1 infeasible (an LP and the one flip of its last
    fixing both were), 2 the round cap or an LP's iteration limit, 3 skipped (a point that is not finite, an integer
    column with a fractional or infinite bound), 4 rejected (the last LP said optimal, the recomputed point does not
    hold), 5 cutoff; a point that is not feasible comes back unchanged with obj 0; the LPs solved, the columns fixed,
    the fixings flipped and the tableau pivots of each dive."""
    from simple_mip_solver_amd import _ffi
    from simple_mip_solver_amd.lp import get_backend, HipBackend
    if isinstance(bb_or_model, MILPInstance):
        lp, ints = bb_or_model.lp, bb_or_model.integerIndices
    else:
        assert hasattr(bb_or_model, 'root_node') and hasattr(bb_or_model, 'model'), \
            'lp_dive takes a BranchAndBound or a MILPInstance'
        lp, ints = bb_or_model.root_node.lp, bb_or_model.model.integerIndices
    backend = get_backend()
    assert isinstance(backend, HipBackend), 'lp_dive needs the HIP backend'
    assert rule in _ffi.LPDIVE_RULES, "rule is 'fractional' or 'coefficient'"
    assert isinstance(max_rounds, int) and 1 <= max_rounds <= _ffi.MAX_LP_DIVE_ROUNDS, 'max_rounds is 1..1024'
    rs = lp._engine_form()
    n = rs.A.shape[1]
    X = np.asarray(X, dtype=np.float64)
    assert X.ndim in (1, 2) and X.shape[-1] == n, 'X holds one point of n columns per row'
    X = X.reshape(-1, n)
    l, u = lp._bounds()
    L = np.broadcast_to(np.asarray(l if L is None else L, dtype=np.float64), X.shape)
    U = np.broadcast_to(np.asarray(u if U is None else U, dtype=np.float64), X.shape)
    problem = backend._problem(rs.A, rs.b, rs.c, rs.key)
    out = problem.lpdive_batch(X, L, U, sorted(set(int(j) for j in ints)), vstat=vstat, cutoff=cutoff, max_rounds=max_rounds,
                               rule=_ffi.LPDIVE_RULES[rule])
    return out['x'], out['obj'], out['status'], out['rounds'], out['fixings'], out['flips'], out['pivots']
