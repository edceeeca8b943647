"""Lifted knapsack cover cuts (include/mipx_cover.h): stand-alone separation on the GPU for users of lp_batch or of a
loop of their own.  The root cut loop that merges them with the MIR cuts is utils/mir_cuts.root_cut_loop(cover=True),
behind BranchAndBound(root_cuts=..., cover_cuts=True)."""
import numpy as np

from simple_mip_solver_amd.milp_instance import MILPInstance

DEFAULT_MIN_EFFICACY = 1e-6


def separate_covers(bb_or_model, X, L=None, U=None, rows=None, min_efficacy=DEFAULT_MIN_EFFICACY):
    """Lifted cover cuts of a BranchAndBound's root problem or of a MILPInstance at the points X ((batch, n) or (n,))
    inside the boxes L <= x <= U (None: the model's own bounds), one GPU workgroup per point and row
    (mipx_cover_separate_batch).  rows: None for the model's m rows, or the indices of the rows to separate.

    Returns (pi, pi0, efficacy, cover_size, status): the cuts pi . x >= pi0 ((batch, R, n) and (batch, R)), their
    efficacy at the point, the size of the cover and a status per row (0 a cut, 1 no cover, 2 too shallow,
    4 skipped).  With the model's own bounds the cuts are valid for the model, with a node's box for that node."""
    from simple_mip_solver_amd.lp import get_backend, HipBackend
    if isinstance(bb_or_model, MILPInstance):
        lp, ints = bb_or_model.lp, bb_or_model.integerIndices
    else:
        assert hasattr(bb_or_model, 'root_node') and hasattr(bb_or_model, 'model'), \
            'separate_covers takes a BranchAndBound or a MILPInstance'
        lp, ints = bb_or_model.root_node.lp, bb_or_model.model.integerIndices
    backend = get_backend()
    assert isinstance(backend, HipBackend), 'separate_covers needs the HIP backend'
    rs = lp._engine_form()
    m, n = rs.A.shape
    X = np.asarray(X, dtype=np.float64)
    assert X.ndim in (1, 2) and X.shape[-1] == n, 'X holds one point of n columns per row'
    l0, u0 = lp._bounds()
    L = np.broadcast_to(l0, X.shape) if L is None else np.asarray(L, dtype=np.float64)
    U = np.broadcast_to(u0, X.shape) if U is None else np.asarray(U, dtype=np.float64)
    assert L.shape == X.shape and U.shape == X.shape, 'L and U hold one box per point'
    if rows is not None:
        rows = np.asarray(rows)
        assert rows.ndim == 1 and len(rows) >= 1 and np.issubdtype(rows.dtype, np.integer), \
            'rows is a list of row indices'
    ints = sorted(set(int(j) for j in ints))
    problem = backend._problem(rs.A, rs.b, rs.c, rs.key)
    out = problem.cover_separate_batch(X.reshape(-1, n), L.reshape(-1, n), U.reshape(-1, n), ints, rows, min_efficacy)
    return out['pi'], out['pi0'], out['efficacy'], out['cover_size'], out['status']
