"""Clique cuts (include/mipx_clique.h): the conflict graph of a model's rows and stand-alone separation on the GPU for
users of lp_batch or of a loop of their own.  The root cut loop that merges them with the MIR and cover cuts is
utils/mir_cuts.root_cut_loop(clique=True), behind BranchAndBound(root_cuts=..., clique_cuts=True)."""
import numpy as np

from simple_mip_solver_amd.milp_instance import MILPInstance

DEFAULT_MIN_EFFICACY = 1e-6


def _problem_of(bb_or_model, who):
    from simple_mip_solver_amd.lp import get_backend, HipBackend
    if isinstance(bb_or_model, MILPInstance):
        lp, ints = bb_or_model.lp, bb_or_model.integerIndices
    else:
        assert hasattr(bb_or_model, 'root_node') and hasattr(bb_or_model, 'model'), \
            f'{who} takes a BranchAndBound or a MILPInstance'
        lp, ints = bb_or_model.root_node.lp, bb_or_model.model.integerIndices
    backend = get_backend()
    assert isinstance(backend, HipBackend), f'{who} needs the HIP backend'
    rs = lp._engine_form()
    l0, u0 = lp._bounds()
    ints = sorted(set(int(j) for j in ints))
    return backend._problem(rs.A, rs.b, rs.c, rs.key), np.asarray(l0, np.float64), np.asarray(u0, np.float64), ints


def unpack_adjacency(adj, n):
    """The packed adjacency ((2n, Wd) uint32 words, literal k in bit k mod 32 of word k div 32) as a boolean (2n, 2n)
    matrix: entry (2j, 2k + 1) says that x_j at its upper and x_k at its lower bound exclude each other."""
    adj = np.ascontiguousarray(adj, dtype=np.uint32)
    assert adj.shape == (2 * n, (2 * n + 31) // 32), 'adj holds 2n rows of ceil(2n / 32) words'
    bits = (adj[:, :, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return bits.reshape(2 * n, -1)[:, :2 * n].astype(bool)


def conflict_graph(bb_or_model, l=None, u=None):
    """The conflict graph of a BranchAndBound's root problem or of a MILPInstance in the box l <= x <= u (None: the
    model's own bounds), one GPU workgroup per row (mipx_clique_graph).  Literal 2j is x_j - l_j, literal 2j + 1 is
    u_j - x_j; two literals are joined when one row alone keeps them from both being 1.  Returns the packed adjacency,
    (2n, ceil(2n / 32)) uint32 words (unpack_adjacency makes a boolean matrix of it)."""
    problem, l0, u0, ints = _problem_of(bb_or_model, 'conflict_graph')
    l = l0 if l is None else np.asarray(l, dtype=np.float64)
    u = u0 if u is None else np.asarray(u, dtype=np.float64)
    assert l.shape == (problem.n,) and u.shape == (problem.n,), 'l and u hold one box of n columns'
    return problem.conflict_graph(l, u, ints)['adj']


def separate_cliques(bb_or_model, X, adj=None, seeds=None, min_efficacy=DEFAULT_MIN_EFFICACY):
    """Clique cuts of a BranchAndBound's root problem or of a MILPInstance at the points X ((batch, n) or (n,)) inside
    the model's own bounds, one GPU workgroup per point and seed literal (mipx_clique_separate_batch).  adj: a packed
    adjacency (None: conflict_graph of the model is built first); seeds: None for all 2n literals, or the literals to
    grow a clique from.

    Returns (pi, pi0, efficacy, size, status): the cuts pi . x >= pi0 ((batch, R, n) and (batch, R)), their efficacy at
    the point, the size of the clique and a status per seed (0 a cut, 1 no clique, 2 too shallow, 4 skipped).  With
    the graph of the model's own bounds the cuts are valid for the model."""
    problem, l0, u0, ints = _problem_of(bb_or_model, 'separate_cliques')
    n = problem.n
    X = np.asarray(X, dtype=np.float64)
    assert X.ndim in (1, 2) and X.shape[-1] == n, 'X holds one point of n columns per row'
    if adj is None:
        adj = problem.conflict_graph(l0, u0, ints)['adj']
    if seeds is not None:
        seeds = np.asarray(seeds)
        assert seeds.ndim == 1 and len(seeds) >= 1 and np.issubdtype(seeds.dtype, np.integer), \
            'seeds is a list of literals'
    out = problem.clique_separate_batch(X.reshape(-1, n), l0, u0, ints, adj, seeds, min_efficacy)
    return out['pi'], out['pi0'], out['efficacy'], out['size'], out['status']
