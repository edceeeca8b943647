"""Mixed-integer rounding cuts (include/mipx_mir.h): stand-alone separation on the GPU for users of lp_batch or of a
loop of their own, the tableau rows of a basis as base rows, and the root cut loop behind
BranchAndBound(root_cuts=...), which with cover=True also takes the lifted cover cuts of include/mipx_cover.h and with
clique=True the clique cuts of include/mipx_clique.h."""
from math import cos, radians

import numpy as np

from simple_mip_solver_amd.milp_instance import MILPInstance
from simple_mip_solver_amd.utils import tolerance as tol

DEFAULT_ROOT_CUT_ROUNDS = 10
DEFAULT_ROOT_CUT_ROWS = 64
MAX_ROWS = 1024   # rows of a model the separation takes (m + cut rows)


def row_integral_flags(A, b, int_idx):
    """One flag per row of A x >= b: its slack A_i x - b_i is an integer at every point with integer int_idx columns
    (b_i and every a_ij integers, a_ij = 0 on the continuous columns)."""
    A, b = np.asarray(A, np.float64), np.asarray(b, np.float64)
    cont = np.ones(A.shape[1], bool)
    cont[np.asarray(int_idx, dtype=np.int64)] = False
    whole = np.all(np.floor(A) == A, axis=1) & (np.floor(b) == b)
    return (whole & ~np.any(A[:, cont] != 0.0, axis=1)).astype(np.uint8)


def separate_mir(bb_or_model, X, L=None, U=None, multipliers=None, **params):
    """MIR cuts of a BranchAndBound's root problem or of a MILPInstance at the points X ((batch, n) or (n,)) inside
    the boxes L <= x <= U (None: the model's own bounds), one GPU workgroup per point and base row
    (mipx_mir_separate_batch).  multipliers: None for the model's m rows, or an (R, m) matrix whose rows aggregate them
    (tableau_multipliers).  params: max_divisors, f0_min, min_efficacy, max_dynamism.

    Returns (pi, pi0, efficacy, delta, sign, status): the cuts pi . x >= pi0 ((batch, R, n) and (batch, R)), their
    efficacy at the point, the divisor and sign that won, and a status per row (0 a cut, 1 no admissible trial,
    2 too shallow, 3 too wide a range of coefficients, 4 skipped).  With the model's own bounds the cuts are valid
    for the model, with a node's box for that node."""
    from simple_mip_solver_amd.lp import get_backend, HipBackend
    if isinstance(bb_or_model, MILPInstance):
        lp, ints = bb_or_model.lp, bb_or_model.integerIndices
    else:
        assert hasattr(bb_or_model, 'root_node') and hasattr(bb_or_model, 'model'), \
            'separate_mir takes a BranchAndBound or a MILPInstance'
        lp, ints = bb_or_model.root_node.lp, bb_or_model.model.integerIndices
    backend = get_backend()
    assert isinstance(backend, HipBackend), 'separate_mir needs the HIP backend'
    unknown = set(params) - {'max_divisors', 'f0_min', 'min_efficacy', 'max_dynamism'}
    assert not unknown, f'separate_mir parameters are max_divisors, f0_min, min_efficacy and max_dynamism, not {sorted(unknown)}'
    rs = lp._engine_form()
    m, n = rs.A.shape
    X = np.asarray(X, dtype=np.float64)
    assert X.ndim in (1, 2) and X.shape[-1] == n, 'X holds one point of n columns per row'
    l0, u0 = lp._bounds()
    L = np.broadcast_to(l0, X.shape) if L is None else np.asarray(L, dtype=np.float64)
    U = np.broadcast_to(u0, X.shape) if U is None else np.asarray(U, dtype=np.float64)
    assert L.shape == X.shape and U.shape == X.shape, 'L and U hold one box per point'
    if multipliers is not None:
        multipliers = np.asarray(multipliers, dtype=np.float64)
        assert multipliers.ndim == 2 and multipliers.shape[1] == m and multipliers.shape[0] >= 1, \
            'multipliers is an (R, m) matrix, one base row per row'
    ints = sorted(set(int(j) for j in ints))
    problem = backend._problem(rs.A, rs.b, rs.c, rs.key)
    out = problem.mir_separate_batch(X.reshape(-1, n), L.reshape(-1, n), U.reshape(-1, n), ints,
                                     row_integral_flags(rs.A, rs.b, ints), multipliers, **params)
    return out['pi'], out['pi0'], out['efficacy'], out['delta'], out['sign'], out['status']


def tableau_multipliers(problem_arrays, vstat, x, int_idx, max_rows=64):
    """The rows of B^-1 for the basic integer columns that are fractional at x by more than variable_epsilon, the most
    fractional first, at most max_rows: a (T, m) matrix of multipliers over the rows A x >= b of problem_arrays = (A, b).
    The basis is the one `vstat` names (n + m codes as solve_batch returns them, 1 = basic) over the columns of
    [A, -I]; one LU factorisation.  No rows where the basis does not have m columns or is singular."""
    A = np.asarray(problem_arrays[0], np.float64)
    m, n = A.shape
    vstat = np.asarray(vstat).reshape(-1)
    assert len(vstat) == n + m, 'vstat holds n + m codes'
    basic = np.flatnonzero(vstat == 1)
    none = np.zeros((0, m))
    if len(basic) != m or m == 0:
        return none
    x = np.asarray(x, np.float64)
    frac = np.abs(x - np.round(x))
    ints = set(int(j) for j in int_idx)
    pos = [p for p, j in enumerate(basic) if j < n and int(j) in ints and frac[j] > tol.variable_epsilon]
    if not pos:
        return none
    pos.sort(key=lambda p: -frac[basic[p]])   # (stable: ties in column order)
    pos = pos[:max_rows]
    B = np.zeros((m, m))
    for p, j in enumerate(basic):
        if j < n:
            B[:, p] = A[:, j]
        else:
            B[j - n, p] = -1.0
    E = np.zeros((m, len(pos)))
    E[pos, np.arange(len(pos))] = 1.0
    try:
        lam = np.linalg.solve(B.T, E).T   # row p of B^-1 is the solution of B' y = e_p
    except np.linalg.LinAlgError:
        return none
    return np.ascontiguousarray(lam[np.all(np.isfinite(lam), axis=1)])


class GpuRows:
    """One row set on the GPU for root_cut_loop: its LP and its separation."""

    def __init__(self, A, b, c):
        from simple_mip_solver_amd import _ffi
        from simple_mip_solver_amd.lp import get_backend, HipBackend
        backend = get_backend()
        assert isinstance(backend, HipBackend), 'the root cut loop needs the HIP backend'
        self.problem = _ffi.Problem(backend._context(), A, b, c)

    def solve(self, l, u, vstat):
        r = self.problem.solve_batch(l[None], u[None], None if vstat is None else vstat[None])
        return dict(status=int(r['status'][0]), obj=float(r['obj'][0]), x=r['x'][0], y=r['y'][0], vstat=r['vstat'][0],
                    npivots=int(r['npivots'][0]))

    def separate(self, x, l, u, int_idx, row_integral, multipliers, **params):
        r = self.problem.mir_separate_batch(x[None], l[None], u[None], int_idx, row_integral, multipliers, **params)
        return dict(pi=r['pi'][0], pi0=r['pi0'][0], efficacy=r['efficacy'][0], status=r['status'][0],
                    kernel_us=r['kernel_us'])

    def separate_cover(self, x, l, u, int_idx, rows, min_efficacy):
        r = self.problem.cover_separate_batch(x[None], l[None], u[None], int_idx, rows, min_efficacy)
        return dict(pi=r['pi'][0], pi0=r['pi0'][0], efficacy=r['efficacy'][0], status=r['status'][0],
                    kernel_us=r['kernel_us'])

    def conflict_graph(self, l, u, int_idx):
        r = self.problem.conflict_graph(l, u, int_idx)
        return dict(adj=r['adj'], row_status=r['row_status'], kernel_us=r['kernel_us'])

    def separate_clique(self, x, l, u, int_idx, adj, min_efficacy):
        r = self.problem.clique_separate_batch(x[None], l, u, int_idx, adj, None, min_efficacy)
        return dict(pi=r['pi'][0], pi0=r['pi0'][0], efficacy=r['efficacy'][0], status=r['status'][0],
                    kernel_us=r['kernel_us'])

    def close(self):
        self.problem.close()


def select_cuts(pi, pi0, efficacy, status, taken, room, max_cuts, cos_parallel):
    """Greedy selection in order of efficacy (ties: the earlier row): a status-0 cut is refused when the cosine of its
    angle with a cut of `taken` or one selected before it is above cos_parallel.  At most min(max_cuts, room)."""
    order = [k for k in np.argsort(-efficacy, kind='stable') if status[k] == 0]
    dirs = [p / np.linalg.norm(p) for p, _ in taken]
    chosen = []
    for k in order:
        if len(chosen) >= min(max_cuts, room):
            break
        d = pi[k] / np.linalg.norm(pi[k])
        if any(float(d @ e) > cos_parallel for e in dirs):
            continue
        dirs.append(d)
        chosen.append((pi[k].copy(), float(pi0[k])))
    return chosen


def _chosen_places(sep, chosen):
    """The candidate row each chosen cut was copied from: the first status-0 row with its coefficients (select_cuts
    refuses a second copy as parallel)."""
    places = []
    for pi, pi0 in chosen:
        places.append(next(k for k in range(len(sep['status'])) if sep['status'][k] == 0 and sep['pi0'][k] == pi0
                           and np.array_equal(sep['pi'][k], pi)))
    return places


def root_cut_loop(A, b, c, l, u, int_idx, rounds=DEFAULT_ROOT_CUT_ROUNDS, max_rows=DEFAULT_ROOT_CUT_ROWS,
                  max_cuts_per_round=16, max_tableau_rows=64, parallel_cut_tolerance=tol.parallel_cut_tolerance,
                  cutting_plane_progress_tolerance=tol.cutting_plane_progress_tolerance, make_rows=GpuRows, cover=False,
                  cover_min_efficacy=1e-6, clique=False, clique_min_efficacy=1e-6, **params):
    """Rounds of MIR separation at the root of min c x, A x >= b, l <= x <= u with the integer columns int_idx.

    Every round solves the LP over the model's rows and the cut rows alive (warm from the last basis, new rows basic),
    drops the cut rows that are slack with a zero dual at the new point, stops when the LP is not optimal, its point
    is integral or the bound gained less than cutting_plane_progress_tolerance (relative), separates the unit rows of
    the model's m rows and the tableau rows of the fractional basic integer columns, and takes at most
    max_cuts_per_round cuts in order of efficacy, none within parallel_cut_tolerance degrees of one alive or taken.  At
    most max_rows cut rows are alive, and m + rows <= 1024.  make_rows(A, b, c) gives the object that solves and
    separates one row set (GpuRows; tests put a CPU restatement there); params go to the separation.

    cover=True: every round also separates lifted cover cuts (include/mipx_cover.h) from the model's m rows, not from
    the cut rows, in a second launch.  Their candidates stand behind the MIR candidates in the selection, so a tie in
    efficacy goes to the MIR row.

    clique=True: the conflict graph of include/mipx_clique.h is built once, from the first row set (the model's rows
    alone) and the box l, u, and every round also grows a clique from each of the 2n literals at the round's point, in
    a launch behind the other two.  The status-0 cuts are reduced to the distinct (pi, pi0), the first seed's kept, and
    stand behind the MIR and the cover candidates in the selection.

    Returns dict(cuts=[(pi, pi0)], A, b (the model's rows and the cuts), vstat (the last basis or None), stats), and
    with cover=True also cover_stats (rounds, rows, found, skipped, selected, kept, kernel_us), with clique=True also
    clique_stats (rounds, seeds, found (distinct), selected, kept, edges, rows_skipped, kernel_us (the graph and the
    separations)); `selected` and `kept` of stats then count the MIR cuts alone, so the cuts returned are
    stats['kept'] + cover_stats['kept'] + clique_stats['kept']."""
    A, b, c = np.asarray(A, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64)
    l, u = np.asarray(l, np.float64), np.asarray(u, np.float64)
    m0, n = A.shape
    assert np.all(np.isfinite(l)), 'the root cut loop needs finite lower bounds'
    ints = sorted(set(int(j) for j in int_idx))
    max_rows = min(int(max_rows), MAX_ROWS - m0)
    flags0 = row_integral_flags(A, b, ints)
    cos_par = cos(radians(parallel_cut_tolerance))
    cuts, vstat, prev = [], None, None
    stats = dict(rounds=0, base_rows=0, found=0, selected=0, kept=0, bound_before=None, bound_after=None, lp_pivots=0,
                 kernel_us=0.0)
    cover_stats = dict(rounds=0, rows=0, found=0, skipped=0, selected=0, kept=0, kernel_us=0.0) if cover else None
    clique_stats = dict(rounds=0, seeds=0, found=0, selected=0, kept=0, edges=0, rows_skipped=0, kernel_us=0.0) if clique else None
    adj = None        # the packed conflict graph, built before the first clique separation
    kind = []         # one code per cut alive: 0 a MIR cut, 1 from the cover separation, 2 from the clique separation

    def rows_of(cuts):
        if not cuts:
            return A, b
        return np.vstack([A] + [p[None] for p, _ in cuts]), np.concatenate([b, [p0 for _, p0 in cuts]])

    made = []

    def make(Ak, bk):
        made.append(make_rows(Ak, bk, c))
        return made[-1]

    for rnd in range(int(rounds) + 1):
        Ak, bk = rows_of(cuts)
        rows = make(Ak, bk)
        res = rows.solve(l, u, vstat)
        stats['lp_pivots'] += res['npivots']
        if res['status'] != 0:
            vstat = None
            break
        x, y, vstat = res['x'], res['y'], np.array(res['vstat'], dtype=np.int8)
        if stats['bound_before'] is None:
            stats['bound_before'] = res['obj']
        stats['bound_after'] = res['obj']
        # cut rows that are slack with a zero dual leave: their slacks are basic, the point and the basis stay optimal
        if cuts:
            keep = [k for k, (p, p0) in enumerate(cuts)
                    if not (float(p @ x) - p0 > 1e-9 * (abs(p0) + float(np.abs(p) @ np.abs(x))) and abs(y[m0 + k]) <= 1e-12
                            and vstat[n + m0 + k] == 1)]
            if len(keep) < len(cuts):
                cuts = [cuts[k] for k in keep]
                kind = [kind[k] for k in keep]
                vstat = np.concatenate([vstat[:n + m0], vstat[n + m0:][keep]])
                Ak, bk = rows_of(cuts)
                rows = None
        if np.all(np.abs(x[ints] - np.round(x[ints])) <= tol.variable_epsilon):
            break
        if prev is not None and res['obj'] - prev < cutting_plane_progress_tolerance * (abs(prev) if prev != 0 else 1.0):
            break
        prev = res['obj']
        room = max_rows - len(cuts)
        if rnd == int(rounds) or room <= 0:
            break
        if rows is None:
            rows = make(Ak, bk)
        mk = Ak.shape[0]
        T = tableau_multipliers((Ak, bk), vstat, x, ints, max_rows=max_tableau_rows)
        M = np.zeros((m0 + len(T), mk))
        M[np.arange(m0), np.arange(m0)] = 1.0
        M[m0:] = T
        flags = np.concatenate([flags0, np.zeros(mk - m0, np.uint8)])
        sep = rows.separate(x, l, u, ints, flags, M, **params)
        stats['rounds'] += 1
        stats['base_rows'] += len(M)
        stats['found'] += int(np.sum(sep['status'] == 0))
        stats['kernel_us'] += sep.get('kernel_us', 0.0)
        n_mir = len(sep['status'])
        if cover:
            cov = rows.separate_cover(x, l, u, ints, None if mk == m0 else np.arange(m0, dtype=np.int32), cover_min_efficacy)
            cover_stats['rounds'] += 1
            cover_stats['rows'] += m0
            cover_stats['found'] += int(np.sum(cov['status'] == 0))
            cover_stats['skipped'] += int(np.sum(cov['status'] == 4))
            cover_stats['kernel_us'] += cov.get('kernel_us', 0.0)
            sep = {key: np.concatenate([sep[key], cov[key]]) for key in ('pi', 'pi0', 'efficacy', 'status')}
        n_cover = len(sep['status'])
        if clique:
            if adj is None:
                g = made[0].conflict_graph(l, u, ints)
                adj = g['adj']
                clique_stats['edges'] = int(np.unpackbits(np.ascontiguousarray(adj).view(np.uint8)).sum()) // 2
                clique_stats['rows_skipped'] = int(np.sum(g['row_status'] == 4))
                clique_stats['kernel_us'] += g.get('kernel_us', 0.0)
            clq = rows.separate_clique(x, l, u, ints, adj, clique_min_efficacy)
            seen, places = set(), []   # the distinct (pi, pi0) of the status-0 seeds, the first seed's kept
            for k in np.flatnonzero(clq['status'] == 0):
                cut = (clq['pi'][k].tobytes(), float(clq['pi0'][k]))
                if cut not in seen:
                    seen.add(cut)
                    places.append(k)
            clique_stats['rounds'] += 1
            clique_stats['seeds'] += len(clq['status'])
            clique_stats['found'] += len(places)
            clique_stats['kernel_us'] += clq.get('kernel_us', 0.0)
            places = np.asarray(places, dtype=np.int64)
            sep = {key: np.concatenate([sep[key], clq[key][places]]) for key in ('pi', 'pi0', 'efficacy', 'status')}
        chosen = select_cuts(sep['pi'], sep['pi0'], sep['efficacy'], sep['status'], cuts, room, max_cuts_per_round, cos_par)
        if not chosen:
            break
        # which kind each chosen cut is: select_cuts copies the rows, so they are found again by their place
        codes = [0 if k < n_mir else 1 if k < n_cover else 2 for k in _chosen_places(sep, chosen)] if cover or clique \
            else [0] * len(chosen)
        stats['selected'] += codes.count(0)
        if cover:
            cover_stats['selected'] += codes.count(1)
        if clique:
            clique_stats['selected'] += codes.count(2)
        kind = kind + codes
        cuts = cuts + chosen
        vstat = np.concatenate([vstat, np.ones(len(chosen), np.int8)])
    for rows in made:   # (the row sets of the rounds: their device buffers go now)
        if hasattr(rows, 'close'):
            rows.close()
    stats['kept'] = kind.count(0)
    if cover:
        cover_stats['kept'] = kind.count(1)
    if clique:
        clique_stats['kept'] = kind.count(2)
    Ak, bk = rows_of(cuts)
    if vstat is not None and len(vstat) != n + Ak.shape[0]:
        vstat = None
    out = dict(cuts=cuts, A=np.ascontiguousarray(Ak), b=np.ascontiguousarray(bk), vstat=vstat, stats=stats)
    if cover:
        out['cover_stats'] = cover_stats
    if clique:
        out['clique_stats'] = clique_stats
    return out
