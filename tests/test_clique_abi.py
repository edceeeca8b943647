"""The clique cuts (include/mipx_clique.h), the parts that need no GPU: the header against the ctypes table and the
exported symbols, one launch site per kernel, the NumPy restatement (tests/support/clique_reference.py) worked by hand,
the validity of its cuts by exhaustion over every 0/1 point of small conflict models and by HiGHS on rows that mix
column kinds, the order of ties, the instance family, and the root cut loop with the clique option on the
restatements with HiGHS LPs."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest
from scipy.optimize import Bounds, LinearConstraint, linprog, milp

from simple_mip_solver_amd import _ffi
from simple_mip_solver_amd.generators import conflict_packing_milp_arrays, random_dense_milp_arrays
from simple_mip_solver_amd.utils import clique_cuts, mir_cuts
from tests.support import clique_reference as ref
from tests.support import cover_reference, mir_reference
from tests.support.abi_check import agrees, prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'simple_mip_solver_amd', 'csrc')
INF = float('inf')
GRAPH, SEPARATE = 'mipx_clique_graph', 'mipx_clique_separate_batch'


def test_header_and_signature_table_agree():
    protos = prototypes('mipx_clique.h')
    assert sorted(protos) == sorted(_ffi.CLIQUE_SYMBOLS) == [GRAPH, SEPARATE]
    for name, count in ((GRAPH, 7), (SEPARATE, 16)):
        ret, params = protos[name]
        restype, argtypes = _ffi._CLIQUE_SIGNATURES[name]
        assert agrees(ret, restype) and len(params) == len(argtypes) == count
        for k, (decl, ctype) in enumerate(zip(params, argtypes)):
            assert agrees(decl, ctype), f'{name} parameter {k} is `{decl}`, the table says {ctype}'


def test_new_symbols_overlap_no_existing_list():
    old = set()
    for attr in dir(_ffi):
        if attr.endswith('SYMBOLS') and attr != 'CLIQUE_SYMBOLS':
            old |= set(getattr(_ffi, attr))
    assert old and not set(_ffi.CLIQUE_SYMBOLS) & old
    assert not any(name in _ffi._SIGNATURES for name in _ffi.CLIQUE_SYMBOLS)


def test_mipx_h_includes_the_header_behind_cover_and_the_library_exports_its_entries():
    text = open(os.path.join(ROOT, 'include', 'mipx.h')).read()
    assert '#include "mipx_clique.h"' in text
    assert text.index('#include "mipx_cover.h"') < text.index('#include "mipx_clique.h"')
    L = _ffi.lib()
    assert L.mipx_abi_version() == 1
    for name in (GRAPH, SEPARATE):
        assert hasattr(L, name) and getattr(L, name).restype is C.c_int
    assert L.mipx_clique_graph(None, None, None, None, 0, None, None) == -1   # MIPX_EINVAL
    assert L.mipx_clique_separate_batch(None, 1, *([None] * 4), 0, None, None, 0, 1e-6, *([None] * 5)) == -1


def test_status_codes_cover_the_header():
    text = open(os.path.join(ROOT, 'include', 'mipx_clique.h')).read()
    codes = {name: int(v) for name, v in re.findall(r'#define MIPX_CLIQUE_(\w+) (\d+)', text)}
    assert sorted(codes.values()) == sorted(_ffi.CLIQUE_STATUS) == [0, 1, 2, 4]
    assert (codes['CUT'], codes['NO_CLIQUE'], codes['SHALLOW'], codes['SKIPPED']) == \
        (ref.CUT, ref.NO_CLIQUE, ref.SHALLOW, ref.SKIPPED)


def test_one_launch_site_per_kernel_and_one_knapsack_form():
    source = ''.join(open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith(('.hip', '.h')))
    for kernel in ('clique_graph', 'clique_separate', 'cover_separate'):
        assert len(re.findall(r'hipLaunchKernelGGL\(\s*mipx::%s\b' % kernel, source)) == 1, kernel
        assert len(re.findall(r'__global__[^;{]*\b%s\(' % kernel, source)) == 1, kernel
    # the knapsack form is one device function, called by the cover kernel and by the graph kernel
    assert len(re.findall(r'__device__[^;{]*\bcover_knapsack_form\(', source)) == 1
    assert len(re.findall(r'= cover_knapsack_form\(', source)) == 2


# ---- the restatement worked by hand -----------------------------------------------------------------------------------

HAND_A = -np.array([[3.0, 3.0, 0.0, 0.0], [0.0, 3.0, 3.0, 0.0], [3.0, 0.0, 3.0, 0.0], [2.0, 0.0, 0.0, -5.0]])
HAND_B = -np.array([4.0, 4.0, 4.0, -2.0])


def test_the_restatement_worked_by_hand():
    """3 xa + 3 xb <= 4, 3 xb + 3 xc <= 4, 3 xa + 3 xc <= 4 and 2 xa - 5 xd <= -2 on binaries.  The first three rows
    have W = 4 and two items of weight 3: 3 + 3 - 4 = 2 > tau, the edges (0, 2), (2, 4), (0, 4) between the plain
    literals of a, b, c.  In the fourth xd is complemented (literal 7, weight 5) and W = -2 + 5 = 3: 2 + 5 - 3 = 4,
    the edge (0, 7): xa = 1 and xd = 0 cannot be.  Four edges, no other."""
    l, u, ints = np.zeros(4), np.ones(4), range(4)
    adj, status = ref.graph(HAND_A, HAND_B, l, u, ints)
    edges = {(0, 2), (0, 4), (2, 4), (0, 7)}
    assert {(int(k), int(h)) for k, h in np.argwhere(adj)} == edges | {(h, k) for k, h in edges}
    assert status.tolist() == [0, 0, 0, 0]
    assert np.array_equal(ref.unpack(ref.pack(adj), 4), adj) and ref.pack(adj).shape == (8, 1)
    assert ref.pack(adj)[:, 0].tolist() == [0b10010100, 0, 0b00010001, 0, 0b00000101, 0, 0, 0b00000001]
    assert np.array_equal(clique_cuts.unpack_adjacency(ref.pack(adj), 4), adj)
    # at 0.5 everywhere the seed a takes b (ties to the smaller literal), then c: xa + xb + xc <= 1
    r = ref.separate_seed(np.full(4, 0.5), l, u, ints, adj, 0)
    assert r['clique'] == [0, 2, 4] and r['status'] == ref.CUT and r['size'] == 3
    assert np.array_equal(r['pi'], [-1.0, -1.0, -1.0, 0.0]) and r['pi0'] == -1.0
    assert abs(r['efficacy'] - 0.5 / np.sqrt(3.0)) < 1e-15
    # the seed 1 - xd takes a: (1 - xd) + xa <= 1 is xd - xa >= 0 = u_d - 1, tight at 0.5: shallow, yet written
    r = ref.separate_seed(np.full(4, 0.5), l, u, ints, adj, 7)
    assert r['clique'] == [7, 0] and r['status'] == ref.SHALLOW and r['size'] == 2
    assert np.array_equal(r['pi'], [-1.0, 0.0, 0.0, 1.0]) and r['pi0'] == 0.0 and r['efficacy'] == 0.0
    # at (0.6, 0.2, 0.2, 0.3) the seed a prefers 1 - xd (0.7) to b and c (0.2), and no literal joins both
    x = np.array([0.6, 0.2, 0.2, 0.3])
    r = ref.separate_seed(x, l, u, ints, adj, 0)
    assert r['clique'] == [0, 7] and r['status'] == ref.CUT and np.array_equal(r['pi'], [-1.0, 0.0, 0.0, 1.0])
    assert r['pi0'] == 0.0 and abs(r['efficacy'] - 0.3 / np.sqrt(2.0)) < 1e-15
    # the statuses: a literal without neighbours, a seed at value 0, a literal that is not live
    assert ref.separate_seed(x, l, u, ints, adj, 1)['status'] == ref.NO_CLIQUE
    r = ref.separate_seed([0.0, 1.0, 0.0, 1.0], l, u, ints, adj, 0)
    assert r['status'] == ref.NO_CLIQUE and not r['pi'].any() and r['size'] == 0
    assert ref.separate_seed(x, l, u, [1, 2, 3], adj, 0)['status'] == ref.SKIPPED
    # literals at 0 come last and still join: from b at (0, 1, 0, 1) the clique is b, then a before c
    r = ref.separate_seed([0.0, 1.0, 0.0, 1.0], l, u, ints, adj, 2)
    assert r['clique'] == [2, 0, 4] and r['pi0'] == -1.0 and r['efficacy'] == 0.0 and r['status'] == ref.SHALLOW
    # a shifted box: binaries on {2, 3}: the same edges, pi0 = T - 1 = -(l_a + l_b + l_c) - 1
    b3 = HAND_B + HAND_A @ np.full(4, 2.0)
    adj3, _ = ref.graph(HAND_A, b3, l + 2.0, u + 2.0, ints)
    assert np.array_equal(adj3, adj)
    r = ref.separate_seed(np.full(4, 2.5), l + 2.0, u + 2.0, ints, adj3, 0)
    assert r['clique'] == [0, 2, 4] and r['pi0'] == -7.0
    # a general integer or a continuous column is relaxed out; one that needs an infinite bound skips its row only
    A5 = np.hstack([HAND_A, -np.array([[1.0], [0.0], [0.0], [0.0]])])
    u5 = np.append(u, INF)
    adj5, st5 = ref.graph(A5, HAND_B, np.zeros(5), u5, range(5))
    assert st5.tolist() == [0, 0, 0, 0] and np.array_equal(adj5[:8, :8], adj) and not adj5[8:].any()   # (g > 0: relaxed at l)
    adj5, st5 = ref.graph(np.hstack([HAND_A, np.array([[1.0], [0.0], [0.0], [0.0]])]), HAND_B, np.zeros(5), u5, range(5))
    assert st5.tolist() == [4, 0, 0, 0] and {(int(k), int(h)) for k, h in np.argwhere(adj5) if k < h} == {(2, 4), (0, 4), (0, 7)}


def test_the_knapsack_form_is_covers():
    """Skipped rows are the rows the cover restatement skips, on rows of every column kind."""
    rng = np.random.default_rng(3)
    n = 12
    l = np.zeros(n)
    u = np.where(np.arange(n) % 4 == 3, INF, np.where(np.arange(n) % 4 == 2, 3.0, 1.0))
    ints = [j for j in range(n) if j % 4 != 1]
    seen = set()
    for _ in range(200):
        a = rng.integers(-9, 10, n) * (rng.random(n) < 0.5)
        b = float(rng.integers(-20, 5))
        form = ref.knapsack_form(a, b, l, u, ref.binary_columns(l, u, ints))
        cov = cover_reference.separate_row(a, b, np.zeros(n), l, u, ints)
        assert (form is None) == (cov['status'] == cover_reference.SKIPPED)
        seen.add(form is None)
    assert seen == {True, False}


def test_ties_in_value_go_to_the_smaller_literal():
    """The complete graph on the plain literals of 6 binaries: at equal values the clique grows in literal order from
    any seed, and a larger value goes first wherever it stands."""
    n = 6
    adj = np.zeros((2 * n, 2 * n), bool)
    adj[0::2, 0::2] = True
    np.fill_diagonal(adj, False)
    l, u = np.zeros(n), np.ones(n)
    r = ref.separate_seed(np.full(n, 0.5), l, u, range(n), adj, 6)
    assert r['clique'] == [6, 0, 2, 4, 8, 10]
    x = np.array([0.5, 0.25, 0.5, 0.5, 0.75, 0.25])
    assert ref.separate_seed(x, l, u, range(n), adj, 6)['clique'] == [6, 8, 0, 4, 2, 10]
    assert ref.separate_seed(x, l, u, range(n), adj, 10)['clique'] == [10, 8, 0, 4, 6, 2]
    # exact 0s come last, in literal order
    x = np.array([0.0, 0.0, 1.0, 0.0, 0.5, 0.0])
    assert ref.separate_seed(x, l, u, range(n), adj, 4)['clique'] == [4, 8, 0, 2, 6, 10]


# ---- validity by exhaustion ---------------------------------------------------------------------------------------------

POINTS12 = np.array(list(itertools.product((0.0, 1.0), repeat=12)))


def test_exhaustive_validity_on_the_conflict_family():
    """Every cut of every seed (violated or not) at 20 random points of 6 models of 12 columns holds at every feasible
    0/1 point.  Integer data: the check is exact."""
    cuts = complemented = 0
    for seed in range(6):
        A, b, c, l, u, ints = conflict_packing_milp_arrays(12, 20, 3, 6, seed)
        feasible = POINTS12[np.all(POINTS12 @ A.T >= b, axis=1)]
        assert len(feasible) > 1
        adj, status = ref.graph(A, b, l, u, ints)
        assert not status.any() and np.array_equal(adj, adj.T) and not adj.diagonal().any()
        assert not adj[np.arange(24), np.arange(24) ^ 1].any() and adj.sum() // 2 >= 20
        rng = np.random.default_rng(50 + seed)
        X = rng.random((20, 12))
        where = rng.random((20, 12))
        X = np.where(where < 0.2, 0.0, np.where(where < 0.4, 0.5, np.where(where < 0.5, 1.0, X)))
        out = ref.separate(X, l, u, ints, adj)
        for p, k in np.argwhere(np.isin(out['status'], (ref.CUT, ref.SHALLOW))):
            pi, pi0 = out['pi'][p, k], out['pi0'][p, k]
            assert np.all(feasible @ pi >= pi0), (seed, p, k)
            assert int(np.abs(pi).sum()) == out['size'][p, k] >= 2
            cuts += 1
            complemented += bool(np.any(pi > 0))
        none = np.isin(out['status'], (ref.NO_CLIQUE, ref.SKIPPED))
        assert not out['pi'][none].any() and not out['size'][none].any()
    print('cuts checked', cuts, 'with a complemented literal', complemented)
    assert cuts >= 900


def mixed_model(seed):
    """10 binaries, 2 general integers in [0, 4], 2 continuous columns in [0, 2.5]; 8 rows of about 4 non-integer
    weights, a quarter negative, with capacities low enough for conflicts; a node's box that fixes two binaries."""
    rng = np.random.default_rng(300 + seed)
    n, m = 14, 8
    G = rng.integers(1, 30, (m, n)) / 7.0 * np.where(rng.random((m, n)) < 0.25, -1.0, 1.0)
    G *= rng.random((m, n)) < 0.3
    G[:, 10:] *= 0.125
    l = np.zeros(n)
    u = np.concatenate([np.ones(10), np.full(2, 4.0), np.full(2, 2.5)])
    lo = (np.minimum(G, 0.0) * u).sum(1)
    d = lo + rng.uniform(0.5, 1.2, m) * np.abs(G[:, :10]).max(1)
    c = -rng.integers(1, 20, n).astype(np.float64)
    ln, un = l.copy(), u.copy()
    fixed = rng.choice(10, 2, replace=False)
    ln[fixed[0]] = 1.0
    un[fixed[1]] = 0.0
    return -G, -d, c, l, u, ln, un, list(range(12))


def test_cuts_of_mixed_rows_are_valid_by_highs_inside_the_box():
    found = complemented = 0
    for seed in range(8):
        A, b, c, l, u, ln, un, ints = mixed_model(seed)
        integrality = np.zeros(len(c))
        integrality[ints] = 1
        for box_l, box_u in ((l, u), (ln, un)):
            adj, _ = ref.graph(A, b, box_l, box_u, ints)
            live = ref.live_literals(box_l, box_u, ints)
            assert not adj[~live].any() and not adj[:, ~live].any() and np.array_equal(adj, adj.T)
            rng = np.random.default_rng(seed)
            out = ref.separate(box_l + rng.random((3, 14)) * (box_u - box_l), box_l, box_u, ints, adj, min_efficacy=-INF)
            for p in range(3):
                for k in ref.distinct_cuts(out, p):
                    pi, pi0 = out['pi'][p, k], out['pi0'][p, k]
                    assert not pi[10:].any() and not pi[box_l == box_u].any() and pi0 == round(pi0)
                    h = milp(pi, constraints=LinearConstraint(A, lb=b, ub=np.inf), bounds=Bounds(box_l, box_u),
                             integrality=integrality, options=dict(mip_rel_gap=0.0))
                    assert h.status in (0, 2)
                    if h.status == 0:   # (2: the box is infeasible, every cut is valid)
                        assert float(h.fun) >= pi0 - 1e-6 * (abs(pi0) + float(np.abs(pi) @ box_u)), (seed, k, h.fun, pi0)
                    found += 1
                    complemented += bool(np.any(pi > 0))
    print('cuts checked', found, 'with a complemented literal', complemented)
    assert found >= 20 and complemented >= 3


# ---- the instance family and the root loop ----------------------------------------------------------------------------

def test_the_conflict_packing_family():
    A, b, c, l, u, ints = conflict_packing_milp_arrays(16, 36, 3, 6, seed=1)
    assert A.shape == (39, 16) and b.shape == (39,) and c.shape == (16,) and ints == list(range(16))
    assert np.all((A[:36] != 0).sum(1) == 2) and np.all(A[:36][A[:36] != 0] == -1.0) and np.all(b[:36] == -1.0)
    pairs = [tuple(np.flatnonzero(r)) for r in A[:36]]
    assert pairs == sorted(set(pairs))   # (distinct, in lexicographic order)
    assert np.all((A[36:] != 0).sum(1) == 6) and np.all(A[36:][A[36:] != 0] <= -5) and np.all(A >= -30)
    assert np.array_equal(b[36:], -np.floor(0.25 * (-A[36:]).sum(1))) and np.all((c <= -5) & (c >= -30))
    assert np.array_equal(l, np.zeros(16)) and np.array_equal(u, np.ones(16))
    again = conflict_packing_milp_arrays(16, 36, 3, 6, seed=1)
    assert all(np.array_equal(p, q) for p, q in zip((A, b, c), again[:3]))
    rng = np.random.Generator(np.random.PCG64(1))   # (the stream: the pairs, then one knapsack after the other, then c)
    pick = np.sort(rng.choice(120, size=36, replace=False))
    lex = [(i, j) for i in range(16) for j in range(i + 1, 16)]
    assert pairs == [lex[q] for q in pick]
    cols = rng.choice(16, size=6, replace=False)
    assert np.array_equal(-A[36, cols], rng.integers(5, 31, 6))


@pytest.mark.parametrize('shape, edges', [((16, 36, 3, 6), (60, 58, 60)), ((24, 70, 4, 8), (113, 112, 112))])
def test_the_edges_of_the_family(shape, edges):
    for seed, expected in enumerate(edges):
        A, b, c, l, u, ints = conflict_packing_milp_arrays(*shape, seed=seed)
        adj, status = ref.graph(A, b, l, u, ints)
        assert adj.sum() // 2 == expected and not status.any()
        assert not adj[1::2].any()   # (every weight is positive: only plain literals)


def test_the_cuts_at_one_half():
    """At x = 0.5 on 24 x 74: 15 / 16 / 17 distinct cuts of sizes 3 to 7 / 3 to 5 / 3 to 5."""
    for seed, (count, lo, hi) in enumerate([(15, 3, 7), (16, 3, 5), (17, 3, 5)]):
        A, b, c, l, u, ints = conflict_packing_milp_arrays(24, 70, 4, 8, seed=seed)
        adj, _ = ref.graph(A, b, l, u, ints)
        out = ref.separate(np.full((1, 24), 0.5), l, u, ints, adj)
        places = ref.distinct_cuts(out)
        sizes = out['size'][0, places]
        assert (len(places), sizes.min(), sizes.max()) == (count, lo, hi)


def test_general_integer_rows_give_an_empty_graph():
    A, b, c, l, u, ints = random_dense_milp_arrays(20, 10, seed=1)
    adj, status = ref.graph(A, b, l, u, ints)
    assert not adj.any() and not status.any()
    out = ref.separate(np.full((1, 20), 0.5), l, u, ints, adj)
    assert np.all(out['status'] == ref.SKIPPED) and not out['pi'].any()


class HighsRows:
    """One row set for root_cut_loop on the CPU: HiGHS for the LP (no basis: no tableau rows), the restatements for
    the three separations and the graph."""
    graph_calls = []

    def __init__(self, A, b, c):
        self.A, self.b, self.c = A, b, c

    def solve(self, l, u, vstat):
        res = linprog(self.c, A_ub=-self.A, b_ub=-self.b, bounds=list(zip(l, u)), method='highs')
        if res.status != 0:
            return dict(status=1, obj=INF, x=None, y=None, vstat=None, npivots=int(res.nit))
        m, n = self.A.shape
        return dict(status=0, obj=float(res.fun), x=res.x, y=-np.asarray(res.ineqlin.marginals),
                    vstat=np.zeros(n + m, np.int8), npivots=int(res.nit))

    def separate(self, x, l, u, int_idx, row_integral, multipliers, **params):
        out = mir_reference.separate(self.A, self.b, x[None], l[None], u[None], int_idx, row_integral, multipliers, **params)
        return dict(pi=out['pi'][0], pi0=out['pi0'][0], efficacy=out['efficacy'][0], status=out['status'][0])

    def separate_cover(self, x, l, u, int_idx, rows, min_efficacy):
        out = cover_reference.separate(self.A, self.b, x[None], l[None], u[None], int_idx, rows, min_efficacy)
        return dict(pi=out['pi'][0], pi0=out['pi0'][0], efficacy=out['efficacy'][0], status=out['status'][0])


class HighsCliqueRows(HighsRows):
    def conflict_graph(self, l, u, int_idx):
        HighsRows.graph_calls.append(self.A.shape[0])
        adj, status = ref.graph(self.A, self.b, l, u, int_idx)
        return dict(adj=ref.pack(adj), row_status=status)

    def separate_clique(self, x, l, u, int_idx, adj, min_efficacy):
        out = ref.separate(x[None], l, u, int_idx, adj, None, min_efficacy)
        return dict(pi=out['pi'][0], pi0=out['pi0'][0], efficacy=out['efficacy'][0], status=out['status'][0])


STATS = ['rounds', 'base_rows', 'found', 'selected', 'kept', 'bound_before', 'bound_after', 'lp_pivots', 'kernel_us']
COVER_STATS = ['rounds', 'rows', 'found', 'skipped', 'selected', 'kept', 'kernel_us']
CLIQUE_STATS = ['rounds', 'seeds', 'found', 'selected', 'kept', 'edges', 'rows_skipped', 'kernel_us']


def highs_optimum(A, b, c, l, u):
    h = milp(c, constraints=LinearConstraint(A, lb=b, ub=np.inf), bounds=Bounds(l, u), integrality=np.ones(len(c)),
             options=dict(mip_rel_gap=0.0))
    assert h.status == 0
    return float(h.fun)


def loop_checked(shape, seed, edges):
    A, b, c, l, u, ints = conflict_packing_milp_arrays(*shape, seed=seed)
    HighsRows.graph_calls = []
    out = mir_cuts.root_cut_loop(A, b, c, l, u, ints, rounds=10, make_rows=HighsCliqueRows, cover=True, clique=True)
    st, cs, qs = out['stats'], out['cover_stats'], out['clique_stats']
    print(shape, seed, st, cs, qs)
    assert list(out) == ['cuts', 'A', 'b', 'vstat', 'stats', 'cover_stats', 'clique_stats']
    assert list(st) == STATS and list(cs) == COVER_STATS and list(qs) == CLIQUE_STATS
    assert HighsRows.graph_calls == [A.shape[0]]   # (once, from the model's rows alone)
    assert qs['rounds'] == st['rounds'] == cs['rounds'] >= 1 and qs['seeds'] == 2 * shape[0] * qs['rounds']
    assert qs['edges'] == edges and qs['rows_skipped'] == 0
    assert 1 <= qs['kept'] <= qs['selected'] <= qs['found']
    assert st['kept'] + cs['kept'] + qs['kept'] == len(out['cuts'])
    assert st['kept'] <= st['selected'] <= st['found'] and cs['kept'] <= cs['selected'] <= cs['found']
    for pi, pi0 in out['cuts']:
        h = milp(pi, constraints=LinearConstraint(A, lb=b, ub=np.inf), bounds=Bounds(l, u), integrality=np.ones(len(c)),
                 options=dict(mip_rel_gap=0.0))
        assert h.status == 0 and float(h.fun) >= pi0 - 1e-6 * (abs(pi0) + float(np.abs(pi).sum()))
    best = highs_optimum(A, b, c, l, u)
    closed = (st['bound_after'] - st['bound_before']) / (best - st['bound_before'])
    print(shape, seed, 'optimum', best, 'root gap closed', closed)
    return st, best, closed


@pytest.mark.parametrize('seed, edges', [(0, 60), (1, 58), (2, 60)])
def test_the_root_loop_with_cliques_closes_16_by_39(seed, edges):
    st, best, closed = loop_checked((16, 36, 3, 6), seed, edges)
    assert abs(st['bound_after'] - best) <= 1e-6


@pytest.mark.parametrize('seed, edges', [(0, 113), (1, 112), (2, 112)])
def test_the_root_loop_with_cliques_closes_most_of_24_by_74(seed, edges):
    """Measured with the CPU prototype: 1.00, 0.84 and 0.92 of the root gap closed; at most 0.62 without cliques."""
    st, best, closed = loop_checked((24, 70, 4, 8), seed, edges)
    assert closed >= 0.8
    A, b, c, l, u, ints = conflict_packing_milp_arrays(24, 70, 4, 8, seed=seed)
    off = mir_cuts.root_cut_loop(A, b, c, l, u, ints, rounds=10, make_rows=HighsRows, cover=True)
    without = (off['stats']['bound_after'] - off['stats']['bound_before']) / (best - off['stats']['bound_before'])
    print(seed, 'without cliques', without)
    assert without <= 0.62 + 1e-9 < closed


def test_with_the_option_off_the_return_value_is_as_before():
    """A row-set object without the two new methods still works, and the keys are those of before."""
    A, b, c, l, u, ints = conflict_packing_milp_arrays(16, 36, 3, 6, seed=0)
    off = mir_cuts.root_cut_loop(A, b, c, l, u, ints, rounds=3, make_rows=HighsRows)
    assert list(off) == ['cuts', 'A', 'b', 'vstat', 'stats'] and list(off['stats']) == STATS
    cov = mir_cuts.root_cut_loop(A, b, c, l, u, ints, rounds=3, make_rows=HighsRows, cover=True, clique=False)
    assert list(cov) == ['cuts', 'A', 'b', 'vstat', 'stats', 'cover_stats'] and list(cov['cover_stats']) == COVER_STATS
    only = mir_cuts.root_cut_loop(A, b, c, l, u, ints, rounds=3, make_rows=HighsCliqueRows, clique=True)
    assert list(only) == ['cuts', 'A', 'b', 'vstat', 'stats', 'clique_stats']
    assert only['stats']['kept'] + only['clique_stats']['kept'] == len(only['cuts'])
