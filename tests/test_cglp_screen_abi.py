"""The dual screen of the support sessions and the in-out separator, the parts that need no GPU
(include/mipx_cglp_screen.h): the NumPy restatement of the bound worked by hand and against rational arithmetic, weak
duality against HiGHS, the in-out logic of DisjunctiveSeparator on a session whose leaf LPs are HiGHS, and the
signatures and refusals of the new entries."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from simple_mip_solver_amd import DisjunctiveSeparator, _ffi
from simple_mip_solver_amd.generators import random_dense_milp_arrays
from simple_mip_solver_amd.lp import CyLPArray
from tests.support import cglp_reference as highs
from tests.support import cglp_screen_reference as ref
from tests.support.abi_check import agrees, library_prerequisites, prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['mipx_tree_support_open_ex', 'mipx_tree_support_eval_ex', 'mipx_support_screen_batch']
HIGHS_TOL = 1e-7


# ---- the restatement ---------------------------------------------------------------------------------------------
def test_bound_worked_by_hand():
    A, b, pi = np.array([[1.0, 2.0], [3.0, 1.0]]), np.array([2.0, 3.0]), np.array([1.0, 1.0])
    l = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 0.0]])
    u = np.array([[4.0, 4.0], [2.0, 3.0], [4.0, 4.0]])
    y = np.array([[0.5, -1.0], [0.25, 0.5], [9.0, 9.0]])
    has_y = np.array([1, 1, 0], np.uint8)
    # leaf 0: y+ = (0.5, 0), A'y+ = (0.5, 1), r = (0.5, 0): terms min(0, 2) and 0, y+.b = 1                -> L = 1
    # leaf 1: A'y+ = (0.25 + 1.5, 0.5 + 0.5), r = (-0.75, 0): terms min(-0.75, -1.5) and 0, y+.b = 0.5 + 1.5 -> L = 0.5
    #         (its h is 1.5: x1 = 1 forces x2 >= 0.5)
    # leaf 2: no duals on record
    assert ref.bound(A, b, pi, l, u, y, has_y).tolist() == [1.0, 0.5, -np.inf]
    assert highs.support(pi, A, b, l[1], u[1]) == (0, 1.5)
    out = ref.screen(A, b, pi, 0.75, 0.0, l, u, y, has_y)
    assert out['screened'].tolist() == [1, 0, 0] and out['packed'].tolist() == [1, 2, -1] and out['count'] == 2
    # the margin of leaf 1 is -0.25: it screens at that tolerance and not an ulp below
    assert ref.screen(A, b, pi, 0.75, 0.25, l, u, y, has_y)['screened'].tolist() == [1, 1, 0]
    assert ref.screen(A, b, pi, 0.75, np.nextafter(0.25, 0), l, u, y, has_y)['screened'].tolist() == [1, 0, 0]
    # a bound that is not finite never screens
    y[0, 0] = np.inf
    assert ref.screen(A, b, pi, -np.inf, 0.0, l, u, y, has_y)['screened'].tolist() == [0, 1, 0]


def test_fma_of_the_restatement_is_exact():
    rng = np.random.default_rng(1)
    N = 4000
    a, b, c = (rng.standard_normal(N) * 10.0 ** rng.integers(-5, 5, N) for _ in range(3))
    c[:1000] = -(a[:1000] * b[:1000])                        # the sum is the product's rounding error
    c[1000:1500] = -(a[1000:1500] * b[1000:1500]) * (1 + 2.0 ** -52)
    c[1500:1600], a[1600:1700] = 0.0, 0.0
    want = np.array([float(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(a, b, c)])
    assert np.array_equal(ref.fma(a, b, c).view(np.int64), want.view(np.int64))
    assert np.any(ref.fma(a, b, c) != a * b + c)            # (the cases tell a fused from an unfused product)


def test_sum_order_is_lanes_then_butterfly():
    # 130 terms: lane 0 adds terms 0, 64, 128, lane 1 adds 1, 65, 129; with 1e16 in lane 0 the order shows
    terms = np.ones((1, 130))
    terms[0, 0], terms[0, 64], terms[0, 128] = 1e16, 1.0, 1.0
    lanes = ref._lane_sums(terms)
    assert lanes[0, 0] == (1e16 + 1.0) + 1.0 == 1e16 and lanes[0, 1] == 3.0 and lanes[0, 2] == 2.0
    v = lanes.copy()
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[:, np.arange(64) ^ off]
    assert np.all(v == v[0, 0]) and ref._butterfly(lanes)[0] == v[0, 0]


@pytest.mark.parametrize('n, m, seed', [(10, 5, 0), (40, 20, 3)])
def test_weak_duality_against_highs(n, m, seed):
    A, b, _, l, u, _ = random_dense_milp_arrays(n, m, seed=seed)
    rng = np.random.default_rng(seed)
    done = 0
    for _ in range(200):
        if done == 20:
            break
        lo, up = l.copy(), u.copy()   # a sub-box as a search makes them: a few columns cut on one side
        for j in rng.choice(n, 3, replace=False):
            cut = l[j] + rng.uniform(0.2, 0.8) * (u[j] - l[j])
            if rng.random() < 0.5:
                lo[j] = cut
            else:
                up[j] = cut
        pi = rng.uniform(-1, 1, n)
        status, h, _, y_star = ref.support_with_duals(pi, A, b, lo, up)
        if status != 0:
            continue
        done += 1
        slack = 1e-9 * max(1.0, abs(h))
        for _ in range(5):   # any y >= 0 bounds from below (negative entries read as 0)
            y = rng.uniform(-0.5, 2.0, m) * (rng.random(m) < 0.5)
            assert ref.bound(A, b, pi, lo, up, y)[0] <= h + slack
        assert np.all(y_star >= -1e-12)
        L = ref.bound(A, b, pi, lo, up, y_star)[0]
        assert L <= h + slack and abs(L - h) <= HIGHS_TOL * max(1.0, abs(h)), (L, h)
    assert done == 20


# ---- in-out and screening on a session without a GPU ------------------------------------------------------------------
class HighsSeparator(DisjunctiveSeparator):
    _solve_master = ref.highs_master


_tree = {}


def small_tree():
    if not _tree:
        A, b, c, l, u, ints = random_dense_milp_arrays(20, 10, seed=3)
        x_root, L, U = ref.highs_tree(A, b, c, l, u, np.asarray(ints), 50)
        _tree.update(A=A, b=b, l=l, u=u, x=x_root, L=L, U=U)
    return _tree


def run(**options):
    t = small_tree()
    ses = ref.HighsSession(t['A'], t['b'], t['L'], t['U'])
    sep = HighsSeparator.on_session(ses, t['l'], t['u'], tol=1e-7, **options)
    pi, pi0 = sep.solve(CyLPArray(t['x']))
    return sep, pi, pi0


def plain():
    if 'plain' not in _tree:
        _tree['plain'] = run()
    return _tree['plain']


def test_fake_session_tree_is_a_disjunction_of_about_50_leaves():
    t = small_tree()
    assert 40 <= len(t['L']) <= 60
    sep, pi, pi0 = plain()
    assert sep.stats['converged'] and pi is not None
    assert 'screened' not in sep.stats and sep.stats['leaf_lps'] == sep.stats['rounds'] * len(t['L'])
    for k in range(len(t['L'])):   # the cut holds on every leaf
        status, h = highs.support(np.asarray(pi), t['A'], t['b'], t['L'][k], t['U'][k])
        assert status == 0 and h - pi0 >= -2e-7 * max(1.0, abs(pi0), float(np.abs(pi).sum()))


@pytest.mark.parametrize('options', [dict(stabilisation=0.5), dict(screen=True), dict(screen=True, stabilisation=0.5),
                                     dict(stabilisation=1.0)])
def test_options_converge_to_the_plain_violation(options):
    base, _, _ = plain()
    sep, pi, pi0 = run(**options)
    scale = max(1.0, abs(pi0), float(np.abs(np.asarray(pi)).sum()))
    print(options, 'stats', sep.stats, 'plain', base.stats)
    assert sep.stats['converged']
    assert abs(sep.stats['violation'] - base.stats['violation']) <= 2 * sep.tol * scale + HIGHS_TOL
    t = small_tree()
    for k in range(len(t['L'])):
        status, h = highs.support(np.asarray(pi), t['A'], t['b'], t['L'][k], t['U'][k])
        assert status == 0 and h - pi0 >= -HIGHS_TOL * scale
    if options.get('screen'):
        assert sep.stats['screened'] > 0 and sep.stats['leaf_lps'] < base.stats['leaf_lps']
        assert sep.stats['screened'] + sep.stats['leaf_lps'] == sep.stats['rounds'] * len(t['L'])
    if options.get('stabilisation') == 1.0:   # the master's point every round: the plain run
        assert sep.stats['rounds'] == base.stats['rounds'] and sep.stats['violation'] == base.stats['violation']
    if 'stabilisation' in options:
        assert sep.stats['in_moves'] >= 1


def test_defaults_pass_no_new_keyword_to_the_session():
    t = small_tree()

    class Strict(ref.HighsSession):
        def eval(self, pi, pi0, tol=0.0, max_points=1):   # (the signature of a session before the options)
            return ref.HighsSession.eval(self, pi, pi0, tol=tol, max_points=max_points)

    sep = HighsSeparator.on_session(Strict(t['A'], t['b'], t['L'], t['U']), t['l'], t['u'])
    sep.solve(CyLPArray(t['x']))
    base, _, _ = plain()
    assert sep.stats == base.stats


@pytest.mark.parametrize('kw', [dict(stabilisation=0.0), dict(stabilisation=1.5), dict(stabilisation='0.5'), dict(screen=1),
                                dict(retry_cold='yes')])
def test_refuses_bad_options(kw):
    t = small_tree()
    with pytest.raises(AssertionError):
        HighsSeparator.on_session(ref.HighsSession(t['A'], t['b'], t['L'], t['U']), t['l'], t['u'], **kw)


# ---- signatures and refusals -------------------------------------------------------------------------------------
def test_header_and_signature_table_agree():
    protos = prototypes('mipx_cglp_screen.h')
    assert sorted(protos) == sorted(_ffi.CGLP_SCREEN_SYMBOLS) == sorted(NAMES)
    for name, (ret, params) in protos.items():
        restype, argtypes = _ffi._CGLP_SCREEN_SIGNATURES[name]
        assert agrees(ret, restype), name
        assert len(params) == len(argtypes), name
        for k, (decl, ctype) in enumerate(zip(params, argtypes)):
            assert agrees(decl, ctype), f'{name} parameter {k} is `{decl}`, the table says {ctype}'


def test_new_symbols_overlap_no_existing_list():
    old = set()
    for attr in dir(_ffi):
        if attr.endswith('SYMBOLS') and attr != 'CGLP_SCREEN_SYMBOLS':
            old |= set(getattr(_ffi, attr))
    assert old and not set(_ffi.CGLP_SCREEN_SYMBOLS) & old


def test_mipx_h_includes_the_header_and_the_constants_match():
    assert '#include "mipx_cglp_screen.h"' in open(os.path.join(ROOT, 'include', 'mipx.h')).read()
    head = open(os.path.join(ROOT, 'include', 'mipx_cglp_screen.h')).read()
    assert 'TEST SCAFFOLDING' in head
    assert int(re.search(r'#define MIPX_SUPPORT_KEEP_DUALS (\d+)', head).group(1)) == _ffi.SUPPORT_KEEP_DUALS
    assert 'mipx_cglp_screen.h' in open(os.path.join(ROOT, 'include', 'mipx_cglp.h')).read()
    kernels = open(os.path.join(ROOT, 'simple_mip_solver_amd', 'csrc', 'cglp_screen_kernels.hip.h')).read()
    assert int(re.search(r'kScrMax = (\d+)', kernels).group(1)) == 1024 and 'above 1024' in head
    assert os.path.join(ROOT, 'include', 'mipx_cglp_screen.h') in library_prerequisites()   # (a change of the header rebuilds the library)
    assert len(_ffi.CGLP_EXTRA_KEYS) == 6 and 'extra (null, or 6 doubles)' in head


def test_library_exports_the_entries():
    L = _ffi.lib()
    for name in _ffi.CGLP_SCREEN_SYMBOLS:
        assert hasattr(L, name), name
        assert getattr(L, name).restype is _ffi._CGLP_SCREEN_SIGNATURES[name][0]


def test_c_entries_refuse_null_arguments():
    L = _ffi.lib()
    assert L.mipx_tree_support_open_ex(None, None, 0, 1, None) == -1      # MIPX_EINVAL
    assert L.mipx_tree_support_eval_ex(None, None, 0.0, 0.0, 0.0, 1, 1, None, None, None) == -1
    assert L.mipx_support_screen_batch(None, 1, None, 0.0, 0.0, *([None] * 8)) == -1


def test_no_product_code_calls_the_scaffolding():
    pkg = os.path.join(ROOT, 'simple_mip_solver_amd')
    for base, _, files in os.walk(pkg):
        for f in files:
            if f.endswith('.py') and f != '_ffi.py':
                assert 'support_screen_batch' not in open(os.path.join(base, f)).read(), f


def test_the_lp_kernels_are_not_touched_by_the_screen():
    """The packed launch is launch_lp_any over the launch buffers; the screen's kernels live in their own file."""
    csrc = os.path.join(ROOT, 'simple_mip_solver_amd', 'csrc')
    api = open(os.path.join(csrc, 'cglp_api.hip.h')).read()
    assert api.count('launch_lp_any(') == 2     # every leaf; the packed leaves
    for f in os.listdir(csrc):
        if f.startswith('lp_kernel'):
            assert 'support_' not in open(os.path.join(csrc, f)).read(), f
