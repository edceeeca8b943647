"""The kernels behind a support evaluation on a caller's leaves (include/mipx_supportkernels.h), the parts that need no
GPU: the header against the ctypes table and the exported symbols, the one launch site of each of the eight kernels,
and the reference the kernels are compared with (tests/support/support_kernels_reference.py): the selection against
np.lexsort, the pack against np.flatnonzero, the chained evaluation against its own bookkeeping, and that the generated
cases hold the edges their names say."""
import os
import re

import numpy as np
import pytest

from simple_mip_solver_amd import _ffi
from tests.support import support_kernels_reference as ref
from tests.support.abi_check import agrees, library_prerequisites, prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'simple_mip_solver_amd', 'csrc')
NAMES = ['mipx_support_select_batch', 'mipx_support_pack_batch', 'mipx_support_gather_batch', 'mipx_support_scatter_batch',
         'mipx_support_mark_batch']
KERNELS = ['support_screen', 'support_pack_count', 'support_pack', 'support_gather', 'support_scatter', 'support_mark',
           'support_select', 'support_select_merge']
SEG = ref.SEG


def test_header_and_signature_table_agree():
    protos = prototypes('mipx_supportkernels.h')
    assert sorted(protos) == sorted(_ffi.SUPPORTKERNELS_SYMBOLS) == sorted(NAMES)
    for name, (ret, params) in protos.items():
        restype, argtypes = _ffi._SUPPORTKERNELS_SIGNATURES[name]
        assert agrees(ret, restype), name
        assert len(params) == len(argtypes), name
        for k, (decl, ctype) in enumerate(zip(params, argtypes)):
            assert agrees(decl, ctype), f'{name} parameter {k} is `{decl}`, the table says {ctype}'


def test_new_symbols_overlap_no_existing_list():
    old = set()
    for attr in dir(_ffi):
        if attr.endswith('SYMBOLS') and attr != 'SUPPORTKERNELS_SYMBOLS':
            old |= set(getattr(_ffi, attr))
    assert old and not set(_ffi.SUPPORTKERNELS_SYMBOLS) & old


def test_mipx_h_includes_the_header_behind_the_screen_and_keeps_its_version():
    text = open(os.path.join(ROOT, 'include', 'mipx.h')).read()
    assert 0 < text.index('#include "mipx_cglp_screen.h"') < text.index('#include "mipx_supportkernels.h"')
    assert _ffi.lib().mipx_abi_version() == 1
    assert 'TEST SCAFFOLDING' in open(os.path.join(ROOT, 'include', 'mipx_supportkernels.h')).read()
    assert '_ffi.SUPPORTKERNELS_SYMBOLS' in open(os.path.join(ROOT, '__graft_entry__.py')).read()
    needed = library_prerequisites()
    assert os.path.join(ROOT, 'include', 'mipx_supportkernels.h') in needed
    assert os.path.join(CSRC, 'supportkernels_api.hip.h') in needed


def test_library_exports_the_entries():
    L = _ffi.lib()
    for name in _ffi.SUPPORTKERNELS_SYMBOLS:
        assert hasattr(L, name), name
        assert getattr(L, name).restype is _ffi._SUPPORTKERNELS_SIGNATURES[name][0]


def test_c_entries_refuse_a_null_context():
    L = _ffi.lib()
    for name in NAMES:
        args = [1 if t in (_ffi._i, _ffi._i64) else 0.0 if t is _ffi._d else None for t in _ffi._SUPPORTKERNELS_SIGNATURES[name][1][1:]]
        assert getattr(L, name)(None, *args) == -1, name   # MIPX_EINVAL


def test_no_product_code_calls_the_scaffolding():
    short = [n[len('mipx_'):] for n in NAMES]
    pkg = os.path.join(ROOT, 'simple_mip_solver_amd')
    for base, _, files in os.walk(pkg):
        for f in files:
            if f.endswith('.py') and f != '_ffi.py':
                text = open(os.path.join(base, f)).read()
                assert not any(s in text for s in short), f
    for f in sorted(os.listdir(CSRC)):
        if f.endswith(('.h', '.hip')) and f != 'supportkernels_api.hip.h':
            text = open(os.path.join(CSRC, f)).read()
            assert not any(n in text for n in NAMES), f


def test_the_support_kernels_are_launched_from_one_place():
    """One copy of the grid rule per kernel: the enqueue_support_* functions of tree_engine.hip.h, which the session,
    mipx_support_screen_batch (both in cglp_api.hip.h) and the entries of supportkernels_api.hip.h go through; they
    alone set the leaves, the count and the segments into the args."""
    sources = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith(('.h', '.hip'))}
    engine, session, api = sources['tree_engine.hip.h'], sources['cglp_api.hip.h'], sources['supportkernels_api.hip.h']
    for kernel in KERNELS:
        hits = [f for f, text in sources.items() for _ in re.finditer(r'hipLaunchKernelGGL\(\s*\(?\s*mipx::%s\b' % kernel, text)]
        assert hits == ['tree_engine.hip.h'], (kernel, hits)
        assert sum(len(re.findall(r'\b%s\s*<<<' % kernel, text)) for text in sources.values()) == 0, kernel
        assert len(re.findall(r'^void enqueue_%s\(' % kernel, engine, flags=re.M)) == 1, kernel
        body = engine[engine.index('void enqueue_%s(' % kernel):]
        body = body[:body.index('\n}')]
        assert body.count('hipLaunchKernelGGL') == 1 and 'mipx::%s,' % kernel in body, kernel
    for text in (session, api):
        assert 'hipLaunchKernelGGL' not in text and 'dim3' not in text and '<<<' not in text
        assert not re.search(r'\.(G|count)\s*=[^=]', text)
    # (the T of a gather or a scatter is the kernels' guard on a packed position, not a grid: its callers set it)
    assert len(re.findall(r'\b\w+\.T\s*=[^=]', session)) == 1 and 'g.T = (int)s->T' in session
    assert len(re.findall(r'\b\w+\.T\s*=[^=]', api)) == 2 == api.count('a.T = (int)T; a.n = n; a.m = m; a.packed = ')
    # the session: every kernel once, the pack pair a second time in mipx_support_screen_batch; the entries: every kernel
    # but the screen once (the screen's entry is mipx_support_screen_batch)
    want_session = dict.fromkeys(KERNELS, 1)
    want_session.update(support_pack_count=2, support_pack=2)
    for kernel in KERNELS:
        assert len(re.findall(r'\benqueue_%s\(' % kernel, session)) == want_session[kernel], kernel
        assert len(re.findall(r'\benqueue_%s\(' % kernel, api)) == (0 if kernel == 'support_screen' else 1), kernel
        users = [f for f, text in sources.items() if re.search(r'(?<!void )\benqueue_%s\(' % kernel, text)]
        assert users == (['cglp_api.hip.h'] if kernel == 'support_screen' else ['cglp_api.hip.h', 'supportkernels_api.hip.h']), (kernel, users)
    assert session.count('sup_launch_screen(ctx') == 2 and session.count('sup_pack(s, sup_pack_args(') == 2
    assert 'kSupSeg == mipx::kScrSeg' in engine and re.search(r'\bkSupSeg = kSupNT \* kSupItems\b', sources['cglp_kernels.hip.h'])
    assert SEG == 256 * 8


# ---- the reference against other statements of the same thing ----------------------------------------------------------------
SMALL = [(content, T, P) for content in ref.CONTENTS for T in (1, 65, 2049, 3 * SEG + 5) for P in (1, 16, 1024)]


@pytest.mark.parametrize('content, T, P', SMALL + [('mixed', ref.T_WAVES, 16), ('ties', ref.T_TWICE, 16)])
def test_select_is_lexsort_over_the_ok_leaves(content, T, P):
    c = ref.select_case(content, T, 2 if T < ref.T_WAVES else 1, P)
    n = c['n']
    out = ref.select(c, ref.select_buffers(c))
    ok = (c['status'] == 0) & (c['obj'] == c['obj'])
    with np.errstate(invalid='ignore'):
        mg = np.where(ok, c['obj'] - c['pi0'], np.inf)
    assert ref.same_bits(out['margin'], mg)
    pos = np.flatnonzero(ok)
    order = pos[np.lexsort((c['ids'][pos], mg[pos]))]
    nsel = min(P, len(order))
    head, rows = out['block'][:ref.HEAD], out['block'][ref.HEAD:].reshape(P, n + 2)
    assert head[3] == nsel and head[7] == T and head[4] == T - len(pos)
    assert head[2] == (mg[pos] < -c['tol']).sum() and head[5] == c['iters'].astype(np.int64).sum()
    assert (head[0], head[1]) == ((mg[order[0]], c['ids'][order[0]]) if nsel else (np.inf, -1))
    assert ref.same_bits(rows[:nsel, 0], c['ids'][order[:nsel]].astype(np.float64))
    assert ref.same_bits(rows[:nsel, 1], c['obj'][order[:nsel]]) and ref.same_bits(rows[:nsel, 2:], c['x'][order[:nsel]])
    assert ref.untouched(rows[nsel:])
    for g in range(ref.segments(T)):
        mine = order[(order >= g * SEG) & (order < (g + 1) * SEG)][:P]
        k = len(mine)
        assert ref.same_bits(out['cand_t'][g, :k], mine.astype(np.int32)) and np.all(out['cand_t'][g, k:] == -1)
        assert ref.same_bits(out['cand_id'][g, :k], c['ids'][mine].astype(np.int32)) and np.all(out['cand_id'][g, k:] == ref.NONE)
        assert ref.same_bits(out['cand_m'][g, :k], mg[mine]) and np.all(out['cand_m'][g, k:] == np.inf)
    # the merged rows are the P smallest of the segments' candidates: the two-stage statement is the one-stage one
    cand = [(m, i, t) for m, i, t in zip(out['cand_m'].ravel().tolist(), out['cand_id'].ravel().tolist(), out['cand_t'].ravel().tolist())
            if i != ref.NONE]
    assert [t for _, _, t in sorted(cand)[:P]] == order[:nsel].tolist()
    assert ref.same_bits(out['seg_sum'].sum(axis=0), np.array([head[2], head[4], head[5], head[6]]))


def test_select_cases_hold_their_edges():
    T = 3 * SEG + 5
    for size in ref.SIZES:
        if size >= 255:
            k = ref.select_case('mixed', size, 2, 16)['kinds']
            assert k['status_bad'] and k['nan'] and k['pos_inf'] and k['neg_inf'] and k['tie_pairs'] and k['ids_unordered'], size
            assert k['max_id'] == ref.MAX_ID == 2 ** 31 - 2
    for P in (1, 16, 1024):
        k = ref.select_case('ties', T, 2, P)['kinds']
        assert k['ties_across_segments'] and k['ties_descending_ids'] and k['neg_zero'] and k['tie_pairs'] > T // 2
        assert ref.select_case('empty-segment', T, 2, P)['kinds']['empty_segments'] == 1
        k = ref.select_case('none-ok', T, 2, P)['kinds']
        assert k['ok'] == 0 and k['nan'] and k['status_bad']
        k = ref.select_case('few-ok', T, 2, P)['kinds']
        assert (P == 1 or k['short_segments'] >= 1) and (P <= 3 or (k['short_overall'] and k['ok'] > 0))   # (P = 1: none can be short)
        k = ref.select_case('tol-edge', T, 2, P)['kinds']
        assert k['at_tol'] and k['just_below_tol']
        k = ref.select_case('big-counts', T, 2, P)['kinds']
        assert k['iters_total'] > 2 ** 32 and k['pivots_total'] > 2 ** 32 and k['iters_total'] < 2 ** 53
    assert (ref.T_WAVES, ref.T_TWICE) == (65 * 2048 + 3, 257 * 2048 + 3) and ref.segments(ref.T_65) == 65
    assert ref.segments(ref.T_WAVES) == 66 and ref.segments(ref.T_TWICE) == 258 and ref.segments(2048) == 1 and ref.segments(2049) == 2
    c = ref.select_case('mixed', 5, 2, 3)
    assert len(set(c['ids'].tolist())) == 5 and not c['ids'].flags.writeable


@pytest.mark.parametrize('T', ref.SIZES + (ref.T_WAVES,))
def test_pack_is_flatnonzero(T):
    for density in ref.DENSITIES:
        c = ref.pack_case(density, T)
        for mode, skip, status, bound in ((0, c['skip'], None, c['bound']), (0, c['skip'], None, None), (1, None, c['status'], None)):
            out = ref.pack(T, mode, c['pi0'], skip, status, bound, ref.pack_buffers(T))
            keep = np.flatnonzero(c['take'])
            count = int(out['count'][0])
            assert count == len(keep) and ref.same_bits(out['packed'][:count], keep.astype(np.int32)) and ref.untouched(out['packed'][count:])
            assert out['seg_count'].sum() == count and len(out['seg_count']) == ref.segments(T)
            left = ~c['take']
            want = (c['bound'][left] - c['pi0']).min() if mode == 0 and bound is not None and left.any() else np.inf
            assert out['min_margin'][0] == want == out['seg_min'].min()


def test_pack_cases_hold_their_edges():
    for T in (2049, 3 * SEG + 5, ref.T_WAVES, ref.T_TWICE):
        G = ref.segments(T)
        assert ref.pack_case('first', T)['take'].nonzero()[0].tolist() == [0]
        assert ref.pack_case('last', T)['take'].nonzero()[0].tolist() == [T - 1]
        assert ref.pack_case('first-of-segment', T)['take'].nonzero()[0].tolist() == [(G - 1) * SEG]
        assert ref.pack_case('last-of-segment', T)['take'].nonzero()[0].tolist() == [(G - 1) * SEG - 1]
        if G >= 3:
            take = ref.pack_case('empty-middle-segment', T)['take']
            assert not take[(G // 2) * SEG:(G // 2 + 1) * SEG].any() and take[:SEG].any() and take[(G // 2 + 1) * SEG:].any()
        for spot in ref.MARGIN_SPOTS[:3]:
            c = ref.pack_case('half', T, spot)
            at = c['at']
            assert not c['take'][at] and c['bound'][at] == -7.625 and (c['bound'][~c['take']] > -7.625).sum() == (~c['take']).sum() - 1
            assert {'last-segment': at // SEG == G - 1, 'first-segment': at < SEG, 'last-item-of-a-thread': at % 8 == 7}[spot]
            assert c['bound'][c['take']].max() < -7.625
        assert ref.pack_case('all', T, 'absent')['take'].all()


def test_move_cases_hold_their_edges():
    assert ref.MOVE_SHAPES == ((1, 0), (1, 1), (5, 3), (255, 1), (256, 0), (257, 255), (1024, 1024))
    for n, m in ref.MOVE_SHAPES:
        for T in ref.MOVE_LEAVES:
            counts = ref.move_counts(T)
            assert {0, 1, T} <= set(counts) and (T < 4 or T // 2 in counts)
            for count in counts:
                c = ref.move_case(n, m, T, count)
                p = c['packed']
                assert len(p) == count and np.all(np.diff(p) > 0) and (count == 0 or (0 <= p[0] and p[-1] < T))
                if count >= 4:
                    pairs = {(int(c['leaf']['has_y'][t]), int(s != 0)) for t, s in zip(p, c['lp']['pstatus'])}
                    assert pairs == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # scatter on a small case worked by hand
    leaf = dict(x=np.zeros((3, 1)), obj=np.zeros(3), y=np.full((3, 1), 7.0), v=np.zeros((3, 1 + 1), np.int8), status=np.zeros(3, np.int32),
                iters=np.array([10, 20, 30], np.int32), npivots=np.array([1, 2, 3], np.int32), has_y=np.array([1, 0, 1], np.uint8))
    lp = dict(px=np.array([[1.0], [2.0]]), pobj=np.array([5.0, 6.0]), py=np.array([[8.0], [9.0]]), pv_out=np.ones((2, 2), np.int8),
              pstatus=np.array([3, 0], np.int32), piters=np.array([4, 5], np.int32), pnpivots=np.array([1, 1], np.int32))
    ref.scatter(2, np.array([0, 1], np.int32), 1, lp, leaf)
    assert leaf['y'].ravel().tolist() == [7.0, 9.0, 7.0] and leaf['has_y'].tolist() == [1, 1, 1] and leaf['status'].tolist() == [3, 0, 0]
    assert leaf['iters'].tolist() == [14, 25, 30] and leaf['x'].ravel().tolist() == [1.0, 2.0, 0.0] and leaf['obj'].tolist() == [5.0, 6.0, 0.0]
    ref.scatter(1, np.array([2], np.int32), 0, lp, leaf)
    assert leaf['iters'].tolist() == [14, 25, 4] and leaf['has_y'].tolist() == [1, 1, 1] and leaf['status'][2] == 3 and leaf['y'][2, 0] == 7.0
    has_y = np.full(4, ref.FILL, np.uint8)
    ref.mark(3, np.array([0, 2, 0], np.int32), has_y)
    assert has_y.tolist() == [1, 0, 1, ref.FILL]


def test_the_chained_evaluation_has_leaves_that_fail_once_and_twice():
    from tests.test_support_kernels_gpu import drawn_evaluation
    e = drawn_evaluation()
    T, P = e['T'], e['P']
    assert (T, e['m'], e['n']) == (2049 + 300, 6, 9)
    leaf = {k: a.copy() for k, a in e['leaf'].items()}
    s = ref.evaluation(e['A'], e['b'], e['pi'], e['pi0'], e['tol'], e['screen_tol'], P, e['ids'], e['l'], e['u'], leaf, e['lp1'], e['lp2'])
    solved = int(s['pack1']['count'][0])
    screened = s['screen']['screened'] != 0
    assert 0 < solved < T and solved == T - screened.sum() == s['screen']['count']
    assert s['retried'] > 0 and 0 < s['retried_ok'] < s['retried']
    first_failed = np.flatnonzero(~screened & (e['lp1']['pstatus'] != 0))
    assert ref.same_bits(s['pack2']['packed'][:s['retried']], first_failed.astype(np.int32)) and 0.05 * solved < len(first_failed) < 0.2 * solved
    assert s['pack2']['min_margin'][0] == np.inf and s['pack1']['min_margin'][0] == (s['screen']['bound'][screened] - e['pi0']).min()
    twice = first_failed[e['lp2']['pstatus'][first_failed] != 0]
    assert ref.same_bits(np.flatnonzero(leaf['status'] != 0), twice) and s['select']['block'][4] == len(twice)
    assert ref.same_bits(leaf['y'][twice], e['leaf']['y'][twice]) and ref.same_bits(leaf['has_y'][twice], e['leaf']['has_y'][twice])
    once = np.setdiff1d(first_failed, twice)
    assert ref.same_bits(leaf['y'][once], e['lp2']['py'][once]) and np.all(leaf['has_y'][once] == 1)
    assert np.array_equal(leaf['iters'][once], e['lp1']['piters'][once] + e['lp2']['piters'][once])
    clean = np.flatnonzero(~screened & (e['lp1']['pstatus'] == 0))
    assert np.array_equal(leaf['iters'][clean], e['lp1']['piters'][clean]) and ref.same_bits(leaf['y'][clean], e['lp1']['py'][clean])
    assert np.all(leaf['iters'][screened] == 0) and ref.same_bits(leaf['obj'][screened], s['screen']['bound'][screened])
    assert ref.same_bits(leaf['x'][screened], e['leaf']['x'][screened]) and ref.same_bits(leaf['v'][screened], e['leaf']['v'][screened])
    assert ref.untouched(s['gather1']['pl'][solved:]) and ref.untouched(s['gather2']['pv_in']) and not ref.untouched(s['gather2']['pl'])
