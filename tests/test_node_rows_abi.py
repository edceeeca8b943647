"""The kernels that move node rows on a caller's pools (include/mipx_noderows.h), the parts that need no GPU: the
header against the ctypes table and the exported symbols, the one launch site of every kernel, and the reference the
kernels are compared with (tests/support/node_rows_reference.py): the two statements of a lineage against each other
and against hand-worked trees, the spill encoder against its decoder, and that the named cases hold what their names
say."""
import os
import re

import numpy as np
import pytest

from simple_mip_solver_amd import _ffi
from tests.support import node_rows_reference as ref
from tests.support.abi_check import agrees, prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'simple_mip_solver_amd', 'csrc')
NAMES = ['mipx_noderows_children', 'mipx_noderows_pack', 'mipx_noderows_unpack', 'mipx_noderows_gather_plain',
         'mipx_noderows_lineage_bounds', 'mipx_noderows_lineage_seed', 'mipx_noderows_cut_lists', 'mipx_noderows_cut_gather',
         'mipx_noderows_cut_scatter', 'mipx_noderows_cut_unpack_lists', 'mipx_noderows_spill_pack',
         'mipx_noderows_spill_unpack', 'mipx_noderows_spill_gather_rows']
KERNELS = ['make_children', 'pack_nodes', 'unpack_nodes', 'gather_plain_nodes', 'treerec_bounds', 'restart_seed', 'cutmig_lists',
           'cutmig_gather', 'cutmig_scatter', 'cutmig_unpack_lists', 'spill_count', 'spill_scan', 'spill_pack', 'spill_unpack',
           'spill_gather_rows']


def test_header_and_signature_table_agree():
    protos = prototypes('mipx_noderows.h')
    assert sorted(protos) == sorted(_ffi.NODEROWS_SYMBOLS) == sorted(NAMES)
    for name, (ret, params) in protos.items():
        restype, argtypes = _ffi._NODEROWS_SIGNATURES[name]
        assert agrees(ret, restype), name
        assert len(params) == len(argtypes), name
        for k, (decl, ctype) in enumerate(zip(params, argtypes)):
            assert agrees(decl, ctype), f'{name} parameter {k} is `{decl}`, the table says {ctype}'


def test_new_symbols_overlap_no_existing_list():
    old = set()
    for attr in dir(_ffi):
        if attr.endswith('SYMBOLS') and attr != 'NODEROWS_SYMBOLS':
            old |= set(getattr(_ffi, attr))
    assert old and not set(_ffi.NODEROWS_SYMBOLS) & old


def test_mipx_h_includes_the_header_and_keeps_its_version():
    text = open(os.path.join(ROOT, 'include', 'mipx.h')).read()
    assert '#include "mipx_noderows.h"' in text
    assert _ffi.lib().mipx_abi_version() == 1
    assert 'TEST SCAFFOLDING' in open(os.path.join(ROOT, 'include', 'mipx_noderows.h')).read()
    entry = open(os.path.join(ROOT, '__graft_entry__.py')).read()
    assert '_ffi.NODEROWS_SYMBOLS' in entry


def test_library_exports_the_entries():
    L = _ffi.lib()
    for name in _ffi.NODEROWS_SYMBOLS:
        assert hasattr(L, name), name
        assert getattr(L, name).restype is _ffi._NODEROWS_SIGNATURES[name][0]


def test_c_entries_refuse_a_null_context():
    L = _ffi.lib()
    for name in NAMES:
        args = [1 if t in (_ffi._i, _ffi._i64) else None for t in _ffi._NODEROWS_SIGNATURES[name][1][1:]]
        assert getattr(L, name)(None, *args) == -1, name   # MIPX_EINVAL


def test_no_product_code_calls_the_scaffolding():
    pkg = os.path.join(ROOT, 'simple_mip_solver_amd')
    for base, _, files in os.walk(pkg):
        for f in files:
            if f.endswith('.py') and f != '_ffi.py':
                assert 'noderows_' not in open(os.path.join(base, f)).read(), f
    for f in sorted(os.listdir(CSRC)):
        if f.endswith(('.h', '.hip')) and f != 'noderows_api.hip.h':
            assert 'mipx_noderows_' not in open(os.path.join(CSRC, f)).read(), f


def test_the_node_row_kernels_are_launched_from_one_place():
    """One copy of the grid, block and LDS rule per kernel: the enqueue_* functions of tree_engine.hip.h, which the
    engine's sites and the entries of noderows_api.hip.h both go through."""
    sources = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith(('.h', '.hip'))}
    for kernel in KERNELS:
        hits = [f for f, text in sources.items() for _ in re.finditer(r'hipLaunchKernelGGL\(\s*\(?\s*mipx::%s\b' % kernel, text)]
        assert hits == ['tree_engine.hip.h'], (kernel, hits)
        # ... and nothing launches it by another spelling
        assert sum(len(re.findall(r'\b%s\s*<<<' % kernel, text)) for text in sources.values()) == 0, kernel
        assert len(re.findall(r'^void enqueue_%s\(' % kernel, sources['tree_engine.hip.h'], flags=re.M)) == 1, kernel
    api = sources['noderows_api.hip.h']
    assert 'hipLaunchKernelGGL' not in api and 'dim3' not in api
    for kernel in KERNELS:
        assert api.count('enqueue_%s(' % kernel) == 1, kernel
    users = {'make_children': ['tree_engine.hip.h'], 'treerec_bounds': ['cglp_api.hip.h', 'treerec_api.hip.h'],
             'restart_seed': ['restart_api.hip.h'], 'spill_pack': ['mipx.hip', 'tree_engine.hip.h'],
             'spill_unpack': ['mipx.hip', 'tree_engine.hip.h'], 'cutmig_scatter': ['tree_engine.hip.h']}
    for kernel, files in users.items():
        got = [f for f, text in sources.items() if f != 'noderows_api.hip.h' and
               len(re.findall(r'(?<!void )enqueue_%s\(' % kernel, text)) > 0]
        assert got == files, (kernel, got)


def test_the_lineage_walk_keeps_its_ownership_rule():
    """treerec_bounds and restart_seed have no barrier and no atomic because column j is initialised and branched by
    thread j % 256 alone.  Dropping the rule gives the same bits whenever every initialising store happens to land
    before the first branching (one GPU run of that mutant passed every lineage case), so no comparison of outputs can
    hold it: the sources are read instead."""
    def code(path):   # the source without comments, every run of white space one blank
        text = re.sub(r'//[^\n]*', '', open(os.path.join(CSRC, path)).read())
        return re.sub(r'\s+', ' ', text)
    rec, seed = code('treerec_kernels.hip.h'), code('restart_kernels.hip.h')
    walk = rec[rec.index('void tr_apply_lineage('):rec.index('__global__')]
    guards = re.findall(r'if \(([^{}]*)\) \{[^{}]*seen\[var\]', walk)        # the condition around every use of the column
    assert len(guards) == 1 and re.search(r'\(? ?var % kTrNT ?\)? == tid', guards[0]), guards
    stores = [m.start() for m in re.finditer(r'(lo|up|seen)\[var\] ?\|?=[^=]', walk)]
    assert len(stores) == 3 and min(stores) > walk.index(guards[0])       # no store to the column outside the guard
    for text, kernel in ((rec, 'treerec_bounds'), (seed, 'restart_seed')):
        body = text[re.search(r'\b%s ?\(' % kernel, text).start():]
        assert re.search(r'\btid = threadIdx\.x\b', body)
        assert len(re.findall(r'for \(int j = tid; j < n; j \+= kTrNT\)', body)) == 1   # the owner initialises its columns
        assert len(re.findall(r'tr_apply_lineage\([^;]*\btid\b[^;]*\);', body)) == 1
        assert '__syncthreads' not in body and 'atomic' not in body
    assert re.search(r'\bkTrNT = 256\b', rec)
    assert 'test_the_lineage_walk_keeps_its_ownership_rule' in open(os.path.join(CSRC, 'treerec_kernels.hip.h')).read()


# ---- the lineage: two statements, and trees worked by hand ---------------------------------------------------------------
@pytest.mark.parametrize('name', ref.LINEAGE_CASES)
def test_the_walk_up_is_the_descent(name):
    c = ref.case(name)
    for a, b in zip(ref.bounds_restated(c, ref.walk), ref.bounds_restated(c, ref.descend)):
        assert ref.same_bits(a, b)
    for a, b in zip(ref.seed_restated(c, ref.walk), ref.seed_restated(c, ref.descend)):
        assert ref.same_bits(a, b)


def test_hand_worked_trees():
    # three levels, n = 3, root [0, 9]^3:
    #   0 -+- 1: x0 <= floor(2.5)  -+- 3: x1 >= ceil(4.2)
    #      |                        +- 4: x0 <= floor(1.5)
    #      +- 2: x0 >= ceil(2.5)   --- 5: x0 >= ceil(-0.5): the bound goes DOWN to -0.0, as the search's overwrite did
    parent, vd, val = [-1, 0, 0, 1, 1, 2], [-2, 0, 1, 3, 0, 1], [0.0, 2.5, 2.5, 4.2, 1.5, -0.5]
    rl, ru = np.zeros(3), np.full(3, 9.0)
    rows = {0: ([0, 0, 0], [9, 9, 9]), 1: ([0, 0, 0], [2, 9, 9]), 2: ([3, 0, 0], [9, 9, 9]), 3: ([0, 5, 0], [2, 9, 9]),
            4: ([0, 0, 0], [1, 9, 9]), 5: ([-0.0, 0, 0], [9, 9, 9])}
    for how in (ref.walk, ref.descend):
        for node, (lo, up) in rows.items():
            l, u = how(parent, vd, val, node, rl, ru)
            assert ref.same_bits(l, np.array(lo, float)) and ref.same_bits(u, np.array(up, float)), (how.__name__, node)
    assert np.signbit(ref.descend(parent, vd, val, 5, rl, ru)[0][0])
    # four levels on one column (n = 300, column 260, whose thread also owns column 4): left 9.5, right 2.5, left 6.5,
    # then column 4 right at 1.5: the LAST left branching stands, u = 6, although the walk up meets it first
    parent, vd, val = [-1, 0, 1, 2, 3], [-2, 520, 521, 520, 9], [0.0, 9.5, 2.5, 6.5, 1.5]
    rl, ru = np.full(300, -ref.INF), np.full(300, ref.INF)
    for how in (ref.walk, ref.descend):
        l, u = how(parent, vd, val, 4, rl, ru)
        assert (l[260], u[260], l[4], u[4]) == (3.0, 6.0, 2.0, ref.INF)
        assert np.all(np.delete(l, [4, 260]) == -ref.INF) and np.all(np.delete(u, [260]) == ref.INF)
        l, u = how(parent, vd, val, 2, rl, ru)
        assert (l[260], u[260], l[4]) == (3.0, 9.0, -ref.INF)
    # the guards: an id past the mirror is the root's row; a parent that is not below its child ends the walk after the
    # child's own branching; a variable outside 0 .. n-1 is passed over
    parent, vd, val = [-1, 0, 2, 1], [-2, 0, 3, 2 * 5], [0.0, 1.5, 2.5, 3.5]
    rl, ru = np.zeros(2), np.full(2, 9.0)
    for how in (ref.walk, ref.descend):
        assert [a.tolist() for a in how(parent, vd, val, 4, rl, ru)] == [[0, 0], [9, 9]]
        assert [a.tolist() for a in how(parent, vd, val, 2, rl, ru)] == [[0, 3], [9, 9]]
        assert [a.tolist() for a in how(parent, vd, val, 3, rl, ru)] == [[0, 0], [1, 9]]


# ---- the spill encoder against its decoder --------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [n for n in ref.SPILL_CASES if 'count4100' in n or 'n1024' in n or 'n65-' in n])
def test_decode_inverts_encode(name):
    c = ref.case(name)
    keys = ('l', 'u', 'v') + (('ncut', 'ids') if c['kc'] else ())
    got = ref.decode(c['root_l'], c['root_u'], c['offsets'], c['records'], c['slot'], *(ref.filled(c[k].shape, c[k].dtype) for k in keys))
    sel = np.arange(c['count']) if c['slot'] is None else c['slot']
    rest = np.setdiff1d(np.arange(len(c['l'])), sel)
    for g, k in zip(got, keys):
        if k == 'ids':
            for r in sel:
                assert ref.same_bits(g[r, :c['ncut'][r]], c['ids'][r, :c['ncut'][r]])
                assert np.all(g[r, c['ncut'][r]:].view(np.uint8) == ref.FILL)
        else:
            assert ref.same_bits(g[sel], c[k][sel]), (name, k)
        assert np.all(g[rest].view(np.uint8) == ref.FILL)
    sizes = np.diff(c['offsets'])
    assert np.all(sizes >= 16) and np.all(sizes % 8 == 0) and c['offsets'][0] == 0


# ---- the cases -------------------------------------------------------------------------------------------------------
def test_cases_hold_what_the_tests_are_there_for():
    assert [ref.case(n)['n'] for n in ref.CHILDREN_PLAIN] == list(ref.WIDTHS_256)
    assert [ref.case(n)['n'] for n in ref.MESSAGE_CASES] == [ref.case(n)['n'] for n in ref.GATHER_CASES] == list(ref.WIDTHS_256)
    assert [ref.case(n)['n'] for n in ref.LINEAGE_CASES[:8]] == [ref.case(n)['n'] for n in ref.GATHER_ROWS_CASES] == list(ref.WIDTHS_256)
    # children
    seen_kcut, seen_slack = set(), set()
    for name in ref.CHILDREN_CASES:
        c = ref.case(name)
        n, m, count = c['n'], c['m'], len(c['var'])
        pairs = list(zip(c['parent_pos'].tolist(), c['var'].tolist()))
        assert len(set(pairs)) == count                                            # every (pos, var) holds one pair's x
        xs = {float(c['x'][p, j]) for p, j in pairs}
        assert xs == set(ref.BRANCH_VALUES) and np.signbit(np.ceil(-0.5))
        assert set(c['var'].tolist()) == {v for v in (0, 255, 256, n - 1) if 0 <= v < n}
        cs = c['child_slot']
        assert len(set(cs.tolist())) == 2 * count and cs.min() == 0 and cs.max() == len(c['dst_l']) - 1
        assert len(c['dst_l']) > 2 * count and not np.array_equal(cs, np.sort(cs))
        assert {0, 4} <= set(c['parent_slot'].tolist()) and len(c['src_l']) == 5
        first = c['var'][:len(set(c['var'].tolist()))]
        assert n == 1 or (len(set(first.tolist())) == len(first) > 1 and len(set(c['parent_slot'][:len(first)].tolist())) == 1)
        assert c['src_l'][4, c['var'][0]] == -ref.INF and c['src_u'][4, c['var'][0]] == ref.INF and c['parent_slot'][0] == 4
        if n > 4:
            free = np.setdiff1d(np.arange(n), c['var'])
            assert any(np.signbit(c['src_l'][4, j]) and c['src_l'][4, j] == 0.0 for j in free)
        if c['mstride']:
            assert c['mstride'] >= m + c['kc']
            for p in c['parent_pos']:
                seen_kcut.add(int(c['src_ncut'][p]))
                seen_slack.add('tight' if c['mstride'] == m + c['src_ncut'][p] else 'loose')
    assert {0, 1, 63, 64} <= seen_kcut and seen_slack == {'tight', 'loose'}
    assert {ref.case(n)['mstride'] - ref.case(n)['m'] for n in ref.CHILDREN_CUT} >= {0, 1, 63, 64}
    nvs = [ref.case(n)['n'] + ref.case(n)['m'] for n in ref.CHILDREN_PLAIN]
    assert any(v % 2 for v in nvs) and any(v % 2 == 0 for v in nvs) and max(nvs) > 1024 and sum(256 < v <= 1024 for v in nvs)
    # message and the gathers
    assert {s[1] % 8 for s in ref.MESSAGE_SHAPES} >= {0, 1, 7} and max(s[1] for s in ref.MESSAGE_SHAPES) > 1024
    assert any((16 * n + v) % 8 for n, v in ref.MESSAGE_SHAPES) and any((16 * n + v) % 8 == 0 for n, v in ref.MESSAGE_SHAPES)
    for name in ref.MESSAGE_CASES:
        c = ref.case(name)
        for s, rows in ((c['slot'], len(c['pool_l'])), (c['other'], len(c['pool_l']) + 2)):
            assert len(set(s.tolist())) == len(s) and s.min() == 0 and s.max() == rows - 1 and rows > len(s)
            assert not np.array_equal(s, np.sort(s))
        assert not np.array_equal(c['slot'], c['other'])
    wider = [p > n + m for n, m, p in ref.GATHER_SHAPES]   # (equal: the pool of a search without cut rounds)
    assert sum(wider) >= 4 and not all(wider) and all(p >= n + m for n, m, p in ref.GATHER_SHAPES)
    for name in ref.GATHER_ROWS_CASES:
        s = ref.case(name)['slot']
        assert (s < 0).sum() == 2 and s.max() == 5 and (s == 0).sum() == 2
    # lineage
    for name in ref.LINEAGE_CASES[:8]:
        c = ref.case(name)
        ids = c['ids'].tolist()
        assert len(ids) > len(set(ids)) and 0 in ids and ids != sorted(ids)
        depth = max(len(ref.path_up(c['parent'], i)) for i in ids)
        assert depth >= 3
        if c['n'] >= 512:   # some lineage holds two columns of one owner thread
            assert any(len({(int(c['vd'][i]) >> 1) % 256 for i in ref.path_up(c['parent'], k)}) <
                       len({int(c['vd'][i]) >> 1 for i in ref.path_up(c['parent'], k)}) for k in ids)
    c = ref.case('lineage-chain-3000')
    assert len(ref.path_up(c['parent'], c['ids'][0])) == 3000 and {0, 256} <= {int(v) >> 1 for v in c['vd'][1:]}
    c = ref.case('lineage-columns-n1024')
    cols = [int(c['vd'][i]) >> 1 for i in ref.path_up(c['parent'], c['ids'][0])]
    assert {255, 256, 257, 511, 1023, 3, 259} <= set(cols) and c['n'] == 1024
    c = ref.case('lineage-same-column')
    sides = [(int(v) >> 1, int(v) & 1) for v in c['vd'][1:]]
    assert sides[:3] == [(260, 0), (260, 1), (260, 0)] and sides[3:6] == [(4, 1)] * 3
    c = ref.case('lineage-malformed')
    N, n = len(c['parent']), c['n']
    assert sum(i >= N for i in c['ids']) == 2 and any(c['parent'][i] >= i for i in range(1, N))
    assert any((int(v) >> 1) >= n for v in c['vd']) and sum((int(v) >> 1) < 0 for v in c['vd'][1:]) == 2
    assert (c['slots'] < 0).sum() == 1 and (c['slots'] >= c['capacity']).sum() == 1
    l, _ = ref.lineage_rows(c)
    assert np.signbit(l[0, 1]) and l[0, 1] == 0.0                                   # ceil(-0.5) = -0.0 in a lineage
    assert ref.case('lineage-no-root-codes')['root_v'] is None and len(ref.case('lineage-empty-mirror')['parent']) == 0
    c = ref.case('lineage-two-chunks')
    assert len(c['ids']) > ref.LINEAGE_CHUNK and len(set(c['ids'][ref.LINEAGE_CHUNK:].tolist())) == 5
    assert 'kTrChunk = 1 << 14' in open(os.path.join(CSRC, 'treerec_api.hip.h')).read()
    l, u = ref.lineage_rows(c)
    assert len({(a, b) for a, b in zip(l[:, 0].tolist(), u[:, 0].tolist())}) >= 6    # (the rows tell the ids apart)
    c = ref.case('lineage-depth-1-2')
    assert [len(ref.path_up(c['parent'], i)) for i in c['ids']] == [0, 1, 1, 2, 2]
    # cut migration
    for kc in ref.CUT_KC:
        c = ref._cut_unpack_case(kc, 0, 7, kc)
        assert {'good-full', 'good-empty', 'nc=-1', 'nc=kc+1', 'ref=-1', 'ref=ctab'} <= set(c['what'])
        assert ref.cut_unpack_restated(c)[2] == 4
        assert set(ref._cut_unpack_case(kc, 5, 0, kc)['what']) >= {'good-empty', 'ref=ctab'}
    # spill
    counts = {ref.case(n)['count'] for n in ref.SPILL_CASES}
    assert counts == {1, 3, 4, 5, 1023, 1024, 1025, 2049, 4100}
    for k in (1023, 1024, 1025, 2049, 4100):
        assert {ref.case(n)['form'] for n in ref.SPILL_CASES if ref.case(n)['count'] == k} == set(ref.SPILL_FORMS)
    assert {ref.case(n)['n'] for n in ref.SPILL_CASES if ref.case(n)['count'] <= 5} == set(ref.WIDTHS_64)
    for name in ref.SPILL_CASES:
        c = ref.case(name)
        if c['slot'] is not None:
            s = c['slot']
            assert len(set(s.tolist())) == len(s) and s.max() == len(c['l']) - 1 and len(c['l']) > len(s)
            assert len(s) < 2 or (s.min() == 0 and not np.array_equal(s, np.sort(s)))
            assert c['node_id'].max() >= 1 << 32 or len(s) == 1
        if c['count'] >= 1023:   # the records differ in size: a scan that drops or repeats one moves every later offset
            assert len(set(np.diff(c['offsets']).tolist())) > 1
