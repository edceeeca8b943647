"""The four kernels of the dual function (csrc/dualfn_kernels.hip.h) on synthetic records, through the entries of
include/mipx_dualfn_batch.h (the same launches as the engine's: enqueue_df_record, enqueue_df_save and df_eval_tiles of
csrc/dualfn.hip.h), against tests/support/dualfn_reference.py: bit for bit against the restatement of the kernels'
documented order, within the derived bounds against the order-free definition, at every tile edge (R mod 64, K mod 16,
m mod 32, count mod 4, n mod 256, a level and a leaf list longer than 256) and at every launch shape."""
import ctypes
import math
from fractions import Fraction as F

import numpy as np
import pytest

from tests.support import dualfn_reference as ref

pytestmark = pytest.mark.gpu
FILL = 0x5a
EINVAL = -1


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def untouched(a):
    return bool(np.all(np.ascontiguousarray(a).view(np.uint8) == FILL))


def rows_but(rows, dst):
    return np.setdiff1d(np.arange(rows), dst)


# ---- dualfn_record ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ref.RECORD_CASES)
def test_record_equals_the_restatement(gpu_ctx, name):
    from simple_mip_solver_amd import _ffi
    s, want = ref.case(name)
    got = _ffi.dualfn_record_batch(gpu_ctx, s, fill=FILL)
    print(name, 't device', got['store_t'][s['dst']].tolist(), 'restated', want['t'].tolist())
    assert same_bits(got['store_t'][s['dst']], want['t'])
    assert same_bits(got['store_y'][s['dst']], want['y'])
    spare = rows_but(s['store_rows'], s['dst'])
    assert len(spare) == 3 and untouched(got['store_y'][spare]) and untouched(got['store_t'][spare])
    # ... and the definition, which knows no order, within the derived bound
    for e, (t_exact, bound) in enumerate(ref.defined(name)):
        t = float(got['store_t'][s['dst'][e]])
        if math.isfinite(float(want['t'][e])):
            assert math.isfinite(t) and abs(F(t) - t_exact) <= bound, (e, t, float(t_exact), float(bound))


@pytest.mark.parametrize('name', ref.RECORD_CASES)
def test_record_one_call_or_one_call_per_entry(gpu_ctx, name):
    """The same store whether the entries share workgroups of 4 or each has one of its own, three slots idle."""
    from simple_mip_solver_amd import _ffi
    s, _ = ref.case(name)
    whole = _ffi.dualfn_record_batch(gpu_ctx, s, fill=FILL)
    store = None
    for e in range(s['count']):
        one = dict(s, src=s['src'][e:e + 1], lrow=s['lrow'][e:e + 1], dst=s['dst'][e:e + 1], **(store or {}))
        store = _ffi.dualfn_record_batch(gpu_ctx, one, fill=FILL)
    assert same_bits(store['store_y'], whole['store_y']) and same_bits(store['store_t'], whole['store_t'])
    # no entry at all: nothing is launched and the store comes back as it went
    none = _ffi.dualfn_record_batch(gpu_ctx, dict(s, src=s['src'][:0], lrow=s['lrow'][:0], dst=s['dst'][:0], **whole), fill=FILL)
    assert same_bits(none['store_y'], whole['store_y']) and same_bits(none['store_t'], whole['store_t'])


# ---- dualfn_save -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ref.SAVE_CASES)
def test_save_equals_the_restatement(gpu_ctx, name):
    from simple_mip_solver_amd import _ffi
    s, want = ref.case(name)
    got = _ffi.dualfn_save_batch(gpu_ctx, s, fill=FILL)
    assert same_bits(got['out_l'][s['dst']], want['l']) and same_bits(got['out_u'][s['dst']], want['u'])
    assert same_bits(got['out_v'][s['dst']], want['v'])
    spare = rows_but(s['out_rows'], s['dst'])
    assert len(spare) == 3 and all(untouched(got[k][spare]) for k in ('out_l', 'out_u', 'out_v'))
    none = _ffi.dualfn_save_batch(gpu_ctx, dict(s, lrow=s['lrow'][:0], vpos=s['vpos'][:0], dst=s['dst'][:0]), fill=FILL)
    assert all(untouched(none[k]) for k in ('out_l', 'out_u', 'out_v'))


# ---- dualfn_gemm and dualfn_lineage ----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ref.EVAL_CASES)
def test_eval_equals_the_restatement(gpu_ctx, name):
    from simple_mip_solver_amd import _ffi
    s, want = ref.case(name)
    got = _ffi.dualfn_eval_batch(gpu_ctx, s, fill=FILL)
    differ = {k: int(np.sum(got[k].view(np.uint64) != want[k].view(np.uint64))) for k in ('V_gemm', 'V_max', 'out')}
    print(name, 'entries whose bits differ', differ, 'out', got['out'][:4].tolist())
    for k in ('V_gemm', 'V_max', 'out'):
        assert same_bits(got[k], want[k]), k
    # the definition: V within the derived bound, and given the device's own V the lineage by brute force, bitwise
    exact, bound = ref.defined(name)
    for k in range(s['K']):
        for r in range(s['R']):
            v = float(got['V_gemm'][k, r])
            if exact[k][r] is None:
                assert v == -ref.INF
            else:
                assert abs(F(v) - exact[k][r]) <= bound[k][r], (k, r)
    vmax, out = ref.lineage_defined(s, got['V_gemm'])
    assert same_bits(got['V_max'], vmax) and same_bits(got['out'], out)


def test_eval_bits_do_not_depend_on_the_tile(gpu_ctx):
    """K = 33 in one tile (the engine's rule), in 33 tiles of one, in tiles of 16 (16 + 16 + 1) and of 17 (17 + 16)."""
    from simple_mip_solver_amd import _ffi
    s, want = ref.case(ref.TILED_CASE)
    for k_tile in (0, 1, 16, 17):
        got = _ffi.dualfn_eval_batch(gpu_ctx, s, k_tile=k_tile, fill=FILL)
        for k in ('V_gemm', 'V_max', 'out'):
            assert same_bits(got[k], want[k]), (k_tile, k)


def test_eval_one_right_hand_side_alone_gives_its_row(gpu_ctx):
    """What mipx_dualfn.h promises: one w alone gives the same bits, whatever K."""
    from simple_mip_solver_amd import _ffi
    s, want = ref.case(ref.TILED_CASE)
    for k in range(s['K']):
        got = _ffi.dualfn_eval_batch(gpu_ctx, dict(s, W=s['W'][k:k + 1]), fill=FILL)
        assert same_bits(got['V_max'][0], want['V_max'][k]) and same_bits(got['out'], want['out'][k:k + 1]), k
        assert same_bits(got['V_gemm'][0], want['V_gemm'][k]), k


def test_eval_outputs_are_optional(gpu_ctx):
    from simple_mip_solver_amd import _ffi
    s, want = ref.case('eval-forest-3-roots-R63-m31-K15')
    out = _ffi._filled(s['K'], np.float64, FILL)
    rc = raw_eval(gpu_ctx, s, V_gemm=None, V_max=None, out=out)[0]
    assert rc == 0 and same_bits(out, want['out'])
    # no leaf list at all, some leaf bare: the kernels run and every value is -inf
    got = _ffi.dualfn_eval_batch(gpu_ctx, dict(s, leaf=s['leaf'][:0], bare=1), fill=FILL)
    assert np.all(got['out'] == -ref.INF) and same_bits(got['V_max'], want['V_max'])


# ---- refusals --------------------------------------------------------------------------------------------------------
def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _message(ctx):
    from simple_mip_solver_amd import _ffi
    msg = _ffi.lib().mipx_last_error(ctx._h)
    return msg.decode() if msg else ''


def raw_record(ctx, s, **change):
    """The C entry on a case with some arguments replaced (None: a null pointer).  Returns (rc, message, outputs)."""
    from simple_mip_solver_amd import _ffi
    v = dict(s, y_rows=len(s['y_src']), b_rows=len(s['l']), store_y=_ffi._filled((s['store_rows'], s['m']), np.float64, FILL),
             store_t=_ffi._filled(s['store_rows'], np.float64, FILL))
    v.update(change)
    rc = _ffi.lib().mipx_dualfn_record_batch(ctx._h, v['m'], v['n'], _p(v['A']), _p(v['c']), v['count'], _p(v['src']), _p(v['lrow']),
                                             _p(v['dst']), v['y_rows'], _p(v['y_src']), v['b_rows'], _p(v['l']), _p(v['u']),
                                             v['store_rows'], _p(v['store_y']), _p(v['store_t']))
    return rc, _message(ctx), [a for a in (v['store_y'], v['store_t']) if a is not None]


def raw_save(ctx, s, **change):
    from simple_mip_solver_amd import _ffi
    v = dict(s, b_rows=len(s['l']), v_rows=len(s['vstat']), out_l=_ffi._filled((s['out_rows'], s['n']), np.float64, FILL),
             out_u=_ffi._filled((s['out_rows'], s['n']), np.float64, FILL), out_v=_ffi._filled((s['out_rows'], s['nv']), np.int8, FILL))
    v.update(change)
    rc = _ffi.lib().mipx_dualfn_save_batch(ctx._h, v['n'], v['nv'], v['count'], _p(v['lrow']), _p(v['vpos']), _p(v['dst']), v['b_rows'],
                                           _p(v['l']), _p(v['u']), v['v_rows'], _p(v['vstat']), v['out_rows'], _p(v['out_l']),
                                           _p(v['out_u']), _p(v['out_v']))
    return rc, _message(ctx), [a for a in (v['out_l'], v['out_u'], v['out_v']) if a is not None]


def raw_eval(ctx, s, **change):
    from simple_mip_solver_amd import _ffi
    v = dict(s, k_tile=0, nlvl=len(s['lvl_off']) - 1, nleaf=len(s['leaf']), V_gemm=_ffi._filled((s['K'], s['R']), np.float64, FILL),
             V_max=_ffi._filled((s['K'], s['R']), np.float64, FILL), out=_ffi._filled(s['K'], np.float64, FILL))
    v.update(change)
    rc = _ffi.lib().mipx_dualfn_eval_batch(ctx._h, v['R'], v['m'], v['K'], v['k_tile'], _p(v['Y']), _p(v['T']), _p(v['W']), _p(v['prec']),
                                           _p(v['order']), _p(v['lvl_off']), v['nlvl'], _p(v['leaf']), v['nleaf'], v['bare'],
                                           _p(v['V_gemm']), _p(v['V_max']), _p(v['out']))
    return rc, _message(ctx), [a for a in (v['V_gemm'], v['V_max'], v['out']) if a is not None]


def put(a, index, value):
    b = np.array(a)
    b[index] = value
    return b


def refused(result, words):
    rc, message, outputs = result
    return rc == EINVAL and words in message and all(untouched(a) for a in outputs)      # (nothing was launched)


def test_record_and_save_refuse_what_is_out_of_range(gpu_ctx):
    from simple_mip_solver_amd import _ffi
    L = _ffi.lib()
    # the scalars are refused before any array is looked at: one buffer, larger than any array of the valid call
    buf = np.zeros(1 << 12, np.float64)
    p = _p(buf)
    scalars = dict(m=3, n=5, count=4, y_rows=6, b_rows=6, store_rows=7, nv=8, v_rows=6, out_rows=7)

    def record(**change):
        v = dict(scalars, **change)
        return L.mipx_dualfn_record_batch(gpu_ctx._h, v['m'], v['n'], p, p, v['count'], p, p, p, v['y_rows'], p, v['b_rows'], p, p,
                                          v['store_rows'], p, p)

    def save(**change):
        v = dict(scalars, **change)
        return L.mipx_dualfn_save_batch(gpu_ctx._h, v['n'], v['nv'], v['count'], p, p, p, v['b_rows'], p, p, v['v_rows'], p,
                                        v['out_rows'], p, p, p)
    for change in (dict(m=0), dict(m=-2), dict(n=0), dict(count=-1), dict(y_rows=0), dict(b_rows=0), dict(store_rows=0)):
        assert record(**change) == EINVAL, change
    for change in (dict(n=0), dict(nv=0), dict(count=-1), dict(b_rows=0), dict(v_rows=0), dict(out_rows=-1)):
        assert save(**change) == EINVAL, change
    assert not buf.any()
    s, _ = ref.case('record-m3-n5-count4')
    rows = len(s['y_src'])
    for key in ('A', 'c', 'src', 'lrow', 'dst', 'y_src', 'l', 'u', 'store_y', 'store_t'):
        assert refused(raw_record(gpu_ctx, s, **{key: None}), 'a null argument'), key
    for key, index, value, words in (('src', 0, rows, 'a src outside'), ('src', 3, -1, 'a src outside'), ('lrow', 2, rows, 'an lrow outside'),
                                     ('lrow', 0, -1, 'an lrow outside'), ('dst', 1, s['store_rows'], 'a dst outside'),
                                     ('dst', 3, -1, 'a dst outside'), ('dst', 2, 1 << 40, 'a dst outside'),
                                     ('dst', 3, int(s['dst'][0]), 'two equal dst')):
        assert refused(raw_record(gpu_ctx, s, **{key: put(s[key], index, value)}), words), (key, index, value)
    # rows the caller says are not there
    assert refused(raw_record(gpu_ctx, s, y_rows=int(s['src'].max())), 'a src outside')
    assert refused(raw_record(gpu_ctx, s, b_rows=int(s['lrow'].max())), 'an lrow outside')
    s, _ = ref.case('save-n255-nv300-count3')
    for key in ('lrow', 'vpos', 'dst', 'l', 'u', 'vstat', 'out_l', 'out_u', 'out_v'):
        assert refused(raw_save(gpu_ctx, s, **{key: None}), 'a null argument'), key
    for key, index, value, words in (('lrow', 0, len(s['l']), 'an lrow outside'), ('lrow', 2, -1, 'an lrow outside'),
                                     ('vpos', 1, len(s['vstat']), 'a vpos outside'), ('vpos', 0, -5, 'a vpos outside'),
                                     ('dst', 0, s['out_rows'], 'a dst outside'), ('dst', 2, -1, 'a dst outside'),
                                     ('dst', 1, int(s['dst'][2]), 'two equal dst')):
        assert refused(raw_save(gpu_ctx, s, **{key: put(s[key], index, value)}), words), (key, index, value)


def test_eval_refuses_what_is_out_of_range(gpu_ctx):
    from simple_mip_solver_amd import _ffi
    L = _ffi.lib()
    buf = np.zeros(1 << 12, np.float64)
    p = _p(buf)
    scalars = dict(R=8, m=3, K=4, k_tile=0, nlvl=2, nleaf=3, bare=0)

    def call(**change):
        v = dict(scalars, **change)
        return L.mipx_dualfn_eval_batch(gpu_ctx._h, v['R'], v['m'], v['K'], v['k_tile'], *([p] * 6), v['nlvl'], p, v['nleaf'], v['bare'],
                                        p, p, p)
    for change in (dict(R=0), dict(R=-1), dict(m=0), dict(K=0), dict(k_tile=-1), dict(nlvl=0), dict(nleaf=-1), dict(nleaf=0)):
        assert call(**change) == EINVAL, change
    assert not buf.any()
    s, _ = ref.case('eval-forest-3-roots-R63-m31-K15')
    R, order, off, prec = s['R'], s['order'], s['lvl_off'], s['prec']
    for key in ('Y', 'T', 'W', 'prec', 'order', 'lvl_off', 'leaf', 'out'):
        assert refused(raw_eval(gpu_ctx, s, **{key: None}), 'a null argument'), key
    assert refused(raw_eval(gpu_ctx, s, leaf=None, nleaf=0), 'no leaf and none bare')
    root, second, third = order[0], order[off[1]], order[off[2]]            # records of the levels 0, 1 and 2
    peer = order[off[2] + 1]                                               # ... and another of level 2
    for change, words in (
            (dict(lvl_off=put(off, 0, 1)), 'from 0 to R'), (dict(lvl_off=put(off, -1, R - 1)), 'from 0 to R'),
            (dict(lvl_off=put(off, -1, R + 1)), 'from 0 to R'), (dict(lvl_off=put(off, 2, off[1])), 'not ascending'),
            (dict(lvl_off=put(off, 1, off[2] + 1)), 'not ascending'), (dict(lvl_off=put(off, 1, -4)), 'not ascending'),
            (dict(nlvl=len(off) - 2), 'from 0 to R'),
            (dict(order=put(order, 5, order[6])), 'no permutation'), (dict(order=put(order, 0, R)), 'no permutation'),
            (dict(order=put(order, R - 1, -1)), 'no permutation'),
            (dict(prec=put(prec, root, second)), 'level 0 with an ancestor'), (dict(prec=put(prec, root, -2)), 'level 0 with an ancestor'),
            (dict(prec=put(prec, second, -1)), 'no record of a lower level'), (dict(prec=put(prec, second, R)), 'no record of a lower level'),
            (dict(prec=put(prec, third, peer)), 'no record of a lower level'), (dict(prec=put(prec, second, third)), 'no record of a lower level'),
            (dict(prec=put(prec, third, third)), 'no record of a lower level'),
            (dict(leaf=put(s['leaf'], 0, R)), 'a leaf outside'), (dict(leaf=put(s['leaf'], len(s['leaf']) - 1, -1)), 'a leaf outside')):
        assert refused(raw_eval(gpu_ctx, s, **change), words), list(change)
    # a prec that is a record of a lower level, though not the level just below, is a lineage the kernel handles
    rc, _, (V_gemm, V_max, out) = raw_eval(gpu_ctx, s, prec=put(prec, third, root))
    assert rc == 0
    vmax, want = ref.lineage_defined(dict(s, prec=put(prec, third, root)), V_gemm)
    assert same_bits(V_max, vmax) and same_bits(out, want)
