"""The device finish (csrc/finish_kernels.hip.h) on synthetic steps, through mipx_finish_step_batch and
mipx_pc_apply_batch (include/mipx_finish.h: the same launches as the engine's, enqueue_finish), against the plain
restatement of the reference's loop in tests/support/finish_reference.py -- at every width of the one-workgroup kernels
(1 to 5 chains a thread), every register width of finish_write, the outcomes a search rarely produces and the chunk
edges of pc_apply.  Nothing here is a tolerance: every comparison is exact."""
import numpy as np
import pytest

from tests.support import finish_reference as ref

pytestmark = pytest.mark.gpu
FILL = 0x5a
TABLE = ('cost_l', 'cost_r', 'has', 'times', 'own')


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def untouched(a, start=0):
    return bool(np.all(a.view(np.uint8).reshape(len(a), -1)[start:] == FILL))


@pytest.mark.parametrize('name', list(ref.CASES))
def test_finish_step_equals_the_restatement(gpu_ctx, name):
    from simple_mip_solver_amd import _ffi
    step, want = ref.case(name)
    got = _ffi.finish_step_batch(gpu_ctx, step, fill=FILL)
    sm, ws = got['summary'], want['summary']
    if ws['host_path']:
        # more requests than the compact list holds: the flag, and every other output as the caller left it
        assert sm['host_path'] == 1
        assert np.all(np.frombuffer(sm.tobytes(), np.uint8)[4:] == FILL)
        assert untouched(got['open']) and untouched(got['dead']) and untouched(got['samples']) and untouched(got['sample_keys'])
        assert same_bits(got['primal'], np.float64(step['primal']))
        for k in ('pool_l', 'pool_u', 'pool_v') + TABLE:
            assert same_bits(got[k], step[k]), k
        return
    for field in ref.SUMMARY_FIELDS:
        assert same_bits(sm[field], sm[field].dtype.type(ws[field])), (field, sm[field], ws[field])
    assert np.all(np.frombuffer(sm.tobytes(), np.uint8)[80:] == FILL) and same_bits(sm['pad0'], np.frombuffer(bytes([FILL] * 4), np.int32)[0])
    n_open, n_dead, n_samples = ws['n_open'], ws['n_dead'], ws['n_samples']
    assert same_bits(got['open'][:n_open], want['open']) and untouched(got['open'], n_open)
    assert same_bits(got['dead'][:n_dead], want['dead']) and untouched(got['dead'], n_dead)
    assert same_bits(got['samples'][:n_samples], want['samples']) and untouched(got['samples'], n_samples)
    assert same_bits(got['sample_keys'][:n_samples], want['sample_keys']) and untouched(got['sample_keys'], n_samples)
    for k in ('pool_l', 'pool_u', 'pool_v'):
        assert same_bits(got[k], want[k]), k
    # rows outside the budget and the batch's own rows still hold the sentinel
    spare = np.setdiff1d(np.arange(len(got['pool_l'])), np.concatenate([step['slot'], step['budget'].ravel()]))
    assert len(spare) and np.all(got['pool_l'][spare] == ref.SENTINEL_BOUND) and np.all(got['pool_u'][spare] == ref.SENTINEL_BOUND)
    assert np.all(got['pool_v'][spare] == ref.SENTINEL_BASIS)
    assert same_bits(got['primal'], np.float64(want['primal']))
    if step['rule'] == 1:
        for k in TABLE:
            assert same_bits(got[k], want[k]), k
    else:
        assert all(got[k] is None for k in TABLE)


@pytest.mark.parametrize('name', ref.SAMPLE_CASES)
def test_pc_apply_on_host_sent_samples_equals_the_restatement(gpu_ctx, name):
    """The count >= 0 way in: statuses that cost (0, 3) and statuses that only count (1, 2, 4) in one list."""
    from simple_mip_solver_amd import _ffi
    step, samples = ref.host_samples(name)
    table = [step[k] for k in TABLE]
    want = ref.apply_samples(samples, *table)
    got = _ffi.pc_apply_batch(gpu_ctx, step['n'], samples, *table)
    for k, g, w in zip(TABLE, got, want):
        assert same_bits(g, w), k
    if len(samples) == 0:
        for g, before in zip(got, table):
            assert same_bits(g, before)


def test_entries_refuse_what_is_out_of_range(gpu_ctx):
    from simple_mip_solver_amd import _ffi
    step, _ = ref.case('outcome-tie-small')
    # the scalars are refused before any array is looked at: one buffer, larger than any array of the valid call
    buf = np.zeros(1 << 12, np.float64)
    p = _ffi._ptr(buf)
    scalars = dict(n=5, m=3, B=7, dive=1, rule=1, ask_count=0, ask_cap=16, pool_rows=40)

    def call(**change):
        v = dict(scalars, **change)
        return _ffi.lib().mipx_finish_step_batch(gpu_ctx._h, v['n'], v['m'], v['B'], v['dive'], v['rule'], v['ask_count'], v['ask_cap'],
                                                 *([p] * 7), v['pool_rows'], *([p] * 14))
    for change in (dict(B=0), dict(B=-3), dict(dive=9), dict(dive=-1), dict(n=0), dict(n=1025), dict(m=-1), dict(rule=2),
                   dict(pool_rows=0)):
        assert call(**change) == -1, change      # MIPX_EINVAL
    assert _ffi.lib().mipx_pc_apply_batch(gpu_ctx._h, 1025, 0, None, None, *([p] * 5)) == -1
    assert _ffi.lib().mipx_pc_apply_batch(gpu_ctx._h, 5, -1, p, p, *([p] * 5)) == -1
    assert _ffi.lib().mipx_pc_apply_batch(gpu_ctx._h, 5, 3, None, None, *([p] * 5)) == -1
    rows = len(step['pool_l'])
    for key, index, value in (('slot', 0, rows), ('slot', 1, -1), ('budget', (2, 3), rows), ('budget', (0, 0), -1)):
        bad = dict(step)
        bad[key] = np.array(step[key])
        bad[key][index] = value
        with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*outside the pool'):
            _ffi.finish_step_batch(gpu_ctx, bad)
