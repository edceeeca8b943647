"""The scripted second rank (tests/support/scripted_peer.py) without a GPU: its message layout against hand-worked
sizes of the wire format in include/mipx.h, encode / decode, the budget of a script, every script of
tests/test_rank_exchange_gpu.py against the product's own pure decision function (mipx_exchange_decide) -- this is what
says that the GPU cases reach the branches they are named after -- and the f64 merge recurrence against its exact
rational value within the derived bound."""
import itertools

import numpy as np
import pytest

from simple_mip_solver_amd import _ffi
from tests.support import scripted_peer as sp

INF = float('inf')


def test_layout_at_hand_worked_sizes():
    # plain, n = 3, m = 5: nvs = 8, a row is 24 + 24 + 8 = 56 bytes; two rows, then 1 + 10 doubles
    assert sp.layout(3, 8, 2) == sp.Layout(56, None, None, 112, 11, 5, 200)
    # nvs = 9, 12, 15 all pad to 16
    for nvs in (9, 12, 15):
        assert sp.layout(3, nvs, 1) == sp.Layout(64, None, None, 64, 6, 5, 112)
    assert sp.layout(3, 8, 0).bytes == 8 and sp.layout(3, 8, 0).meta_off == 0          # the count alone
    # cut mode, n = 3, m = 5, kc = 1: nvs = 9, rows of 64; 2 x 2 int32 = 16; one table row of 3 + 1 doubles; 1 + 12 + 1
    assert sp.layout(3, 9, 2, kc=1, ctab=1) == sp.Layout(64, 128, 144, 176, 14, 6, 288)
    # kc = 64: nvs = 72, rows of 48 + 72; 65 int32 = 260 -> 264; five table rows = 160 bytes; 1 + 6 + 1 doubles
    assert sp.layout(3, 72, 1, kc=64, ctab=5) == sp.Layout(120, 120, 384, 544, 8, 6, 608)
    assert sp.layout(3, 72, 0, kc=64, ctab=0) == sp.Layout(120, 0, 0, 0, 2, 6, 16)
    # n = 4, m = 3, kc = 1: nvs = 8; one list of 2 int32 = 8 (no pad); no table
    assert sp.layout(4, 8, 1, kc=1, ctab=0) == sp.Layout(72, 72, 80, 80, 8, 6, 144)
    # the whole grid against the sections added up one by one
    for nvs, amount, kc, ctab in itertools.product((16, 17, 20, 23), (0, 1, 2), (0, 1, 64), (0, 1, 5)):
        if kc == 0 and ctab:
            continue
        n = 5
        L = sp.layout(n, nvs + kc, amount, kc=kc, ctab=ctab)
        codes = nvs + kc
        while codes % 8:
            codes += 1
        total = amount * (8 * n + 8 * n + codes)
        if kc:
            lists = 4 * amount * (1 + kc)
            total += lists + (lists % 8 and 8 - lists % 8) + ctab * 8 * n + ctab * 8 + 8
        total += 8 + amount * 8 * (6 if kc else 5)
        assert L.bytes == total and L.bytes % 8 == 0 and L.meta_off + 8 * L.nmeta == L.bytes, (nvs, amount, kc, ctab)
    assert sp.table_rows(1e9, 3, 64) == 192 and sp.table_rows(3.0, 100, 64) == 3 and sp.table_rows(1e9, 4096, 64) == 1 << 14
    assert sp.table_rows(-1.0, 5, 64) == 0 and sp.table_rows(100, 0, 64) == 0
    assert sp.hand_amount(300, 1, 1 << 20) == 149 and sp.hand_amount(300, 1, 3) == 3 and sp.hand_amount(40000, 3, 1 << 20) == 4096


def random_rows(rng, n, nvs, k):
    l = rng.standard_normal((k, n))
    u = l + rng.random((k, n))
    u[rng.random((k, n)) < .2] = INF
    return l, u, rng.integers(-1, 3, (k, nvs)).astype(np.int8)


@pytest.mark.parametrize('n,m,amount,k', [(5, 3, 4, 4), (5, 4, 4, 2), (7, 6, 3, 0), (6, 1, 1, 1)])
def test_encode_decode_plain(n, m, amount, k):
    rng = np.random.default_rng(n * 100 + m)
    nvs = n + m
    l, u, codes = random_rows(rng, n, nvs, k)
    meta = rng.standard_normal((k, 5))
    a = sp.encode_message(n, nvs, amount, l, u, codes, meta, fill=0x5a)
    b = sp.encode_message(n, nvs, amount, l, u, codes, meta, fill=0xc3)
    assert len(a) == len(b) == sp.layout(n, nvs, amount).bytes
    assert (a != b) == (k < amount or nvs % 8 != 0)          # the two differ exactly when unspecified bytes exist
    for msg in (a, b):
        d = sp.decode_message(msg, n, nvs, amount)
        assert d['count'] == k
        assert d['l'].tobytes() == l.tobytes() and d['u'].tobytes() == u.tobytes()
        assert d['codes'].tobytes() == codes.tobytes() and d['meta'].tobytes() == meta.tobytes()


@pytest.mark.parametrize('kc,ctab,used', [(1, 1, 1), (64, 5, 3), (64, 5, 0), (8, 16, 16)])
def test_encode_decode_cut_mode(kc, ctab, used):
    rng = np.random.default_rng(kc + ctab)
    n, m, amount, k = 6, 3, 3, 2
    nvs = n + m + kc
    l, u, codes = random_rows(rng, n, nvs, k)
    lists = [rng.integers(0, used, min(kc, j + 1)).astype(np.int32) if used else np.zeros(0, np.int32) for j in range(k)]
    meta = np.concatenate([rng.standard_normal((k, 5)), np.array([[len(li)] for li in lists], float)], axis=1)
    pi, pi0 = rng.standard_normal((used, n)), rng.standard_normal(used)
    out = []
    for fill in (0x5a, 0xc3):
        msg = sp.encode_message(n, nvs, amount, l, u, codes, meta, kc=kc, ctab=ctab, lists=lists, tab_pi=pi, tab_pi0=pi0,
                                fill=fill)
        d = sp.decode_message(msg, n, nvs, amount, kc=kc, ctab=ctab)
        assert (d['count'], d['rows_used']) == (k, used)
        assert d['l'].tobytes() == l.tobytes() and d['u'].tobytes() == u.tobytes() and d['codes'].tobytes() == codes.tobytes()
        assert d['meta'].tobytes() == meta.tobytes() and d['tab_pi'].tobytes() == pi.tobytes() and d['tab_pi0'].tobytes() == pi0.tobytes()
        assert all(np.array_equal(x, y) for x, y in zip(d['lists'], lists))
        out.append(msg)
    assert out[0] != out[1]


def test_a_decoder_without_the_pad_reads_other_rows():
    """The mutant that drops the pad behind the codes moves addresses, so it is shown here and not on a GPU: with
    (n + m) % 8 != 0 a row stride of 16 n + nvs lands in the middle of the next row."""
    n, m, amount = 37, 15, 3
    nvs = n + m
    assert nvs % 8 == 4
    rng = np.random.default_rng(1)
    l, u, codes = random_rows(rng, n, nvs, amount)
    msg = sp.encode_message(n, nvs, amount, l, u, codes, rng.standard_normal((amount, 5)))
    L = sp.layout(n, nvs, amount)
    assert L.rowbytes == 16 * n + nvs + 4
    wrong = 16 * n + nvs
    row1 = np.frombuffer(msg[wrong:wrong + 8 * n], np.float64)
    assert row1.tobytes() != l[1].tobytes()
    assert np.frombuffer(msg[L.rowbytes:L.rowbytes + 8 * n], np.float64).tobytes() == l[1].tobytes()


def test_the_budget_of_a_script_ends_a_solve_with_an_exception():
    n = 4
    reply = sp.make_record(n, dual=INF)
    peer = sp.ScriptedPeer(n, [reply, lambda rec: sp.make_record(n, open_nodes=rec[2] + 1)])
    comm = peer.comm(_ffi, None)                     # a host-only communicator inside libmipx.so
    mine = sp.make_record(n, open_nodes=5, exchange=0)
    got = comm.allgather(mine)
    assert np.array_equal(got[0], mine) and np.array_equal(got[1], reply)
    assert comm.allgather(mine)[1][2] == 6           # a reply that depends on the record received
    with pytest.raises(AssertionError, match='all-gather 3 exceeds the script of 2'):
        comm.allgather(mine)
    assert len(peer.records) == 2 and sp.parse_record(peer.records[0], n)['open_nodes'] == 5
    with pytest.raises(AssertionError, match='nothing queued'):
        peer.recv(1, 16)
    assert peer.asked == [(1, 16)]
    peer.push(b'x' * 24)
    with pytest.raises(AssertionError, match='asks for 16 bytes, a donor sends 24'):
        peer.recv(1, 16)
    with pytest.raises(AssertionError, match='no script step expects'):
        peer.send(1, b'y' * 8)
    comm.close()


def test_record_round_trip():
    n = 3
    r = sp.make_record(n, primal=-2.0, dual=-3.0, open_nodes=7, stop=2, counts=(1, 2, 3, 4), x=[1, 2, 3], batch=16,
                       samples=np.arange(12.0), room=9, exchange=5, inflight_min=-2.5, region_free=11, kc=64, cut_rounds=1)
    assert len(r) == _ffi.exchange_record_len(n) == sp.record_len(n)
    assert list(r[:16]) == [-2.0, -3.0, 7, 2, 1, 2, 3, 4, 1, 5, 16, 9, -2.5, 11, 64, 1]
    p = sp.parse_record(r.tobytes(), n)
    x = p.pop('x')
    assert np.array_equal(sp.make_record(n, x=x, **p), r)


def played(case):
    for i, (rec0, want) in enumerate(zip(case.rank0, case.expect)):
        step = case.script[i]
        yield i, rec0, np.asarray(step(rec0) if callable(step) else step), want


@pytest.mark.parametrize('kw', [dict(), dict(room=3), dict(kc=64, region=1 << 14), dict(kc=8, region=1 << 14, peer_region=3),
                                dict(B=8), dict(B=1, steps=30)], ids=str)
def test_every_script_reaches_its_branch(kw):
    n = 5
    cs = sp.cases(n, x=np.arange(n, dtype=float), **kw)
    assert set(cs) == {'idle', 'merge', 'adopt', 'adopt_at_close', 'tie', 'limit', 'failure', 'gap', 'quotas', 'donor',
                       'no_move', 'receiver'}
    reasons = set()
    B = kw.get('B', 16)
    for name, case in cs.items():
        if B == 1 and name in ('quotas', 'donor', 'no_move', 'receiver', 'adopt'):
            continue        # (the exact mode, max_batch = 1, plays the idle, merge and termination scripts only)
        assert len(case.rank0) == len(case.expect) <= len(case.script)
        for i, rec0, reply, want in played(case):
            if want is None:
                assert i == len(case.script) - 1, (name, 'only the last exchange is the closing one')
                continue
            d = _ffi.exchange_decide(np.stack([rec0, reply]), n, mip_gap=1e-4)
            reason, inc, move = want
            assert (d['reason'], d['incumbent_rank']) == (reason, inc), (name, i, d)
            reasons.add(reason)
            if move is None:
                assert d['moves'] == [], (name, i, d)
            else:
                s, t = move
                pair = [sp.parse_record(rec0, n), sp.parse_record(reply, n)]
                amount = sp.hand_amount(pair[s]['open_nodes'], pair[t]['open_nodes'], pair[t]['room'])
                assert amount > 0 and d['moves'] == [(s, t, amount)], (name, i, d, amount)
    assert reasons == {0, 1, 2, 3, 4, 5}
    if B == 1:
        return
    # the amounts the GPU cases rely on
    donor = cs['donor']
    _, rec0, reply, _ = list(played(donor))[1]
    d = _ffi.exchange_decide(np.stack([rec0, reply]), n)
    assert d['moves'] == [(0, 1, min(149, kw.get('room', 1 << 20)))]
    _, rec0, reply, _ = list(played(cs['receiver']))[1]
    assert _ffi.exchange_decide(np.stack([rec0, reply]), n)['moves'] == [(1, 0, 40)]
    # the adopted incumbent travels with its solution: rank 1's, until rank 0 posts it as its own
    _, rec0, reply, _ = list(played(cs['adopt']))[0]
    assert np.array_equal(reply[16:16 + n], np.arange(n)) and reply[8] == 1.0


@pytest.mark.parametrize('seed,dip_at', [(0, None), (1, None), (2, 3), (3, 2)])
def test_merge_reference_within_the_derived_bound(seed, dip_at):
    n, K = 40, 6
    (cl, cr, tl, tr), seq, hot = sp.merge_sequences(n, seed, K=K, dip_at=dip_at)
    assert np.any(tl == 0) and np.any(tl > 1000) and len(hot) == 6
    moves = np.diff(np.stack([s[2 * n:] for s in seq]), axis=0)
    assert np.any(moves == 0) and np.all(np.diff(np.stack([s[:2 * n] for s in seq]), axis=0)[moves == 0] == 0)
    if dip_at is None:
        assert np.all(moves >= 0)
    else:       # the dip: down at dip_at, both neighbouring deltas of the dipped entries non-zero
        assert np.all(moves[dip_at - 1][hot] < 0) and np.all(moves[dip_at - 2][hot] > 0) and np.all(moves[dip_at][hot] > 0)
    fl, fr, ftl, ftr, has, merges = sp.merge_reference(cl, cr, tl, tr, seq)
    exact, times, bound = sp.merge_exact(cl, cr, tl, tr, seq)
    f64 = np.concatenate([fl, fr])
    assert np.array_equal(np.concatenate([ftl, ftr]), times)                      # times are exact
    # ... and are the table's plus the peer's LAST record, dip or not
    assert np.array_equal(times, np.concatenate([tl, tr]) + seq[-1][2 * n:].astype(np.int64))
    assert np.array_equal(has, (ftl > 0) | (ftr > 0))
    worst = 0.0
    for e in range(2 * n):
        err = abs(sp.F(float(f64[e])) - exact[e])
        assert err <= bound[e], (e, float(err), float(bound[e]))
        if bound[e] > 0:
            worst = max(worst, float(err / bound[e]))
    assert merges.max() <= K and merges.max() >= K - (1 if dip_at is not None else 0)
    print(f'merge_reference: worst |f64 - exact| / bound = {worst:.3f} (bound gamma_3k cost, k <= {merges.max()})')
    # the sum form: the same times, costs within one rounding per operation of the exact mean
    sl, sr, stl, str_, shas = sp.sum_form_reference(cl, cr, tl, tr, seq[-1])
    assert np.array_equal(np.concatenate([stl, str_]), times) and np.array_equal(shas, has)
    assert np.all(sl[stl == 0] == 0.0) and np.all(sr[str_ == 0] == 0.0)
