"""A scripted second rank for the exchange between the ranks of one search, written from include/mipx.h alone
(mipx_exchange_decide: the record; mipx_tree_set_comm: the wire format of a donation and the pseudo-cost merge).
Test infrastructure only; it imports nothing of the engine and calls none of its helpers.

  make_record / parse_record    the record of 16 + 5 n doubles a rank posts
  layout / encode_message / decode_message / table_rows / hand_amount
                                a donation's message, plain and cut mode
  ScriptedPeer                  the three callables of _ffi.Comm(ctx, 0, 2, allgather=, send=, recv=): it IS rank 1
  merge_reference / merge_exact / sum_form_reference
                                the pseudo-cost table after a sequence of exchanges
  cases(n)                      every script the GPU tests play, with a plausible record of rank 0 per exchange and the
                                decision it is meant to reach (tests/test_scripted_peer_abi.py checks them against
                                mipx_exchange_decide without a GPU)

THE BUDGET OF A SCRIPT.  A script is a finite list of L replies.  All-gather number L + 1 raises, a recv with nothing
queued raises, a send beyond the announced number raises: _ffi.Comm turns the exception into a failed callback, the
solve returns an error and the test ends with that exception.  A protocol mistake can therefore never leave the rank
under test spinning in the blocking exchange.

ERROR BOUND OF THE MERGE, derived and not tuned.  One merge of an entry is
    cost' = fl(fl(fl(cost * t) + ds) / T),   T = t + dt exact (integers below 2^31)
with u = 2^-53 three roundings, each a factor (1 + d_i), |d_i| <= u.  cost, t and ds are >= 0 (samples are costs >= 0,
and ds is the double the engine itself forms, fl(sum_others - sum_merged), taken as the recurrence's input), so no
cancellation occurs: if the computed cost carries the relative error e (against the exact rational value of the same
recurrence on the same inputs), then |computed(cost * t) + ds - exact| <= ((1 + e)(1 + u) - 1) exact, and after the
addition and the division (1 + e') <= (1 + e)(1 + u)^3.  After k merges of an entry
    |cost_f64 - cost_exact| <= ((1 + u)^(3k) - 1) cost_exact <= gamma_3k cost_exact,  gamma_j = j u / (1 - j u)
(Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Lemma 3.1).  Times are integers and exact.
"""
import collections
from fractions import Fraction as F

import numpy as np

INF = float('inf')
HEAD = 16                 # doubles in front of a record's solution
MAX_RECORDS = 4096        # node records per donation
MAX_TABLE_ROWS = 1 << 14  # cut rows per donation
U = F(1, 2 ** 53)


def record_len(n):
    return HEAD + 5 * n


def make_record(n, primal=INF, dual=-INF, open_nodes=0, stop=0, counts=(0, 0, 0, 0), x=None, batch=8, samples=None,
                room=1 << 30, has_x=None, exchange=0, inflight_min=INF, region_free=0, kc=0, cut_rounds=0):
    """A record with all 16 head fields, the solution and the 4 n pseudo-cost samples (mipx.h, mipx_exchange_decide).
    has_x defaults to 'a solution was given'."""
    r = np.zeros(record_len(n))
    r[0], r[1], r[2], r[3] = primal, dual, open_nodes, stop
    r[4:8] = counts
    r[8] = (0.0 if x is None else 1.0) if has_x is None else float(has_x)
    r[9] = exchange
    r[10] = batch
    r[11] = room
    r[12] = inflight_min
    r[13], r[14], r[15] = region_free, kc, cut_rounds
    if x is not None:
        r[HEAD:HEAD + n] = x
    if samples is not None:
        r[HEAD + n:] = samples
    return r


def parse_record(r, n):
    """The inverse of make_record: a dict of its keyword arguments (x always given, has_x explicit)."""
    r = np.frombuffer(r, np.float64) if isinstance(r, (bytes, bytearray)) else np.asarray(r, np.float64)
    assert r.shape == (record_len(n),)
    return dict(primal=float(r[0]), dual=float(r[1]), open_nodes=int(r[2]), stop=int(r[3]),
                counts=tuple(int(v) for v in r[4:8]), has_x=int(r[8]), exchange=int(r[9]), batch=int(r[10]),
                room=int(r[11]), inflight_min=float(r[12]), region_free=int(r[13]), kc=int(r[14]), cut_rounds=int(r[15]),
                x=r[HEAD:HEAD + n].copy(), samples=r[HEAD + n:].copy())


# ---- a donation's message ------------------------------------------------------------------------------------------
Layout = collections.namedtuple('Layout', 'rowbytes refs_off tab_off meta_off nmeta per bytes')


def pad8(b):
    return (b + 7) // 8 * 8


def layout(n, nvs, amount, kc=0, ctab=0):
    """Offsets and total bytes of a donation of `amount` rows; kc > 0: cut mode (nvs = n + m + kc there)."""
    rowbytes = 16 * n + pad8(nvs)
    if kc == 0:
        assert ctab == 0
        meta_off = amount * rowbytes
        nmeta = 1 + 5 * amount
        return Layout(rowbytes, None, None, meta_off, nmeta, 5, meta_off + 8 * nmeta)
    refs_off = amount * rowbytes
    tab_off = refs_off + pad8(4 * amount * (1 + kc))
    meta_off = tab_off + 8 * ctab * (n + 1)
    nmeta = 1 + 6 * amount + 1
    return Layout(rowbytes, refs_off, tab_off, meta_off, nmeta, 6, meta_off + 8 * nmeta)


def hand_amount(open_src, open_dst, room_dst):
    return min((open_src - open_dst) // 2, MAX_RECORDS, room_dst)


def table_rows(region_free, amount, kc):
    return max(0, min(int(region_free), MAX_TABLE_ROWS, amount * kc))


def encode_message(n, nvs, amount, l, u, codes, meta, kc=0, ctab=0, lists=None, tab_pi=None, tab_pi0=None,
                   count=None, rows_used=None, fill=0x5a):
    """The message of `amount` planned rows holding len(l) real records.  meta: (count, 5) or in cut mode (count, 6)
    with ncut last; codes: (count, nvs) (what lies beyond the meaningful codes is the caller's); lists: per record
    its refs (ncut of them); tab_pi / tab_pi0: the table rows used.  Every byte the format leaves unspecified is
    `fill`.  count / rows_used override the numbers written into META (for corrupt messages)."""
    L = layout(n, nvs, amount, kc, ctab)
    k = len(l)
    assert k <= amount
    buf = np.full(L.bytes, fill, np.uint8)
    for i in range(k):
        row = buf[i * L.rowbytes:(i + 1) * L.rowbytes]
        row[:8 * n] = np.frombuffer(np.ascontiguousarray(l[i], np.float64).tobytes(), np.uint8)
        row[8 * n:16 * n] = np.frombuffer(np.ascontiguousarray(u[i], np.float64).tobytes(), np.uint8)
        row[16 * n:16 * n + nvs] = np.frombuffer(np.ascontiguousarray(codes[i], np.int8).tobytes(), np.uint8)
    m = np.frombuffer(np.full(L.nmeta, np.frombuffer(bytes([fill]) * 8, np.float64)[0]).tobytes(), np.float64).copy()
    m[0] = k if count is None else count
    for i in range(k):
        m[1 + L.per * i:1 + L.per * (i + 1)] = meta[i]
    if kc:
        used = len(tab_pi0) if tab_pi0 is not None else 0
        assert used <= ctab
        m[-1] = used if rows_used is None else rows_used
        refs = np.frombuffer(buf[L.refs_off:L.refs_off + 4 * amount * (1 + kc)].tobytes(), np.int32).copy()
        for i in range(k):
            li = np.asarray(lists[i], np.int32)
            refs[i * (1 + kc)] = len(li)
            refs[i * (1 + kc) + 1:i * (1 + kc) + 1 + len(li)] = li
        buf[L.refs_off:L.refs_off + 4 * len(refs)] = np.frombuffer(refs.tobytes(), np.uint8)
        if used:
            pi = np.ascontiguousarray(tab_pi, np.float64).reshape(used, n)
            buf[L.tab_off:L.tab_off + 8 * used * n] = np.frombuffer(pi.tobytes(), np.uint8)
            o0 = L.tab_off + 8 * ctab * n
            buf[o0:o0 + 8 * used] = np.frombuffer(np.ascontiguousarray(tab_pi0, np.float64).tobytes(), np.uint8)
    buf[L.meta_off:] = np.frombuffer(m.tobytes(), np.uint8)
    return buf.tobytes()


def decode_message(msg, n, nvs, amount, kc=0, ctab=0):
    """The meaningful content of a message: dict(count, l, u, codes (count x nvs: the caller cuts them to the
    meaningful ones), meta (count x 5 | 6); cut mode: rows_used, ncut, lists (refs[:ncut] per record), tab_pi,
    tab_pi0 (rows_used rows))."""
    L = layout(n, nvs, amount, kc, ctab)
    assert len(msg) == L.bytes, (len(msg), L.bytes)
    raw = np.frombuffer(msg, np.uint8)
    m = np.frombuffer(msg[L.meta_off:], np.float64)
    count = int(m[0])
    assert m[0] == count and 0 <= count <= amount, m[0]
    rows = raw[:count * L.rowbytes].reshape(count, L.rowbytes)
    out = dict(count=count,
               l=np.frombuffer(rows[:, :8 * n].tobytes(), np.float64).reshape(count, n),
               u=np.frombuffer(rows[:, 8 * n:16 * n].tobytes(), np.float64).reshape(count, n),
               codes=np.frombuffer(rows[:, 16 * n:16 * n + nvs].tobytes(), np.int8).reshape(count, nvs),
               meta=m[1:1 + L.per * count].reshape(count, L.per).copy())
    if kc:
        used = int(m[-1])
        assert m[-1] == used and 0 <= used <= ctab, m[-1]
        refs = np.frombuffer(msg[L.refs_off:L.refs_off + 4 * amount * (1 + kc)], np.int32).reshape(amount, 1 + kc)
        ncut = refs[:count, 0].copy()
        assert np.all((ncut >= 0) & (ncut <= kc)) and np.array_equal(ncut, out['meta'][:, 5])
        out.update(rows_used=used, ncut=ncut, lists=[refs[i, 1:1 + ncut[i]].copy() for i in range(count)],
                   tab_pi=np.frombuffer(msg[L.tab_off:L.tab_off + 8 * used * n], np.float64).reshape(used, n),
                   tab_pi0=np.frombuffer(msg[L.tab_off + 8 * ctab * n:L.tab_off + 8 * ctab * n + 8 * used], np.float64))
    return out


# ---- the second rank -----------------------------------------------------------------------------------------------
class ScriptedPeer:
    """Rank 1 of a world of two, played from a script: script[i] answers all-gather number i and is a record or a
    function of the record just received.  sends: how many donations the script expects the rank under test to send.
    Logs: records (every record received, parsed lazily by the tests), sent (every message), asked ((peer, nbytes) of
    every recv)."""

    def __init__(self, n, script, sends=0):
        self.n, self.script, self.sends = n, list(script), sends
        self.records, self.replies, self.sent, self.asked = [], [], [], []
        self.queue = collections.deque()

    def push(self, msg):
        self.queue.append(bytes(msg))

    def allgather(self, data):
        i = len(self.records)
        rec = np.frombuffer(data, np.float64).copy()
        assert rec.shape == (record_len(self.n),), 'the rank posted a record of another length'
        if i >= len(self.script):
            raise AssertionError(f'scripted peer: all-gather {i + 1} exceeds the script of {len(self.script)}')
        self.records.append(rec)
        step = self.script[i]
        reply = np.ascontiguousarray(step(rec) if callable(step) else step, np.float64)
        assert reply.shape == rec.shape
        self.replies.append(reply.copy())
        return [data, reply.tobytes()]

    def send(self, peer, data):
        if len(self.sent) >= self.sends:
            raise AssertionError(f'scripted peer: a send to {peer} of {len(data)} bytes that no script step expects')
        assert peer == 1
        self.sent.append(bytes(data))

    def recv(self, peer, nbytes):
        self.asked.append((peer, nbytes))
        if not self.queue:
            raise AssertionError(f'scripted peer: recv of {nbytes} bytes from {peer} with nothing queued')
        msg = self.queue.popleft()
        if len(msg) != nbytes:
            raise AssertionError(f'scripted peer: the rank asks for {nbytes} bytes, a donor sends {len(msg)}')
        return msg

    def comm(self, ffi, ctx):
        return ffi.Comm(ctx, 0, 2, allgather=self.allgather, send=self.send, recv=self.recv)


# ---- the pseudo-cost table after a sequence of exchanges -----------------------------------------------------------
def _split(samples, n):
    s = np.asarray(samples, np.float64)
    return np.concatenate([s[:n], s[n:2 * n]]), np.concatenate([s[2 * n:3 * n], s[3 * n:]])   # sums, times over 2 n entries


def merge_reference(cost_l, cost_r, times_l, times_r, sample_seq, exact=False):
    """The device-finish path (mipx.h, the pseudo-cost merge): per exchange in order and per entry the increase since
    the highest times merged so far.  Returns (cost_l, cost_r, times_l, times_r, has, merges per entry (2 n)); with
    exact=True the costs are Fractions of the same recurrence on the same inputs (ds the double the engine forms)."""
    n = len(cost_l)
    cost = [F(float(v)) for v in np.concatenate([cost_l, cost_r])] if exact else np.concatenate([cost_l, cost_r]).astype(np.float64)
    times = np.concatenate([times_l, times_r]).astype(np.int64)
    seen_s, seen_t = np.zeros(2 * n), np.zeros(2 * n)
    merges = np.zeros(2 * n, np.int64)
    has = (np.asarray(times_l) > 0) | (np.asarray(times_r) > 0)
    for samples in sample_seq:
        s, t = _split(samples, n)
        for e in range(2 * n):
            dt = t[e] - seen_t[e]
            if not dt > 0.0:
                continue
            ds = s[e] - seen_s[e]                       # one f64 subtraction, the recurrence's input
            if exact:
                cost[e] = (cost[e] * int(times[e]) + F(float(ds))) / (int(times[e]) + int(dt))
            else:
                cost[e] = (cost[e] * np.float64(times[e]) + ds) / (np.float64(times[e]) + dt)
            times[e] += int(dt)
            seen_s[e], seen_t[e] = s[e], t[e]
            merges[e] += 1
            has[e % n] = True
    cl, cr = cost[:n], cost[n:]
    return cl, cr, times[:n].astype(np.int32), times[n:].astype(np.int32), has, merges


def gamma(k):
    return k * U / (1 - k * U)


def merge_exact(cost_l, cost_r, times_l, times_r, sample_seq):
    """(exact costs over the 2 n entries as Fractions, times, the derived bound gamma_3k * cost per entry)."""
    cl, cr, tl, tr, _, merges = merge_reference(cost_l, cost_r, times_l, times_r, sample_seq, exact=True)
    cost = list(cl) + list(cr)
    return cost, np.concatenate([tl, tr]), [gamma(3 * int(k)) * c for k, c in zip(merges, cost)]


def sum_form_reference(cost_l, cost_r, times_l, times_r, others, own=None):
    """The host path: base (the table at set_comm in sum form) + the others' samples of the LAST applied record +
    this rank's own.  Returns (cost_l, cost_r, times_l, times_r, has)."""
    n = len(cost_l)
    own = np.zeros(4 * n) if own is None else np.asarray(own, np.float64)
    others = np.asarray(others, np.float64)
    base = np.concatenate([np.asarray(cost_l, np.float64) * np.asarray(times_l, np.float64),
                           np.asarray(cost_r, np.float64) * np.asarray(times_r, np.float64),
                           np.asarray(times_l, np.float64), np.asarray(times_r, np.float64)])
    tot = (base + others) + own
    out = []
    for d in (0, 1):
        s, t = tot[d * n:(d + 1) * n], tot[(2 + d) * n:(3 + d) * n]
        out.append(np.where(t > 0, s / np.where(t > 0, t, 1.0), 0.0))
    tl, tr = tot[2 * n:3 * n], tot[3 * n:]
    return out[0], out[1], tl.astype(np.int32), tr.astype(np.int32), (tl > 0) | (tr > 0)


def merge_sequences(n, seed, K=6, dip_at=None):
    """A seeded table and K cumulative sample records of a peer: entries absent and entries with times in the
    thousands in the table; samples that do not move between two exchanges, entries on one side only, dyadic and
    non-dyadic sums.  dip_at = k: record k falls back to record k - 2's values on a few entries that moved in
    exchange k - 1 and move again in k + 1 (both neighbouring deltas non-zero), and recovers."""
    rng = np.random.default_rng(seed)
    tl = np.where(rng.random(n) < .4, 0, rng.integers(1, 5000, n)).astype(np.int32)
    tr = np.where(rng.random(n) < .4, 0, rng.integers(1, 5000, n)).astype(np.int32)
    cl = np.where(tl > 0, rng.random(n) * 3, 0.0)
    cr = np.where(tr > 0, np.round(rng.random(n) * 64) / 16, 0.0)
    left_only, right_only = rng.random(n) < .15, rng.random(n) < .15
    dyadic = rng.random(2 * n) < .3
    hot = np.zeros(2 * n, bool)
    hot[rng.choice(2 * n, 6, replace=False)] = True        # entries that move at every exchange
    s, t = np.zeros(2 * n), np.zeros(2 * n)
    seq = []
    for k in range(K):
        move = rng.random(2 * n) < .5
        move[:n] &= ~right_only
        move[n:] &= ~left_only
        move |= hot
        dt = np.where(move, rng.integers(1, 9, 2 * n), 0).astype(np.float64)
        per = np.where(dyadic, rng.integers(0, 33, 2 * n) / 8.0, rng.random(2 * n) * 2.5)
        s = s + dt * per
        t = t + dt
        seq.append(np.concatenate([s, t]))
    if dip_at is not None:
        assert 2 <= dip_at < K - 1
        dipped = seq[dip_at].copy()
        idx = np.where(hot)[0]
        for e in idx:
            dipped[e], dipped[2 * n + e] = seq[dip_at - 2][e], seq[dip_at - 2][2 * n + e]
        seq[dip_at] = dipped
    return (cl, cr, tl, tr), seq, np.where(hot)[0]


# ---- the scripts of the GPU tests ----------------------------------------------------------------------------------
Case = collections.namedtuple('Case', 'script sends rank0 expect')
"""script: the replies, one per all-gather (len(script) is the number of all-gathers the case pins); sends: donations
the rank under test is expected to send; rank0: a plausible record of rank 0 per exchange; expect: per exchange
(reason, incumbent rank, None | (from, to)) the decision is meant to reach -- the amount of a move is the hand
formula on the two records -- or None for the closing exchange (merge and adoption only, no decision)."""


def calm(**change):
    """A reply that neither ends the search nor moves a node whatever the rank under test posted: the rank's own dual
    bound, no incumbent, as many open nodes as its frontier batch (not short of a batch, so it receives nothing;
    not two batches, so it donates nothing), the rank's cut fields.  `change` overrides fields; a value may be a
    function of the parsed record."""
    def reply(rec):
        n = (len(rec) - HEAD) // 5
        p = parse_record(rec, n)
        kw = dict(primal=INF, dual=p['dual'], open_nodes=max(1, p['batch']), batch=max(1, p['batch']), room=1 << 20,
                  region_free=p['region_free'], kc=p['kc'], cut_rounds=p['cut_rounds'])
        kw.update({k: (v(p) if callable(v) else v) for k, v in change.items()})
        return make_record(n, **kw)
    return reply


def cases(n, B=16, opt=-7.0, x=None, room=1 << 20, samples=None, kc=0, region=0, peer_region=1 << 14, open0=300,
          few=3, take=40, steps=12):
    """name -> Case.  opt / x: the optimum a test posts as the peer's incumbent; samples: the cumulative sample
    records of the merge test; room: the pool rows the PEER reports ([11]); kc / region / peer_region: cut mode
    (rank 0's and the peer's [13]); open0 / few: the open nodes rank 0 plausibly reports as donor / as receiver;
    take: the records the receiver is to be given; steps: the step quota of the searches that run."""
    x = np.zeros(n) if x is None else np.asarray(x, np.float64)
    samples = [np.zeros(4 * n)] * 6 if samples is None else samples
    K = len(samples)
    cut = dict(kc=kc, cut_rounds=1 if kc else 0)
    mine = dict(batch=B, room=1 << 14, region_free=region, **cut)          # rank 0's side of a plausible record
    busy0 = make_record(n, dual=opt - 1.0, open_nodes=open0, inflight_min=opt - 1.0, **mine)
    quota0 = make_record(n, dual=opt - 1.0, open_nodes=open0, stop=2, **mine)
    dry0 = make_record(n, dual=INF, open_nodes=0, **mine)
    few0 = make_record(n, dual=opt - 1.0, open_nodes=few, stop=2, **mine)
    closed0 = make_record(n, primal=opt, dual=opt, open_nodes=0, x=x, **mine)
    out = {}
    go, stop, close = (0, -1, None), (4, -1, None), None

    # 4.1: an idle peer, an exchange at every step, the rank stops at its step quota
    idle = make_record(n, dual=INF, batch=B, room=0, **cut)        # (room 0: an idle peer with room would be fed)
    out['idle'] = Case([idle] * (steps + 8), 0, [busy0] * (steps + 6) + [quota0, quota0],
                       [go] * (steps + 6) + [stop, close])
    # 4.2: the rank is dry and blocks; K records of samples, the idle record that ends the search, the closing one
    work = [make_record(n, dual=opt - 1.0, open_nodes=1, batch=B, samples=s, **cut) for s in samples]
    tail = make_record(n, dual=INF, batch=B, samples=samples[-1], **cut)
    out['merge'] = Case(work + [tail, tail], 0, [dry0] * (K + 2), [go] * K + [(1, -1, None), close])
    # 4.3
    inc = make_record(n, primal=opt, dual=INF, open_nodes=0, batch=B, room=0, x=x, **cut)
    has0 = make_record(n, primal=opt, dual=opt - .5, open_nodes=open0, x=x, inflight_min=opt - .5, **mine)
    out['adopt'] = Case([inc] * 400, 0, [busy0, has0], [(0, 1, None), (0, 0, None)])      # a search that closes
    out['adopt_at_close'] = Case([idle, inc], 0, [dry0, dry0], [(1, -1, None), close])
    tie = make_record(n, primal=opt, dual=INF, open_nodes=0, batch=B, room=0, has_x=0, x=np.full(n, 7.0), **cut)
    out['tie'] = Case([tie, tie], 0, [closed0, closed0], [(1, 0, None), close])
    working = make_record(n, dual=opt - 1.0, open_nodes=1, batch=B, **cut)
    # (the closing record repeats the flag and the node: a peer stopped by a limit still holds its open nodes)
    out['limit'] = Case([working, calm(stop=1, open_nodes=1), calm(stop=1, open_nodes=1)], 0, [dry0] * 3,
                        [go, (2, -1, None), close])
    out['failure'] = Case([working, calm(stop=3, open_nodes=1), calm(stop=3, open_nodes=1)], 0, [dry0] * 3,
                          [go, (5, -1, None), close])
    low = make_record(n, dual=opt - 1.0, open_nodes=1, batch=B, **cut)
    risen = make_record(n, dual=opt, open_nodes=1, batch=B, **cut)
    out['gap'] = Case([low, low, risen, risen], 0, [closed0] * 4, [(0, 0, None), (0, 0, None), (3, 0, None), close])
    out['quotas'] = Case([calm(), calm(stop=2), calm(stop=2)], 0, [busy0, quota0, quota0], [go, stop, close])
    # 4.4: the donor at its step quota; the peer has one node and room for `room`
    need = make_record(n, dual=opt - 1.0, open_nodes=1, batch=B, room=room, region_free=peer_region, **cut)
    done = calm(stop=2)
    out['donor'] = Case([calm(), need, done, done], 1, [busy0, quota0, quota0, quota0],
                        [go, (0, -1, (0, 1)), stop, close])
    same = calm(open_nodes=lambda p: p['open_nodes'])
    out['no_move'] = Case([calm(), same, done, done], 0, [busy0, quota0, quota0, quota0], [go, go, stop, close])
    # 4.5: the receiver at its step quota with a few nodes of its own; the peer has 2 take + its few + 1
    rich = calm(open_nodes=lambda p: p['open_nodes'] + 2 * take + 1)
    out['receiver'] = Case([calm(), rich, done, done], 0, [few0, few0, few0, few0], [go, (0, -1, (1, 0)), stop, close])
    return out


