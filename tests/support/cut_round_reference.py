"""A plain restatement of one cut round of a batch of nodes, and seeded synthetic rounds to run it on.

gather(s), begin(s) and generate(s, oracle) say what the six kernels of a round must leave behind
(cut_gather_state, cut_round_begin, K2 in its slab form, pool_append, K3 over the pool lists, cut_round_apply), node by
node, as BaseNode._base_bound's loop does it: nodes/base_node.py:196-203 (who goes on generating), :292-341 (the stall
test and the removal of the cut rows with a zero dual) and :456-463 (the selected cuts become rows, leave the pool),
with the GMI cuts and the selection themselves taken from the oracle (oracle.gomory_from_dump on the node's materialised
rows, oracle.select_cuts on its pool in pool order).  It is written from those lines and from the comments of
csrc/tree_kernels.hip.h, not from the kernels, which must give the same bytes (tests/test_cut_round_kernels_gpu.py
through the two entries of include/mipx_cutround.h).  Test infrastructure only.

A round: B nodes.  Node k has the m0 shared rows and ncut[k] <= kc cut rows, row i of them being row ids[k, i] of the
cut store; ms = m0 + kc rows are allotted per node in vstat (B x (n + ms)), y (B x ms), T (B x ms x n) and idx
(B x (2 n + ms): nvar | bvar | side).  state is FIELDS x B.  A node's candidate cuts live in its slab (slab_rows rows);
the rows below state[slab_n] are taken, pool_list[k, :state[pool_n]] are the rows still in the pool, in pool order.

What the kernels leave as it was, said here and pinned by the tests:
  - the entries of ids and vstat past a node's new ncut (begin compacts in place, apply appends);
  - the slab rows past slab_n, the store rows nobody was given, pool_list past the old pool_n;
  - pool_list[new pool_n : old pool_n]: the in-place compaction leaves there what the marked list held (-1 at a
    selected position, the old entry elsewhere);
  - everything of a node with active == 0 in generate, and counters[1], counters[2] in begin.

The one thing that is not a function of the inputs: with B > 1 the store ids are taken by atomicAdd across
workgroups.  generate hands them out node by node (ONE valid order); `per_node` of its result holds what a test
compares through the ids instead (the rows each node selected, in order, and how many of them its list had room for).
"""
import collections
import math

import numpy as np

FIELDS = ('rounds', 'it_created', 'n_created', 'it_added', 'n_added', 'it_removed', 'n_removed', 'ncut_out', 'stalled',
          'pool_n', 'slab_n', 'dropped')
F = {name: i for i, name in enumerate(FIELDS)}
INF = float('inf')
TOL = 1e-4                       # progress tolerance of the begin cases (base_node.py:292)
# (before, objective) whose relative change |before - obj| / |before| is, as computed, exactly the double below TOL, TOL
# itself and the double above it (found by search; begin() counts them as change_ulp_below_tol / at / above)
AROUND_TOL = dict(tol_below=('0x1.a69b64e054691p+5', '0x1.a6a636793c40ap+5'), tol_at=('0x1.018bcdfefbf40p+3', '0x1.019265d9a8c74p+3'),
                  tol_above=('0x1.0c38e4b87bdcfp+3', '0x1.0c3fc28ababfcp+3'))
BOUND = 100.0                    # max_dual_bound of the begin cases
STALE_SLAB = -3.5                # every entry of a slab row nobody has written
STALE_STORE = -1.25              # ... of a store row nobody was given
STALE_LIST = -9                  # ... of pool_list past pool_n
STALE_ID = 12345                 # ... of ids past ncut
STALE_CODE = 9                   # ... of vstat past the node's rows
VAR_EPS, GOOD_EPS = 1e-4, 1e-2   # tolerance.py:2, :5


def lp_feasible(st):
    return st in (0, 2)


# ---- cut_gather_state --------------------------------------------------------------------------------------------
def gather(s):
    """The working copies of the nodes' cut lists at the start of a step: ncut and the first ncut ids from the pool rows
    slot[k], the state zeroed, counters[2] raised to the largest ncut.  Returns the new ncut, ids, state, counters."""
    B, kc = s['B'], s['kc']
    ncut, ids = np.array(s['ncut'], np.int32), np.array(s['ids'], np.int32).reshape(B, kc)
    counters = np.array(s['counters'], np.int32)
    for k in range(B):
        row = int(s['slot'][k])
        nc = int(s['pool_ncut'][row])
        ncut[k] = nc
        ids[k, :nc] = np.asarray(s['pool_ids']).reshape(-1, kc)[row, :nc]
        counters[2] = max(int(counters[2]), nc)
    return dict(ncut=ncut, ids=ids, state=np.zeros((len(FIELDS), B), np.int32), counters=counters)


# ---- cut_round_begin ---------------------------------------------------------------------------------------------
def begin(s):
    """gather (with s['gather']), then per node: the stall test of the round before (base_node.py:320-324, only for a
    node that generated in it), the loop condition (:196-203), and for a node that goes on: the round counted, the
    objective remembered, the cut rows whose dual is exactly 0 removed (:326-341; -0.0 is 0, NaN is not)."""
    n, m0, kc, B = s['n'], s['m0'], s['kc'], s['B']
    ms = m0 + kc
    paths = collections.Counter()
    w = dict(vstat=np.array(s['vstat'], np.int8).reshape(B, n + ms), ncut=np.array(s['ncut'], np.int32),
             ids=np.array(s['ids'], np.int32).reshape(B, kc), state=np.array(s['state'], np.int32).reshape(len(FIELDS), B),
             obj_before=np.array(s['obj_before'], np.float64), active=np.array(s['active'], np.int32),
             counters=np.array(s['counters'], np.int32), resolve=np.zeros(B, np.int32), need_tab=np.zeros(B, np.int32))
    if s['gather']:
        w.update(gather(s))
        paths['gather'] += 1
        paths['gather_scattered'] += bool(np.any(np.diff(s['slot']) < 0))
        paths['gather_largest_last'] += bool(B > 1 and w['ncut'][-1] > w['ncut'][:-1].max())
    st = w['state']
    y = np.asarray(s['y'], np.float64).reshape(B, ms)
    for k in range(B):
        status = int(s['status'][k])
        paths['status_%d' % status] += 1
        feas = lp_feasible(status)
        obj = np.float64(s['obj'][k]) if feas else np.float64(INF)
        stalled = int(st[F['stalled'], k])
        paths['stalled_on_entry'] += stalled
        if s['round'] > 0:
            paths['was_inactive' if not s['active'][k] else 'was_active'] += 1
        if s['round'] > 0 and s['active'][k]:
            before = np.float64(s['obj_before'][k])
            with np.errstate(all='ignore'):
                change = np.abs(before - obj) / np.abs(before)       # 0 / 0: nan, x / 0: inf -- neither is < tol
                if before == 0:
                    paths['zero_over_zero' if obj == 0 else 'x_over_zero'] += 1
                elif obj == INF:
                    paths['objective_inf'] += 1
                elif change == s['progress_tol']:
                    paths['change_at_tol'] += 1
                elif change == np.nextafter(s['progress_tol'], 0.0):
                    paths['change_ulp_below_tol'] += 1
                elif change == np.nextafter(s['progress_tol'], 1.0):
                    paths['change_ulp_above_tol'] += 1
                if change < s['progress_tol']:
                    stalled = 1
                    paths['stalls_now'] += 1
        rounds = int(st[F['rounds'], k])
        if rounds == s['max_rounds']:
            paths['rounds_at_max'] += 1
        elif rounds == s['max_rounds'] - 1:
            paths['rounds_one_below_max'] += 1
        if feas and obj == s['max_dual_bound']:
            paths['obj_at_bound'] += 1
        elif feas and obj == np.nextafter(s['max_dual_bound'], -INF):
            paths['obj_ulp_below_bound'] += 1
        paths['mip_feasible'] += bool(s['mipf'][k])
        act = bool(feas and not s['mipf'][k] and not stalled and rounds < s['max_rounds'] and obj < s['max_dual_bound'])
        nc, nrem = int(w['ncut'][k]), 0
        if act:
            duals = y[k, m0:m0 + nc]
            gone = duals == 0.0
            keep = ~gone
            nrem = int(gone.sum())
            kept = nc - nrem
            w['ids'][k, :kept] = w['ids'][k, :nc][keep].copy()           # (the tails stay as they were)
            w['vstat'][k, n + m0:n + m0 + kept] = w['vstat'][k, n + m0:n + m0 + nc][keep].copy()
            paths['ncut_%d' % nc] += 1
            if nc == kc:
                paths['list_full_kc%d' % kc] += 1
            if nc:
                pattern = ('none' if nrem == 0 else 'all' if nrem == nc else
                           'first_only' if nrem == 1 and gone[0] else 'last_only' if nrem == 1 and gone[-1] else
                           'alternating' if nc >= 4 and (np.array_equal(gone, np.arange(nc) % 2 == 0) or
                                                         np.array_equal(gone, np.arange(nc) % 2 == 1)) else 'mixed')
                paths['remove_' + pattern] += 1
                if nc == 64 and gone[63]:
                    paths['remove_lane_63'] += 1
                paths['dual_negative_zero'] += bool(np.any(gone & np.signbit(duals)))
                paths['dual_subnormal_kept'] += bool(np.any(keep & (np.abs(duals) < np.finfo(np.float64).tiny) & (duals != 0)))
                paths['dual_nan_kept'] += bool(np.any(keep & np.isnan(duals)))
            st[F['rounds'], k] = rounds + 1
            w['obj_before'][k] = obj
            w['ncut'][k] = kept
            if nrem:
                st[F['it_removed'], k] += 1
                st[F['n_removed'], k] += nrem
            w['counters'][0] += 1
        st[F['stalled'], k] = stalled
        w['active'][k] = int(act)
        w['resolve'][k] = int(act and nrem > 0)
        tab = int(act and (nrem > 0 or not s['have_dump']))
        if tab:
            paths['tableau_after_removal' if nrem else 'tableau_without_dump'] += 1
        w['need_tab'][k] = tab
        w['counters'][3] += tab
    w['paths'] = paths
    return w


# ---- K2, pool_append, K3, cut_round_apply ------------------------------------------------------------------------
def count_cuts(n, bvar, x, is_int):
    """How many GMI cuts a basis gives (base_node.py:468-480): one per basic integer structural whose value, clipped at
    0, is fractional by more than variable_epsilon with a fractional part in [0.01, 0.99]."""
    made = 0
    for v in bvar:
        if v < n and is_int[v]:
            xv = max(float(x[v]), 0.0)
            fl, ce = math.floor(xv), math.ceil(xv)
            f0 = xv - fl
            made += min(xv - fl, ce - xv) > VAR_EPS and not (f0 < GOOD_EPS or f0 + GOOD_EPS > 1.0)
    return made


def support(row):
    return int(np.sum(np.abs(row) > GOOD_EPS))


def generate(s, oracle):
    """The second half of a round.  Returns the arrays as they must be afterwards (store ids handed out node by node),
    per_node (what to compare through the ids) and paths."""
    A, b = np.asarray(s['A'], np.float64), np.asarray(s['b'], np.float64)
    m0, n = A.shape
    B, kc, SR, cap = s['B'], s['kc'], s['slab_rows'], s['store_cap']
    ms = m0 + kc
    paths = collections.Counter()
    w = {k: np.array(s[k]) for k in ('vstat', 'ncut', 'ids', 'state', 'pool_list', 'slab_pi', 'slab_pi0', 'store_pi', 'store_pi0',
                                     'store_count', 'resolve', 'counters')}
    w.update(k2_ncuts=[None] * B, k3_nadded=[None] * B, k3_added=[None] * B, k3_term=[None] * B)
    st = w['state']
    int_idx = np.flatnonzero(s['is_int'])
    count0 = int(s['store_count'][0])
    per_node = []
    paths['n_odd' if n % 2 else 'n_even'] += 1
    paths['n_plus_ms_odd' if (n + ms) % 2 else 'n_plus_ms_even'] += 1
    for k in range(B):
        if not s['active'][k]:
            paths['inactive'] += 1
            per_node.append(None)
            continue
        nc0 = int(s['ncut'][k])
        mk = m0 + nc0
        paths['cut_rows' if nc0 else 'no_cut_rows'] += 1
        # 1. the node's LP rows: the shared ones, then its cuts (base_node.py:602-606 keeps them in list order)
        ids = np.asarray(s['ids'][k][:nc0], int)
        rows = np.vstack([A, np.asarray(s['store_pi'])[ids]]) if nc0 else A
        rhs = np.concatenate([b, np.asarray(s['store_pi0'])[ids]]) if nc0 else b
        # 2. GMI cuts of the dumped tableau; a basis that is not square has no tableau (base_node.py:518-519)
        x = np.asarray(s['x'][k], np.float64)
        vs = np.asarray(s['vstat'][k])
        if int(np.sum(vs[:n + mk] == 1)) != mk:
            paths['not_square'] += 1
            new_pi, new_pi0 = np.zeros((0, n)), np.zeros(0)
        else:
            idx = np.asarray(s['idx'][k])
            dump = dict(T=np.asarray(s['T'][k][:mk], np.float64), nvar=idx[:n], bvar=idx[n:n + mk])
            g = oracle.gomory_from_dump(rows, rhs, dump, x, int_idx, s['max_term'])
            new_pi, new_pi0 = g['safe_pi'], g['safe_pi0']
            assert len(new_pi0) == count_cuts(n, idx[n:n + mk], x, s['is_int'])
            m2 = 1 << max(mk - 1, 0).bit_length()
            if len(new_pi0):
                paths['fold_rows_%d' % mk] += 1
                paths['fold_le_64' if m2 <= 64 else 'fold_1024' if m2 == 1024 else 'fold_gt_64'] += 1
        made = len(new_pi0)
        w['k2_ncuts'][k] = made
        # 3. into the slab behind the rows taken; what does not fit is dropped
        base, pn = int(st[F['slab_n'], k]), int(st[F['pool_n'], k])
        kept = min(made, SR - base)
        w['slab_pi'][k, base:base + kept] = new_pi[:kept]
        w['slab_pi0'][k, base:base + kept] = new_pi0[:kept]
        if made:
            paths['slab_already_full' if base == SR else 'slab_exact_fit' if base + made == SR else
                  'slab_overflow_by_%d' % (base + made - SR) if base + made > SR else 'slab_room'] += 1
        # 4. ... and the pool, in row order (cut_pool = {**old, **new}, base_node.py:306); counted as created (:383)
        w['pool_list'][k, pn:pn + kept] = base + np.arange(kept)
        pn += kept
        st[F['slab_n'], k] = base + kept
        st[F['dropped'], k] += made - kept
        if made:
            st[F['it_created'], k] += 1
            st[F['n_created'], k] += made
        # 5. selection over the pool in pool order, x clipped at 0 (base_node.py:310, :387-454)
        plist = w['pool_list'][k, :pn].copy()
        if np.any(plist != np.arange(pn)):
            paths['pool_with_holes'] += 1
        P, P0 = w['slab_pi'][k][plist], w['slab_pi0'][k][plist]
        added, term, depth = oracle.select_cuts(P, P0, np.maximum(x, 0.0), s['max_nonzero_coefs'], s['min_cut_depth'],
                                                s['cos_parallel'], s['max_abs_coef'])
        added = [int(a) for a in added]
        nadd = len(added)
        w['k3_nadded'][k], w['k3_added'][k], w['k3_term'][k] = nadd, added, term
        paths['terminator_%d' % term] += 1
        paths['pool_empty'] += pn == 0
        paths['pool_of_2040'] += pn == 2040
        sup = [support(r) for r in P]
        paths['empty_support_row'] += any(v == 0 for v in sup)
        paths['support_above_limit'] += any(v > s['max_nonzero_coefs'] for v in sup)
        deep = [q for q in range(pn) if 0 < sup[q] <= s['max_nonzero_coefs'] and depth[q] < -s['min_cut_depth']]
        paths['rejected_large_coefficient'] += any(np.max(np.abs(P[q])) > s['max_abs_coef'] for q in deep)
        paths['rejected_parallel'] += any(q not in added and np.max(np.abs(P[q])) <= s['max_abs_coef'] for q in deep)
        if nadd and pn > 1:
            paths['selects_all' if nadd == pn else 'selects_first_only' if added == [0] else
                  'selects_last_only' if added == [pn - 1] else 'selects_some'] += 1
        # 6. the selection becomes rows (base_node.py:456-463): a store entry, the node's list, the slack basic
        nc, taken = nc0, 0
        room_list = kc - nc0
        for a in added:
            if nc >= kc:
                continue                                   # the list is full: no store entry is asked for
            cid = int(w['store_count'][0])
            w['store_count'][0] += 1
            if cid >= cap:
                continue                                   # the store is full: the entry is lost
            w['store_pi'][cid], w['store_pi0'][cid] = P[a], P0[a]
            w['ids'][k, nc] = cid
            w['vstat'][k, n + m0 + nc] = 1
            nc += 1
            taken += 1
        if nadd:
            paths['list_room_0' if room_list == 0 else 'list_room_exact' if room_list == nadd else
                  'list_room_short_%d' % room_list if room_list < nadd else 'list_room'] += 1
        # ... and leaves the pool, which keeps its order (del self.cut_pool[idx]) -- whether or not there was room
        marked = w['pool_list'][k].copy()
        if nadd:
            marked[added] = -1
        rest = marked[:pn][marked[:pn] >= 0]
        marked[:len(rest)] = rest
        w['pool_list'][k] = marked
        st[F['pool_n'], k] = len(rest)
        w['ncut'][k] = nc
        st[F['ncut_out'], k] = nc
        if nadd:
            st[F['it_added'], k] += 1
            st[F['n_added'], k] += nadd                    # (the selection, including what was then dropped)
        st[F['dropped'], k] += nadd - taken
        changed = int(bool(s['resolve'][k]) or taken > 0)
        paths['resolve_set_on_entry'] += bool(s['resolve'][k])
        w['resolve'][k] = changed
        w['counters'][1] += changed
        w['counters'][2] = max(int(w['counters'][2]), nc)
        per_node.append(dict(nc0=nc0, selected_pi=P[added] if nadd else np.zeros((0, n)), selected_pi0=P0[added] if nadd else np.zeros(0),
                             wanted=min(nadd, room_list), nadd=nadd, k2_dropped=made - kept, resolve_in=int(bool(s['resolve'][k]))))
    attempts = int(w['store_count'][0]) - count0
    room = max(cap - count0, 0)
    if attempts:
        paths['store_room_0' if room == 0 else 'store_room_exact' if room == attempts else
              'store_room_short_%d' % room if room < attempts else 'store_room'] += 1
    w.update(per_node=per_node, paths=paths, attempts=attempts, store_room=room)
    return w


# ---- seeded rounds: begin ----------------------------------------------------------------------------------------
PATTERNS = ('none', 'all', 'first', 'last', 'alternating', 'negzero', 'subnormal', 'nan')
KINDS0 = ('status1', 'status2', 'status3', 'mipf', 'stalled', 'rounds_max', 'rounds_max_1', 'obj_at_bound', 'obj_below_bound')
KINDS1 = ('tol_below', 'tol_at', 'tol_above', 'zero_zero', 'zero_x', 'obj_inf', 'was_inactive')
MAX_ROUNDS = 10


def _begin_round(B, kc, rnd, have_dump, gather, offset, seed, n=5, m0=3):
    """Even nodes generate, with the removal patterns and list lengths in turn; odd nodes take the kinds that stop a
    node (and with round > 0 every node one of the stall-test kinds) in turn."""
    rng = np.random.default_rng(seed)
    ms = m0 + kc
    lengths = (0, 1, 63, 64) if kc == 64 else (kc, max(kc - 2, 0))
    s = dict(n=n, m0=m0, kc=kc, B=B, round=rnd, max_rounds=MAX_ROUNDS, progress_tol=TOL, max_dual_bound=BOUND, have_dump=have_dump,
             gather=gather)
    s['status'] = np.zeros(B, np.int32)
    s['obj'] = np.round(rng.uniform(1.0, 50.0, B), 3)
    s['mipf'] = np.zeros(B, np.int32)
    s['y'] = rng.uniform(0.5, 2.0, (B, ms)) * rng.choice([-1.0, 1.0], (B, ms))
    s['vstat'] = rng.integers(0, 4, (B, n + ms)).astype(np.int8)
    s['ncut'] = np.zeros(B, np.int32)
    s['ids'] = rng.integers(0, 1000, (B, kc)).astype(np.int32)
    s['state'] = rng.integers(0, 5, (len(FIELDS), B)).astype(np.int32)
    s['state'][F['stalled']] = 0
    s['obj_before'] = np.round(rng.uniform(51.0, 90.0, B), 3)
    s['active'] = np.ones(B, np.int32) if rnd > 0 else np.full(B, 7, np.int32)      # (round 0 does not read it)
    s['counters'] = np.array([3, 5, 2, 9], np.int32)                                # (they accumulate)
    for k in range(B):
        j = k + offset
        combo = j // 2 if j % 2 == 0 else j
        nc = lengths[combo % len(lengths)]
        pattern = PATTERNS[(combo // len(lengths)) % len(PATTERNS)]
        s['ncut'][k] = nc
        d = s['y'][k, m0:]
        if pattern == 'all':
            d[:nc] = 0.0
        elif pattern == 'first' and nc:
            d[0] = 0.0
        elif pattern == 'last' and nc:
            d[nc - 1] = 0.0
        elif pattern == 'alternating':
            d[j % 2:nc:2] = 0.0
        elif pattern == 'negzero' and nc:
            d[nc // 2] = -0.0
        elif pattern == 'subnormal' and nc:
            d[nc // 2] = 5e-324
        elif pattern == 'nan' and nc:
            d[nc // 2] = np.nan
        if rnd > 0:
            kind = KINDS1[(j // 2) % len(KINDS1)]
            if kind == 'was_inactive':
                s['active'][k] = 0
                s['obj_before'][k], s['obj'][k] = 4.0, 4.0          # (would stall, were it tested)
            elif kind.startswith('tol'):
                s['obj_before'][k], s['obj'][k] = (float.fromhex(h) for h in AROUND_TOL[kind])
            elif kind == 'zero_zero':
                s['obj_before'][k], s['obj'][k] = 0.0, 0.0
            elif kind == 'zero_x':
                s['obj_before'][k] = 0.0
            elif kind == 'obj_inf':
                s['obj'][k] = INF
        if j % 2 == 1:
            kind = KINDS0[(j // 2) % len(KINDS0)]
            if kind in ('status1', 'status3'):
                s['status'][k], s['obj'][k] = int(kind[-1]), np.nan     # (the objective is not read)
            elif kind == 'status2':
                s['status'][k] = 2
            elif kind == 'mipf':
                s['mipf'][k] = 1
            elif kind == 'stalled':
                s['state'][F['stalled'], k] = 1
            elif kind == 'rounds_max':
                s['state'][F['rounds'], k] = MAX_ROUNDS
            elif kind == 'rounds_max_1':
                s['state'][F['rounds'], k] = MAX_ROUNDS - 1
            elif kind == 'obj_at_bound':
                s['obj'][k] = BOUND
            elif kind == 'obj_below_bound':
                s['obj'][k] = np.nextafter(BOUND, -INF)
    if gather:
        # the lists come from scattered pool rows; the dense copies a caller sends are overwritten
        rows = 3 * B + 2
        s['slot'] = rng.permutation(rows)[:B].astype(np.int32)
        s['pool_ncut'] = rng.integers(0, kc + 1, rows).astype(np.int32)
        s['pool_ids'] = rng.integers(2000, 3000, (rows, kc)).astype(np.int32)
        s['pool_ncut'][s['slot']] = s['ncut']
        for k in range(B):
            s['pool_ids'][s['slot'][k], :s['ncut'][k]] = s['ids'][k, :s['ncut'][k]]
        s['ncut'] = np.full(B, 1, np.int32)
        s['ids'] = np.full((B, kc), STALE_ID, np.int32)
        s['state'] = np.full((len(FIELDS), B), 3, np.int32)
    return s


def _gather_last_largest():
    s = _begin_round(5, 64, 0, 1, 1, 0, 77)
    lengths = np.array([3, 0, 7, 1, 64], np.int32)
    s['slot'] = np.array([11, 2, 16, 0, 5], np.int32)           # neither ascending nor descending
    s['pool_ncut'][s['slot']] = lengths
    s['counters'][2] = 10                                        # below the last node's 64, above every other
    return s


CASES = {}
for _B in (1, 5, 70):
    for _kc in (64, 5):
        for _rnd in (0, 2):
            for _mode in ((1, 0), (0, 0), (1, 1)):                  # (have_dump, gather)
                if _mode[1] and _rnd:
                    continue                                        # (the lists are gathered at the start of a step)
                for _off in ((0, 2, 6, 13, 14, 30, 38, 46, 54, 62) if _B == 1 and _kc == 64 and _mode == (1, 0) else (0,) if _B == 70 else (0, 9)):
                    _name = 'begin-B%d-kc%d-round%d-dump%d-gather%d-off%d' % (_B, _kc, _rnd, _mode[0], _mode[1], _off)
                    CASES[_name] = ('begin', (_B, _kc, _rnd, _mode[0], _mode[1], _off, len(CASES) + 1))
CASES['begin-gather-largest-last'] = ('begin', None)


# ---- seeded rounds: generate -------------------------------------------------------------------------------------
DEFAULTS = dict(chunks=0, group=0, max_term=1e3, min_cut_depth=1e-8, cos_parallel=math.cos(math.radians(10.0)), max_abs_coef=1e6)
FRACTIONS = (0.5, 0.25, 0.75, 0.125, 0.3, 0.62, 0.0099, 0.01, 0.0101, 0.99, 0.9901, 0.9899, 0.00005, 0.0)


def _problem(rng, n, m):
    A = -rng.integers(0, 11, (m, n)).astype(np.float64)
    b = -rng.integers(n, 4 * n + 1, m).astype(np.float64)
    is_int = (rng.random(n) < 0.7).astype(np.uint8)
    return A, b, is_int


def _tableau(rng, n, mk, ms, is_int, square=True):
    """Any split of the n + mk variables into nvar and bvar with a basis code of 1 exactly on bvar is a state K2 can be
    given: it reads T, the split, x and the rows, never how a solve got there."""
    perm = rng.permutation(n + mk)
    idx = np.full(2 * n + ms, -5, np.int32)
    idx[:n + mk] = perm
    idx[n + ms:] = rng.integers(0, 2, n)
    kinds = rng.integers(0, 5, (mk, n))
    T = np.where(kinds == 0, 0.0, np.where(kinds == 1, rng.integers(-3, 4, (mk, n)).astype(np.float64),
                 np.where(kinds == 2, rng.integers(-24, 25, (mk, n)) / 8.0, rng.normal(0.0, 1.5, (mk, n)))))
    T = np.vstack([T, np.full((ms - mk, n), np.nan)])            # (rows the node does not have: never read)
    vstat = np.full(n + ms, STALE_CODE, np.int8)
    vstat[:n + mk] = rng.choice([0, 2, 3], n + mk)
    vstat[perm[n:]] = 1
    if not square:
        vstat[perm[0]] = 1
    x = rng.integers(0, 6, n) + rng.choice(FRACTIONS, n)
    x[rng.random(n) < 0.05] *= -1.0                              # (read as 0)
    return T, idx, vstat, x


def _blank(n, m, kc, B, seed, lengths, slab_rows, store_used=40, store_room=1000, active=None, square=None, **over):
    rng = np.random.default_rng(seed)
    A, b, is_int = _problem(rng, n, m)
    ms = m + kc
    s = dict(DEFAULTS, A=A, b=b, is_int=is_int, B=B, kc=kc, slab_rows=slab_rows, max_nonzero_coefs=n)
    cap = store_used + store_room
    s['store_cap'] = cap
    s['store_pi'] = np.full((cap, n), STALE_STORE)
    s['store_pi0'] = np.full(cap, STALE_STORE)
    s['store_pi'][:store_used] = rng.integers(-12, 13, (store_used, n)) / rng.choice([1.0, 2.0, 3.0, 7.0], (store_used, 1))
    s['store_pi0'][:store_used] = rng.integers(-20, 5, store_used) / 3.0
    s['store_count'] = np.array([store_used], np.int32)
    s['active'] = np.ones(B, np.int32) if active is None else np.array(active, np.int32)
    s['ncut'] = np.array(lengths, np.int32)
    s['ids'] = np.full((B, kc), STALE_ID, np.int32)
    parts = [_tableau(rng, n, m + int(lengths[k]), ms, is_int, square is None or bool(square[k])) for k in range(B)]
    s['T'], s['idx'], s['vstat'], s['x'] = (np.stack([p[q] for p in parts]) for q in range(4))
    for k in range(B):
        s['ids'][k, :lengths[k]] = rng.permutation(store_used)[:lengths[k]]
    s['state'] = rng.integers(0, 4, (len(FIELDS), B)).astype(np.int32)
    s['state'][F['pool_n']] = 0
    s['state'][F['slab_n']] = 0
    s['pool_list'] = np.full((B, slab_rows), STALE_LIST, np.int32)
    s['slab_pi'] = np.full((B, slab_rows, n), STALE_SLAB)
    s['slab_pi0'] = np.full((B, slab_rows), STALE_SLAB)
    s['resolve'] = np.zeros(B, np.int32)
    s['counters'] = np.array([B, 1, 2, 0], np.int32)
    s.update(over)
    return s


def _plant(s, k, rows, plist, x=None):
    """Slab rows 0 .. len(rows) - 1 of node k as given ((pi, pi0) pairs), its pool the entries plist; x of the node."""
    for r, (pi, pi0) in enumerate(rows):
        s['slab_pi'][k, r], s['slab_pi0'][k, r] = pi, pi0
    s['state'][F['slab_n'], k] = len(rows)
    s['state'][F['pool_n'], k] = len(plist)
    s['pool_list'][k, :len(plist)] = plist
    if x is not None:
        s['x'][k] = x


def _unit(n, j, value=1.0):
    e = np.zeros(n)
    e[j] = value
    return e


def _made(s, k):
    n, mk = s['A'].shape[1], s['A'].shape[0] + int(s['ncut'][k])
    return count_cuts(n, s['idx'][k][n:n + mk], s['x'][k], s['is_int'])


def invariance_state(n, m, variant):
    """The state of the launch-shape sweep: kc = 8, three nodes with 0, 3 and 8 cut rows.  Variant 'all': every node
    generates (the node with 8 rows has no room in its list).  Variant 'mixed': the first node does not generate
    (active = 0), the second has a basis that is not square, the third goes on."""
    mixed = variant == 'mixed'
    s = _blank(n, m, 8, 3, 1000 * n + m + mixed, (0, 3, 8), slab_rows=2 * (m + 8), active=(0, 1, 1) if mixed else None,
               square=(1, 0, 1) if mixed else None)
    if mixed:
        # the node without a tableau still selects: from a pool it had before
        _plant(s, 1, [(_unit(n, 4), 1.0), (_unit(n, 9), 2.0), (_unit(n, 2), 1.0)], [2, 0], x=np.full(n, 0.5))
    return s


def _fold(rows):
    m, nc = {1: (1, 0), 2: (1, 1), 63: (60, 3), 64: (60, 4), 65: (60, 5), 128: (120, 8), 129: (121, 8)}[rows]
    n = 7 if m == 1 else 40
    for seed in range(5000 + 100 * rows, 5100 + 100 * rows):      # (the first seed whose two bases both give a cut)
        s = _blank(n, m, 8, 2, seed, (nc, max(nc - 1, 0)), slab_rows=2 * (m + 8))
        s['is_int'][:] = 1
        if min(_made(s, 0), _made(s, 1)) >= 1:
            return s
    raise AssertionError('no seed gives both nodes a cut')


def _big():
    # 1024 x 512 with 60 of 64 cut rows: 572 rows fold over 1024 entries, a group of 8 stages 116 KiB of LDS
    s = _blank(1024, 512, 64, 1, 4242, (60,), slab_rows=600, store_used=80)
    s['is_int'][:] = 0
    s['is_int'][::7] = 1
    return s


def _slab(kind):
    s = _blank(11, 6, 8, 2, 900 + len(kind), (2, 0), slab_rows=20)
    s['is_int'][:] = 1
    for k in range(2):
        made = _made(s, k)
        assert made >= 2
        taken = dict(exact=20 - made, over1=20 - made + 1, full=20)[kind]
        rows = [(np.round(np.sin(np.arange(11) + r + k), 2), -float(r)) for r in range(taken)]
        _plant(s, k, rows, list(range(0, taken, 3)))
    return s


def _k3(kind):
    n = 9
    if kind == 'holes':
        # the pool lost entries in the middle: positions != rows; two nearly parallel cuts; a row without support
        s = _blank(n, 5, 8, 2, 31, (1, 0), slab_rows=16)
        base = np.array([1.0, 2.0, 0.0, -1.0, 0.5, 0.0, 3.0, 0.0, 1.0])
        near = base.copy(); near[0] += 1e-6
        rows = [(_unit(n, 0), 3.0), (base, 40.0), (np.full(n, 0.005), 1.0), (near, 41.0), (_unit(n, 3), 2.0),
                (-base, 1.0), (_unit(n, 5, 2000.0), 4000.0), (_unit(n, 7), 2.5)]
        for k in range(2):
            _plant(s, k, rows, [7, 1, 2, 3, 6, 4] if k == 0 else [3, 5, 1, 0], x=np.linspace(0.1, 0.9, n))
        s['max_abs_coef'] = 1000.0
    elif kind == 'maxnz1':
        s = _blank(n, 5, 8, 2, 32, (0, 2), slab_rows=16, max_nonzero_coefs=1)
        two = _unit(n, 1) + _unit(n, 2)
        rows = [(two, 9.0), (_unit(n, 4), 1.0), (_unit(n, 6, 0.5), 1.0), (_unit(n, 4) + _unit(n, 0, 0.01), 1.5)]
        for k in range(2):
            _plant(s, k, rows, [0, 1, 2, 3][k:], x=np.full(n, 0.25))
    elif kind == 'terminators':
        # 0: a cut deep enough; 1: no candidate (empty pool; a pool of rows without support); 2: nothing violated;
        # 3: violated by less than min_cut_depth
        s = _blank(n, 5, 8, 5, 33, (0, 1, 2, 0, 3), slab_rows=16)
        s['is_int'][:] = 0                                      # (no new cuts: the pools are what is planted)
        half = np.full(n, 0.5)
        _plant(s, 0, [(_unit(n, 0), 1.0)], [0], x=half)
        _plant(s, 1, [], [], x=half)
        _plant(s, 2, [(np.full(n, 0.01), 5.0), (np.zeros(n), 1.0)], [1, 0], x=half)
        _plant(s, 3, [(_unit(n, 0), 0.5), (_unit(n, 1), 0.25)], [0, 1], x=half)
        _plant(s, 4, [(_unit(n, 0), 0.5 + 5e-9), (_unit(n, 1), 0.5)], [0, 1], x=half)
    else:
        # kmax = 2040: a full pool at n = 8 (the slab is full as well: every new cut is dropped)
        for seed in range(34, 64):                              # (the first seed whose basis gives a cut to drop)
            s = _blank(8, 4, 64, 1, seed, (5,), slab_rows=2040)
            s['is_int'][:] = 1
            if _made(s, 0) >= 1:
                break
        rng = np.random.default_rng(35)
        pi = rng.integers(-9, 10, (2040, 8)) / 4.0
        pi0 = rng.uniform(-60.0, -20.0, 2040)                   # far from violated ...
        hit = rng.permutation(2040)[:48]
        pi0[hit] = rng.uniform(30.0, 60.0, 48)                  # ... but for 48 of them
        _plant(s, 0, list(zip(pi, pi0)), rng.permutation(2040))
    return s


def _apply(kind, B):
    """Pools of orthogonal unit cuts x_j >= 1 at x = 0.5 - j / 100: every violated one is selected, the deepest (largest
    j) first; the problem has no integer column, so K2 adds nothing.  list room and store room as the kind says."""
    n, kc = 12, 8
    picks = dict(first=[0], last=[4], all=[0, 1, 2, 3, 4]).get(kind.split('-')[-1], [0, 2, 3])
    size = len(picks)
    lroom = dict(list0=0, list1=1, listexact=size).get(kind.split('-')[0], kc - 2)
    sroom = dict(store0=0, store1=1, storeexact=size * B).get(kind.split('-')[0], 1000)
    if kind.startswith('both'):
        lroom, sroom = 2, 1 if B == 1 else B + 1
    s = _blank(n, 5, kc, B, 60 + B + sum(map(ord, kind)), [kc - lroom] * B, slab_rows=12, store_used=20, store_room=sroom)
    s['is_int'][:] = 0
    x = 0.5 - np.arange(n) / 100.0
    for k in range(B):
        rows = [(_unit(n, j), 1.0 if q in picks else 0.25) for q, j in enumerate((3, 7, 1, 10, 5))]
        _plant(s, k, rows, [0, 1, 2, 3, 4], x=x)
    if kind == 'resolve-in':
        s['resolve'][:] = 1
        s['state'][F['pool_n']] = 0                              # (nothing to select: resolve stays as it came)
    return s


def _real(kind, oracle):
    """The tableau a solve ended with (oracle.debug_dump): the root of a 64 x 32 instance; and the same node once three
    of its own cuts are rows of its LP, re-solved over the 35 materialised rows."""
    from simple_mip_solver_amd.generators import random_dense_milp_arrays
    A, b, c, l, u, ints = random_dense_milp_arrays(64, 32, seed=11)
    n, m, kc = 64, 32, 8
    res, dump = oracle.debug_dump(A, b, c, l, u)
    assert res['status'][0] == 0
    rows, rhs, nc = A, b, 0
    store_used = 6
    s = _blank(n, m, kc, 1, 70, (0,), slab_rows=3 * (m + kc), store_used=store_used)
    s.update(A=A, b=b, is_int=np.ones(n, np.uint8))
    if kind == 'resolved':
        g = oracle.gomory_from_dump(A, b, dump, res['x'][0], ints)
        assert len(g['safe_pi0']) >= 3
        nc = 3
        s['store_pi'][1:4], s['store_pi0'][1:4] = g['safe_pi'][:3], g['safe_pi0'][:3]
        s['ids'][0, :3] = (1, 2, 3)
        rows, rhs = np.vstack([A, g['safe_pi'][:3]]), np.concatenate([b, g['safe_pi0'][:3]])
        res, dump = oracle.debug_dump(rows, rhs, c, l, u)
        assert res['status'][0] == 0
    mk, ms = m + nc, m + kc
    s['ncut'][0] = nc
    s['T'][0] = np.vstack([dump['T'], np.full((ms - mk, n), np.nan)])
    s['idx'][0, :] = -5
    s['idx'][0, :n], s['idx'][0, n:n + mk], s['idx'][0, n + ms:] = dump['nvar'], dump['bvar'], dump['side']
    s['vstat'][0, :] = STALE_CODE
    s['vstat'][0, :n + mk] = res['vstat'][0]
    s['x'][0] = res['x'][0]
    return s


GENERATE = {}
for _rows in (1, 2, 63, 64, 65, 128, 129):
    GENERATE['fold-%d-rows' % _rows] = (_fold, (_rows,))
GENERATE['fold-1024x512-above-64KiB'] = (_big, ())
for _kind in ('exact', 'over1', 'full'):
    GENERATE['slab-' + _kind] = (_slab, (_kind,))
for _kind in ('holes', 'maxnz1', 'terminators', 'kmax2040'):
    GENERATE['k3-' + _kind] = (_k3, (_kind,))
for _kind in ('list0', 'list1', 'listexact', 'store0', 'store1', 'storeexact', 'both', 'select-first', 'select-last', 'select-all',
              'resolve-in'):
    for _B in (1, 3):
        GENERATE['apply-%s-B%d' % (_kind, _B)] = (_apply, (_kind, _B))
for _shape in ((65, 33), (64, 32), (64, 33)):
    for _variant in ('all', 'mixed'):
        GENERATE['sweep-%dx%d-%s' % (_shape + (_variant,))] = (invariance_state, _shape + (_variant,))
REAL = ('real-root', 'real-resolved')
for _name in GENERATE:
    CASES['generate-' + _name] = ('generate', _name)
for _name in REAL:
    CASES['generate-' + _name] = ('generate', _name)
BEGIN_CASES = [name for name, (what, _) in CASES.items() if what == 'begin']
GENERATE_CASES = [name for name, (what, _) in CASES.items() if what == 'generate']
SWEEP_CASES = [name for name in GENERATE_CASES if name.startswith('generate-sweep-')]
_CACHE = {}


def case(name):
    """(round, what it must become): computed once, shared by the tests, and not to be written to."""
    if name not in _CACHE:
        what, arg = CASES[name]
        if what == 'begin':
            s = _gather_last_largest() if arg is None else _begin_round(*arg)
            _CACHE[name] = (s, begin(s))
        else:
            from oracle import oracle
            if arg in REAL:
                s = _real(arg.split('-')[1], oracle)
            else:
                make, args = GENERATE[arg]
                s = make(*args)
            _CACHE[name] = (s, generate(s, oracle))
    return _CACHE[name]
