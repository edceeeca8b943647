"""A plain restatement of what finishing one batched step means, and seeded synthetic steps to run it on.

finish_step(step) walks the batch as the reference's loop does (algorithms/branch_and_bound.py:243-266 for the
decision at a node, nodes/base_node.py:592-608 for the two child records, nodes/branch/pseudo_cost.py:38-43 and
:68-100 for the running mean): chain by chain, level by level, with ONE scalar incumbent that it lowers as it goes.
It has no prefix minimum and no scan; it is not written from the kernels of csrc/finish_kernels.hip.h, which must
give the same bytes (tests/test_finish_kernels_gpu.py through mipx_finish_step_batch of include/mipx_finish.h).
Test infrastructure only.

A step: B chains.  Chain k is the node at position (0, k) of the (dive + 1) x B result arrays and the children solved in
place below it at (1, k), (2, k), ...; the child below (p, k) COUNTS when dvar[p, k] >= 0, status[p + 1, k] >= 0 and
nprobe[p + 1, k] == 0.  A chain with nprobe[0, k] > 0 is deferred: it is the host's, nothing of it is evaluated here and
its whole budget of pool rows comes back.

INPUT CONTRACT.  obj[p + 1, k] >= obj[p, k] wherever the child counts: LP values do not decrease down a plunge.  The
kernels rely on it (finish_candidates takes the incumbent a chain sees as a prefix minimum over the integral leaves of
the chains before it, whether or not those were cut short); every generator below keeps obj non-decreasing down every
chain, and finish_step asserts it.

Order of the lists.  open: in creation order -- chain, level, left then right.  dead (the pool rows free again): chain
by chain, level by level, left then right, every row of the chain's budget that holds no open node.  samples: chain by
chain; the branch that made the chain's node, then one per dive child that counts.
"""
import collections

import numpy as np

from simple_mip_solver_amd._ffi import OPEN_ENTRY_DTYPE, PC_SAMPLE_DTYPE

INF = float('inf')
SENTINEL_BOUND = -7777.25      # every entry of an unused pool row's l and u
SENTINEL_BASIS = 0x5a          # ... and of its basis codes
SUMMARY_FIELDS = ('host_path', 'n_open', 'n_dead', 'n_samples', 'unbounded', 'incumbent_pos', 'n_deferred', 'evaluated',
                  'dives', 'pivots', 'closed_min', 'primal', 'primal_before')
COSTED = (0, 3)                # LP statuses whose sample changes the mean (pseudo_cost.py:86); every other only counts


def lp_feasible(st):
    return st == 0 or st == 2


def variable_change(v, direction):
    """pseudo_cost.py:93-94 with the child's bound at floor / ceil of the branching value."""
    return v - np.floor(v) if direction == 0 else np.ceil(v) - v


def apply_samples(samples, cost_l, cost_r, has, times, own):
    """pseudo_cost.py:68-100, sample by sample in list order, float64 scalars.  times: [left | right] (2 n); own: the
    same samples in sum form, [sum_l | sum_r | times_l | times_r] (4 n) -- a sample that counts without a cost weighs
    in with the current mean.  Returns new arrays."""
    cost = [np.array(cost_l, np.float64), np.array(cost_r, np.float64)]
    has, times, own = np.array(has, np.uint8), np.array(times, np.int32), np.array(own, np.float64)
    n = len(has)
    for s in samples:
        var, d = int(s['var_dir']) >> 1, int(s['var_dir']) & 1
        c, t = float(cost[d][var]), int(times[d * n + var])
        if int(s['status']) in COSTED:
            bound_change = float(s['obj']) - float(s['bound'])
            if bound_change < 0:
                bound_change = 0.0
            rate = bound_change / float(s['vc'])
            cost[d][var] = (c * float(t) + rate) / float(t + 1)
            own[d * n + var] += rate
        else:
            own[d * n + var] += c
        times[d * n + var] = t + 1
        own[(2 + d) * n + var] += 1.0
        has[var] = 1
    return cost[0], cost[1], has, times, own


def finish_step(step):
    """The step finished by the walk.  Returns a dict: summary (the SUMMARY_FIELDS; host_path alone when the step is
    left to the host), open / dead / samples / sample_keys (as long as their counts), pool_l / pool_u / pool_v and the
    table after the step, primal, and paths: a Counter of what the walk met (test_cases_cover_every_path)."""
    n, m, B, dive, rule = (int(step[k]) for k in ('n', 'm', 'B', 'dive', 'rule'))
    L, per = dive + 1, 2 * (1 + dive)
    status, bidx, mipf, nprobe, npiv, dvar, ddir = (np.asarray(step[k]).reshape(L, B) for k in
                                                    ('status', 'bidx', 'mipf', 'nprobe', 'npiv', 'dvar', 'ddir'))
    obj, bval, dval = (np.asarray(step[k], np.float64).reshape(L, B) for k in ('obj', 'bval', 'dval'))
    vout = np.asarray(step['vout'], np.int8).reshape(L, B, n + m)
    slot, par_i, par_d = np.asarray(step['slot']), np.asarray(step['par_i']).reshape(4, B), np.asarray(step['par_d']).reshape(2, B)
    budget = np.asarray(step['budget']).reshape(B, per)
    pool_l, pool_u, pool_v = np.array(step['pool_l'], np.float64), np.array(step['pool_u'], np.float64), np.array(step['pool_v'], np.int8)
    table = tuple(np.array(step[k]) for k in ('cost_l', 'cost_r', 'has', 'times', 'own')) if rule == 1 else (None,) * 5
    paths = collections.Counter()
    out = dict(pool_l=pool_l, pool_u=pool_u, pool_v=pool_v, primal=float(step['primal']), paths=paths,
               open=np.zeros(0, OPEN_ENTRY_DTYPE), dead=np.zeros(0, np.int32), samples=np.zeros(0, PC_SAMPLE_DTYPE),
               sample_keys=np.zeros(0, np.int32))
    out.update(zip(('cost_l', 'cost_r', 'has', 'times', 'own'), table))
    if int(step['ask_count']) > int(step['ask_cap']):    # more probe requests than the compact list holds: the host's
        out['summary'] = dict(host_path=1)
        paths['ask_cap'] += 1
        return out

    def counts(p, k):   # the child below (p, k) was solved in place and counts
        return p < dive and dvar[p, k] >= 0 and status[p + 1, k] >= 0 and nprobe[p + 1, k] == 0

    for k in range(B):
        for p in range(dive):
            assert not counts(p, k) or obj[p + 1, k] >= obj[p, k], 'input contract: obj does not decrease down a chain'

    primal_before = primal = float(step['primal'])
    paths['primal_inf' if primal == INF else 'primal_finite'] += 1
    # the pseudo-cost samples come first, against the value the step starts with (bound() updates the table before
    # _evaluate_node looks at the node: pseudo_cost.py:40-43)
    samples = []
    if rule == 1:
        for k in range(B):
            if nprobe[0, k] > 0 or not lp_feasible(status[0, k]):
                continue
            if par_i[0, k] >= 0:
                d = int(par_i[1, k])
                samples.append((2 * int(par_i[0, k]) + d, status[0, k], obj[0, k], par_d[0, k], variable_change(par_d[1, k], d)))
            p = 0
            while counts(p, k) and obj[p, k] < primal_before and not mipf[p, k] and lp_feasible(status[p, k]):
                if not lp_feasible(status[p + 1, k]):
                    break
                d = int(ddir[p, k])
                samples.append((2 * int(dvar[p, k]) + d, status[p + 1, k], obj[p + 1, k], obj[p, k], variable_change(dval[p, k], d)))
                p += 1
    samples = np.array(samples, PC_SAMPLE_DTYPE)
    for s in samples:
        paths['sample_costed' if int(s['status']) in COSTED else 'sample_count_only'] += 1
        paths['sample_negative_change'] += bool(s['obj'] < s['bound'])

    opened, dead = [], []
    evaluated = pivots = unbounded = n_deferred = 0
    incumbent_pos, closed_min = -1, INF
    leaves = []     # the integral feasible nodes the walk reached
    for k in range(B):
        if nprobe[0, k] > 0:
            n_deferred += 1
            dead.extend(int(r) for r in budget[k])
            continue
        l, u = pool_l[slot[k]].copy(), pool_u[slot[k]].copy()     # the node's bounds, carried down the chain
        p = 0
        while True:
            evaluated += 1
            pivots += int(npiv[p, k])
            st, value = int(status[p, k]), float(obj[p, k])
            if st == 2:
                unbounded = 1
                paths['status_unbounded'] += 1
            branched = go_on = False
            if lp_feasible(st) and value < primal:
                dived = counts(p, k)
                var = int(dvar[p, k] if dived else bidx[p, k])
                if mipf[p, k]:
                    leaves.append(value)
                    primal, incumbent_pos = value, p * B + k
                elif var >= 0:
                    branched, go_on = True, dived
                    x = float(dval[p, k] if dived else bval[p, k])
                    for d in (0, 1):
                        row = int(budget[k, 2 * p + d])
                        if dived and d == ddir[p, k]:     # solved in place: never a record, never queued
                            dead.append(row)
                            continue
                        pool_l[row], pool_u[row] = l, u
                        if d == 0:
                            pool_u[row, var] = np.floor(x)
                        else:
                            pool_l[row, var] = np.ceil(x)
                        pool_v[row] = vout[p, k]         # the basis its parent's LP ended with
                        opened.append((value, x, row, int(par_i[2, k]) + p + 1, 2 * var + d, int(par_i[3, k])))
                    if dived:
                        paths['dive_left' if ddir[p, k] == 0 else 'dive_right'] += 1
                        if ddir[p, k] == 0:
                            u[var] = np.floor(x)
                        else:
                            l[var] = np.ceil(x)
                    if p < dive and dvar[p, k] >= 0 and not dived:
                        paths['dive_dropped_unsolved' if status[p + 1, k] < 0 else 'dive_dropped_probes'] += 1
                    paths['branch_column_%d' % var] += 1
            elif lp_feasible(st):
                if mipf[p, k]:
                    leaves.append(value)
                    paths['leaf_equal_incumbent' if value == primal else 'leaf_worse'] += 1
                    if value == primal and primal < primal_before:
                        paths['leaf_tie'] += 1
                        paths['leaf_tie_same_range' if _same_range(B, k, incumbent_pos % B) else 'leaf_tie_other_range'] += 1
                if p > 0 and value < primal_before:
                    paths['pruned_mid_chain_by_earlier_chain'] += 1
            if not branched:
                closed_min = min(closed_min, value if lp_feasible(st) else INF)
                dead.extend(int(budget[k, 2 * q + d]) for q in range(p, L) for d in (0, 1))
                break
            if not go_on:
                dead.extend(int(budget[k, 2 * q + d]) for q in range(p + 1, L) for d in (0, 1))
                break
            p += 1
    if n_deferred and n_deferred < B:
        paths['deferred_beside_finished'] += 1
    if not opened:
        paths['nothing_open'] += 1
    paths['no_improvement' if incumbent_pos < 0 else 'improvement'] += 1
    assert primal == min([primal_before] + leaves)
    out['summary'] = dict(host_path=0, n_open=len(opened), n_dead=len(dead), n_samples=len(samples), unbounded=unbounded,
                          incumbent_pos=incumbent_pos, n_deferred=n_deferred, evaluated=evaluated,
                          dives=evaluated - (B - n_deferred), pivots=pivots, closed_min=closed_min, primal=primal,
                          primal_before=primal_before)
    out.update(open=np.array(opened, OPEN_ENTRY_DTYPE), dead=np.array(dead, np.int32), samples=samples,
               sample_keys=np.array(samples['var_dir'], np.int32), primal=primal, leaves=leaves)
    if rule == 1:
        out.update(zip(('cost_l', 'cost_r', 'has', 'times', 'own'), apply_samples(samples, *table)))
    return out


def _same_range(B, k0, k1):
    """Chains k0 and k1 fall to the same thread of the one-workgroup kernels (1024 threads, ceil(B / 1024) chains each)."""
    per_thread = -(-B // 1024)
    return k0 // per_thread == k1 // per_thread


# ---- synthetic steps ---------------------------------------------------------------------------------------------
def _blank(n, m, B, dive, rule, rng, spare=3):
    """A step of B chains in which every LP is optimal, nothing is integral, every node branches on a random column and
    takes no dive; distinct pool rows for the batch and its budget in a shuffled order, `spare` rows that nobody owns;
    unused rows hold the sentinels.  Values are multiples of 1/8: ties happen, and every sum below is exact."""
    L, per, nv = dive + 1, 2 * (1 + dive), n + m
    rows = B + B * per + spare
    perm = rng.permutation(rows).astype(np.int32)
    slot, budget = perm[:B].copy(), perm[B:B + B * per].reshape(B, per).copy()
    s = dict(n=n, m=m, B=B, dive=dive, rule=rule, ask_count=0, ask_cap=16, primal=INF)
    s['status'] = np.zeros((L, B), np.int32)
    s['bidx'] = rng.integers(0, n, (L, B)).astype(np.int32)
    s['mipf'] = np.zeros((L, B), np.int32)
    s['nprobe'] = np.zeros((L, B), np.int32)
    s['npiv'] = rng.integers(0, 40, (L, B)).astype(np.int32)
    s['dvar'] = np.full((L, B), -1, np.int32)
    s['ddir'] = rng.integers(0, 2, (L, B)).astype(np.int32)
    s['obj'] = np.cumsum(rng.integers(0, 24, (L, B)) / 8.0, axis=0) + rng.integers(0, 400, B) / 8.0
    s['bval'] = rng.integers(-3, 9, (L, B)) + rng.integers(1, 8, (L, B)) / 8.0
    s['dval'] = rng.integers(-3, 9, (L, B)) + rng.integers(1, 8, (L, B)) / 8.0
    s['vout'] = rng.integers(-4, 4, (L * B, nv)).astype(np.int8)
    s['slot'], s['budget'] = slot, budget
    par_var = rng.integers(0, n, B)
    par_var[rng.random(B) < 0.1] = -1          # (a root, or a seed: no branch made it)
    s['par_i'] = np.stack([par_var, rng.integers(0, 2, B), rng.integers(0, 30, B), rng.integers(-1, 5, B)]).astype(np.int32)
    s['par_d'] = np.stack([s['obj'][0] - rng.integers(-4, 40, B) / 8.0,          # (some above the node's value)
                           rng.integers(-3, 9, B) + rng.integers(1, 8, B) / 8.0])
    s['pool_l'] = np.full((rows, n), SENTINEL_BOUND)
    s['pool_u'] = np.full((rows, n), SENTINEL_BOUND)
    s['pool_v'] = np.full((rows, nv), SENTINEL_BASIS, np.int8)
    s['pool_l'][slot] = -1.0 - np.arange(n) - rng.integers(0, 3, (B, n))
    s['pool_u'][slot] = 1000.0 + np.arange(n) + rng.integers(0, 3, (B, n))
    s['pool_v'][slot] = rng.integers(-4, 4, (B, nv))
    s['cost_l'] = rng.integers(0, 64, n) / 8.0
    s['cost_r'] = rng.integers(0, 64, n) / 8.0
    s['has'] = (rng.random(n) < 0.5).astype(np.uint8)
    s['times'] = rng.integers(0, 6, 2 * n).astype(np.int32)
    s['own'] = rng.integers(0, 64, 4 * n) / 8.0
    return s


def _randomise(s, rng, p_int=0.08, p_inf=0.15, p_unb=0.03, p_dive=0.75, p_defer=0.06, p_drop=0.12, p_nobranch=0.03):
    """The outcomes of a search by chance, on every position of the step -- also on those behind a chain's end, which
    nothing may read."""
    L, B = s['status'].shape
    r = rng.random((L, B))
    s['status'][r < p_inf] = 1
    s['status'][(r >= p_inf) & (r < p_inf + p_unb)] = 2
    s['status'][(r >= p_inf + p_unb) & (r < p_inf + p_unb + 0.02)] = 3      # (stopped on iterations: not lp_feasible)
    s['mipf'][rng.random((L, B)) < p_int] = 1
    s['bidx'][rng.random((L, B)) < p_nobranch] = -1
    dv = rng.integers(0, s['n'], (L, B)).astype(np.int32)
    s['dvar'][:] = np.where(rng.random((L, B)) < p_dive, dv, -1)
    s['dvar'][L - 1] = rng.integers(-1, s['n'], B)        # (never read: no level below the last)
    drop = rng.random((L, B))
    s['status'][1:][drop[1:] < p_drop / 2] = -1            # a dive child whose LP was not solved
    s['nprobe'][1:][(drop[1:] >= p_drop / 2) & (drop[1:] < p_drop)] = 2      # ... or that asks for probes of its own
    s['nprobe'][0][rng.random(B) < p_defer] = 3
    return s


def _median_primal(s):
    """An incumbent value in the middle of the step's root values: about half of the chains are pruned at once."""
    return float(np.median(s['obj'][0]))


def _width(B, nm, dive, rule):
    rng = np.random.default_rng([B, nm[0], dive, rule, 1])
    s = _randomise(_blank(nm[0], nm[1], B, dive, rule, rng), rng)
    if B >= 2:      # a chain that dives to the bottom wherever the step has levels: the lowest values of the step
        s['nprobe'][:, 1] = 0
        s['status'][:, 1] = 0
        s['mipf'][:, 1] = 0
        s['dvar'][:, 1] = np.arange(s['dive'] + 1) % s['n']
        s['obj'][:, 1] = float(s['obj'].min()) - 1.0
    # by turns: no incumbent yet, one in the middle of the batch's values
    if (B + dive + rule + nm[0]) % 2:
        s['primal'] = _median_primal(s)
    return s


def _columns(n):
    """B = 3, dive = 8: chain 0 plunges through the register edges of finish_write (columns 0, 255, 256, 511, 512, n - 1
    where they exist), left and right by turns, and branches on n - 1 at the bottom; chain 1 does the same the other way
    round, and branches twice on one column (right, then left: the carried bound is read back); chain 2 is random."""
    rng = np.random.default_rng([n, 77])
    s = _randomise(_blank(n, 3, 3, 8, 1, rng), rng)
    edges = [c for c in (0, 255, 256, 511, 512, n - 1) if c < n]
    edges = list(dict.fromkeys(edges))
    for k in (0, 1):
        s['status'][:, k], s['mipf'][:, k], s['nprobe'][:, k] = 0, 0, 0
        cols = [edges[(p + k) % len(edges)] for p in range(9)]
        if k == 1:
            cols[1] = cols[0]
        s['dvar'][:, k] = cols
        s['dvar'][8, k] = -1
        s['bidx'][:, k] = cols[::-1]
        s['bidx'][8, k] = n - 1
        s['ddir'][:, k] = (np.arange(9) + k) % 2
        s['dval'][:, k] = 2.0 + np.arange(9) + 0.5
        s['dval'][1, 1] = s['dval'][0, 1] + 1.0       # (chain 1, the column twice: x >= 3 from the right dive, then x <= 3)
        s['bval'][8, k] = 6.25
    s['primal'] = INF
    return s


def _plant_leaf(s, k, level, value):
    """Chain k dives undisturbed to `level` and ends there in an integral node of objective `value`."""
    s['nprobe'][:, k], s['status'][:, k], s['mipf'][:, k] = 0, 0, 0
    s['dvar'][:level, k] = np.arange(level) % s['n']
    s['obj'][:level + 1, k] = value - (level - np.arange(level + 1)) / 8.0
    s['obj'][level + 1:, k] = value + 1.0
    s['mipf'][level, k] = 1


def _outcome(name):
    rng = np.random.default_rng([sum(name.encode()), len(name)])
    if name == 'tie-same-range':        # B = 2049: three chains a thread; chains 300 and 302 are one thread's
        s = _randomise(_blank(5, 3, 2049, 1, 1, rng), rng)
        low = float(s['obj'].min()) - 2.0
        s['primal'] = low + 40.0
        _plant_leaf(s, 300, 1, low)
        _plant_leaf(s, 302, 0, low)
    elif name == 'tie-across-ranges':   # B = 2049: chains 4 and 1500 are far apart; the later one at a lower level
        s = _randomise(_blank(6, 3, 2049, 8, 0, rng), rng)
        low = float(s['obj'].min()) - 2.0
        _plant_leaf(s, 4, 3, low)
        _plant_leaf(s, 1500, 0, low)
    elif name == 'tie-small':           # ... and where every thread has one chain
        s = _randomise(_blank(5, 3, 7, 1, 1, rng), rng)
        low = float(s['obj'].min()) - 2.0
        _plant_leaf(s, 2, 1, low)
        _plant_leaf(s, 5, 1, low)
    elif name == 'leaf-equals-incumbent':   # no improvement: every integral leaf is at or above the incumbent
        s = _randomise(_blank(5, 3, 1025, 1, 1, rng), rng, p_int=0.0)
        s['primal'] = _median_primal(s)
        for k in (0, 513, 1024):
            _plant_leaf(s, k, 1, s['primal'])
        _plant_leaf(s, 700, 0, s['primal'] + 1.0)
    elif name == 'prune-mid-plunge':    # chain 1 finds the incumbent; chains 2 and 1030 start below it and plunge past it
        s = _randomise(_blank(6, 3, 1030 + 3, 8, 1, rng), rng)
        low = float(s['obj'].min()) - 8.0
        s['primal'] = low + 100.0
        _plant_leaf(s, 1, 2, low + 4.0)
        for k in (2, 1031):
            _plant_leaf(s, k, 6, low + 9.0)      # (its levels 0..2 lie below low + 4, level 3 and on at or above)
            s['obj'][:, k] = low + 1.0 + 1.0 * np.arange(9)
    elif name == 'all-closed':          # every node infeasible or pruned: nothing opens
        s = _randomise(_blank(5, 3, 1500, 1, 1, rng), rng)
        s['primal'] = float(s['obj'].min())
        s['status'][0, ::3] = 1
        s['nprobe'][:] = 0
    elif name == 'all-infeasible':
        s = _randomise(_blank(6, 3, 5, 8, 0, rng), rng)
        s['status'][0] = 1
        s['nprobe'][:] = 0
    elif name == 'unbounded':           # LP status 2 counts as feasible, and raises the flag
        s = _randomise(_blank(5, 3, 9, 1, 1, rng), rng, p_unb=0.4)
    elif name == 'deferred':            # chains that filed probe requests beside finished ones
        s = _randomise(_blank(5, 3, 1100, 1, 1, rng), rng, p_defer=0.4)
        s['primal'] = _median_primal(s) + 10.0
    elif name == 'dropped-dive-children':
        s = _randomise(_blank(6, 3, 40, 8, 1, rng), rng, p_drop=0.6, p_inf=0.05, p_int=0.02)
    elif name == 'ask-cap':             # more requests than the compact list holds: every kernel leaves everything alone
        s = _randomise(_blank(5, 3, 1100, 1, 1, rng), rng)
        s['ask_count'], s['ask_cap'] = 17, 16
    elif name == 'ask-at-cap':          # ... and exactly as many: the device finishes the step
        s = _randomise(_blank(5, 3, 6, 1, 1, rng), rng)
        s['ask_count'], s['ask_cap'] = 16, 16
    else:
        raise KeyError(name)
    return s


def _samples(count, owner):
    """rule 1, no dive: exactly `count` samples, one per chain whose node a branch made.  owner: every one of them goes
    to one (variable, direction); else they spread over n = 5 columns.  Status 2 (counts without a cost) among them,
    and parents' bounds above the node's value (a negative change, clamped)."""
    rng = np.random.default_rng([count, int(owner), 5])
    B = max(count, 2)
    s = _blank(5, 3, B, 0, 1, rng)
    s['par_i'][0] = 3 if owner else rng.integers(0, 5, B)
    if owner:
        s['par_i'][1] = 1
    s['par_i'][0, count:] = -1
    s['status'][0][rng.random(B) < 0.2] = 2
    s['primal'] = _median_primal(s)
    return s


WIDTHS = (1, 2, 255, 256, 257, 1023, 1024, 1025, 2047, 2049, 4100)
SAMPLE_COUNTS = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2049)
OUTCOMES = ('tie-same-range', 'tie-across-ranges', 'tie-small', 'leaf-equals-incumbent', 'prune-mid-plunge', 'all-closed',
            'all-infeasible', 'unbounded', 'deferred', 'dropped-dive-children', 'ask-cap', 'ask-at-cap')
CASES = {}
for _B in WIDTHS:
    for _nm in ((5, 3), (6, 3)):
        for _dive in (0, 1, 8):
            for _rule in (0, 1):
                CASES['width-B%d-n%d-dive%d-rule%d' % (_B, _nm[0], _dive, _rule)] = (_width, (_B, _nm, _dive, _rule))
for _n in (256, 257, 512, 513, 1024):
    CASES['columns-n%d' % _n] = (_columns, (_n,))
for _name in OUTCOMES:
    CASES['outcome-' + _name] = (_outcome, (_name,))
for _count in SAMPLE_COUNTS:
    CASES['samples-%d' % _count] = (_samples, (_count, False))
CASES['samples-1025-one-owner'] = (_samples, (1025, True))
SAMPLE_CASES = [name for name in CASES if name.startswith('samples-')]
_CACHE = {}


def case(name):
    """(step, want) of a case, made once: want is finish_step's dict.  Every array is read-only."""
    if name not in _CACHE:
        make, args = CASES[name]
        step = make(*args)
        want = finish_step(step)
        for d in (step, want):
            for v in d.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        _CACHE[name] = (step, want)
    return _CACHE[name]


def host_samples(name):
    """The sample list of a SAMPLE_CASES step as a host would send it (mipx_pc_apply_batch): the same samples with
    statuses drawn afresh from those that cost (0, 3) and those that only count (1, 2, 4)."""
    step, want = case(name)
    rng = np.random.default_rng([len(want['samples']), 11])
    samples = np.array(want['samples'])
    samples['status'] = rng.choice([0, 3, 0, 3, 1, 2, 4], len(samples))
    return step, samples
