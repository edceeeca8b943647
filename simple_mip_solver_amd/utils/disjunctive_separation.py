"""Disjunctive cuts from the recorded tree of a native search, by row generation in the space of the cut.

For the not-infeasible childless nodes t below a node of the tree (the disjunctive terms
P_t = {A x >= b, l_t <= x <= u_t}) a cut pi.x >= pi0 is valid iff pi0 <= h_t(pi) := min {pi.x : x in P_t} for
every t.  The cut most violated at x* under the box normalisation -1 <= pi <= 1 solves

    min  pi.x* - pi0   s.t.   pi.x_k - pi0 >= 0  for every point x_k of every P_t,   -1 <= pi <= 1.

`CutGeneratingLP` writes a disjunctive cut's LP out in the multipliers of every term -- T (m + 2 n) columns,
which the LP kernels' 1024 columns hold for a handful of leaves.  `DisjunctiveSeparator` keeps (pi, pi0) only:

  master      n + 1 columns, one row per point found so far, solved through DenseLP on the LP kernels, each
              time warm-started from the last basis; rows that were slack are dropped when the rows near the
              kernels' limit;
  separation  one call per round evaluates h_t(pi) for all T leaves on the GPU (include/mipx_cglp.h: the leaves'
              bounds and last bases stay on the device, the node-LP kernel runs with pi in the place of c) and
              brings down the few most violated leaves with a minimiser of each: the master's new rows.

After every separation (pi, min_t h_t(pi)) is a valid cut whatever the master knew, so `solve` always returns
a valid cut: the one of largest violation min_t h_t(pi) - pi.x* met so far.  The rounds end when every term holds
within the tolerance (`stats['converged']`), at `max_rounds`, when every violated point is a master row already,
or when the engine stops a master or a leaf LP at its iteration limit (`stats['master_failed']`,
`stats['leaf_lps_not_optimal']`: a direction with such a leaf has no certified pi0 and is not used).

Options, all off by default (include/mipx_cglp_screen.h; DESIGN.md 4g.1 has what they measure to):

  screen         the session keeps each leaf's row duals; a round first computes the weak-duality bound
                 y.b + sum_j min(r_j l_j, r_j u_j), r = pi - A'y, of every leaf, and a leaf whose bound proves its
                 margin to within half the tolerance gets no LP.  Its margin is the bound's, a lower bound on its own,
                 so (pi, pi0 + min margin) stays valid; it is never among the rows used (they lie below -tol).
  stabilisation  lambda, 0 < lambda <= 1 (in-out).  The in-point is a certified cut (pi, pi0 + min margin): the one of
                 largest violation met, or the last separation point that held on every leaf within tol.  A round
                 separates at lambda master + (1 - lambda) in (at the master's point before there is an in-point).  A
                 violated round adds rows and re-solves the master.  A round that holds makes its point the in-point:
                 converged if v_in - v_master <= tol max(1, |v_master|); else it separates again without solving the
                 master, and after three such steps in a row at the master's point itself.
  retry_cold     a leaf LP that did not end optimal is solved once more without a basis before the round counts it.

The two classes normalise differently -- CutGeneratingLP sums the multipliers to one, as the reference does,
this class boxes pi -- so they return different cuts from the same disjunction; both are valid for it.

Terms: the childless nodes of the subtree (cut at `depth` levels, if given) that are not LP-infeasible.  This
includes a childless node the pseudo-cost rule made strong-branching probes from, which `get_leaves` leaves out
(the Python loop clears `is_leaf` on it): without it the terms would not cover the subtree root's integer points.

Scope: every column of the subtree root has finite bounds, so every term is a polytope.
"""
import time

import numpy as np

from simple_mip_solver_amd.lp import Constraint, CyLPArray, DenseLP

FINITE = 1e300   # COIN_INFINITY is 1.8e308: anything at or above this is an infinite bound


class DisjunctiveSeparator:

    def __init__(self, bb, root_id, depth=None, tol=1e-7, max_rounds=500, points_per_round=32, max_master_rows=768,
                 screen=False, stabilisation=None, retry_cold=False):
        """bb: a BranchAndBound solved with frontier_batch and tree_record=True; root_id: the node whose subtree
        gives the disjunction; depth: cut the subtree below this many levels; tol: stop when every term holds
        within tol max(1, |pi0|, |pi|_1); max_rounds: separations at most; points_per_round: rows a separation
        adds to the master at most; max_master_rows: slack rows leave the master above this many; screen: leaves
        whose stored duals prove their margin get no LP; stabilisation: the in-out weight of the master's point,
        0 < lambda <= 1; retry_cold: a leaf LP that did not end optimal is solved once more without a basis."""
        from simple_mip_solver_amd import _ffi
        from simple_mip_solver_amd.algorithms.branch_and_bound import BranchAndBound
        assert isinstance(bb, BranchAndBound), 'bb must be a BranchAndBound instance'
        assert bb.frontier_batch is not None, \
            'DisjunctiveSeparator needs a native search: solve the BranchAndBound with frontier_batch and tree_record=True'
        assert bb._tree_record, \
            'DisjunctiveSeparator reads the recorded tree: pass tree_record=True to the BranchAndBound'
        assert bb._native is not None and bb._native_stats is not None, \
            'bb must be solved before a disjunction is read from its tree'
        assert root_id in bb.tree, 'root node of the disjunction must be present in B & B tree'
        if depth is not None:
            assert isinstance(depth, int) and depth > 0, 'depth is postive integer'
        assert tol > 0 and isinstance(max_rounds, int) and max_rounds >= 1, 'tol is positive, max_rounds a positive integer'
        assert isinstance(points_per_round, int) and 1 <= points_per_round <= _ffi.CGLP_MAX_POINTS, \
            f'points_per_round is an integer from 1 to {_ffi.CGLP_MAX_POINTS}'
        self.bb, self.root_id, self.depth = bb, int(root_id), depth
        self.tol, self.max_rounds, self.points_per_round = float(tol), max_rounds, points_per_round
        self._set_options(screen, stabilisation, retry_cold)
        if self.root_id == 0:
            lo, up = (np.asarray(a, np.float64) for a in (bb.root_node.lp.variablesLower, bb.root_node.lp.variablesUpper))
        else:
            lo, up = (a[0] for a in bb._native.node_bounds([self.root_id]))
        assert np.all(np.abs(lo) < FINITE) and np.all(np.abs(up) < FINITE), \
            'every column of the subtree root must have finite bounds: the terms must be polytopes (rays are not handled)'
        self.n = len(lo)
        assert max_master_rows >= 2 * (self.n + 1) + points_per_round and max_master_rows + points_per_round <= 1024, \
            'max_master_rows is at least 2 (n + 1) + points_per_round and leaves room for a round under the 1024 rows of the LP kernels'
        self.max_master_rows = int(max_master_rows)
        self.R = float(np.maximum(np.abs(lo), np.abs(up)).sum())   # |h_t(pi)| <= R for every pi of the box
        self.leaf_ids = self._terms()
        if not len(self.leaf_ids):
            self._session = None
        elif self.screen or self.retry_cold:   # (the duals and the buffers of a packed launch stay on the device)
            self._session = bb._native.support_open(self.leaf_ids, duals=True)
        else:
            self._session = bb._native.support_open(self.leaf_ids)
        self.dropped_ids = np.zeros(0, np.int64)   # the terms the session found empty (LP infeasible)
        self.best_cut = None   # (pi, pi0) of the last solve(): the valid cut of largest violation met, violated or not
        self.stats = None
        self.timing = None     # wall seconds of the last solve(): dict(separation, master)

    @classmethod
    def on_session(cls, session, lo, up, tol=1e-7, max_rounds=500, points_per_round=32, max_master_rows=768,
                   screen=False, stabilisation=None, retry_cold=False):
        """A separator on an open _ffi.Support session whose leaves all lie in the box lo <= x <= up (no
        BranchAndBound: solve() then needs its x_star).  screen and retry_cold need a session opened with
        duals=True."""
        self = object.__new__(cls)
        self._set_options(screen, stabilisation, retry_cold)
        self.bb, self.root_id, self.depth = None, None, None
        self.tol, self.max_rounds, self.points_per_round = float(tol), int(max_rounds), int(points_per_round)
        self.max_master_rows = int(max_master_rows)
        self.n = len(lo)
        self.R = float(np.maximum(np.abs(lo), np.abs(up)).sum())
        self._session, self.leaf_ids = session, session.leaves()
        self.dropped_ids, self.best_cut, self.stats, self.timing = np.zeros(0, np.int64), None, None, None
        return self

    def _set_options(self, screen, stabilisation, retry_cold):
        assert isinstance(screen, bool) and isinstance(retry_cold, bool), 'screen and retry_cold are bool'
        if stabilisation is not None:
            assert isinstance(stabilisation, (int, float)) and 0 < stabilisation <= 1, \
                'stabilisation is None or the weight of the master\'s point, 0 < lambda <= 1'
        self.screen, self.retry_cold = screen, retry_cold
        self.stabilisation = None if stabilisation is None else float(stabilisation)

    def _terms(self):
        tree = self.bb.tree
        rel = tree._subtree(self.root_id)
        childless = (tree.rec['flags'] & 2) == 0   # (MIPX_TR_HAS_CHILDREN)
        if self.depth is None:
            found = childless & (rel >= 0)
        else:
            found = (childless & (rel >= 0) & (rel < self.depth)) | (rel == self.depth)
        found &= tree.lp_feasible | ~tree.solved
        return np.flatnonzero(found).astype(np.int64)

    def _default_point(self):
        root = self.bb.tree.get_node_instances(self.root_id)
        assert root.solution is not None, 'root must be solved to create CGLP'
        return np.asarray(root.solution, np.float64)

    def _solve_master(self, X, x_star, basis):
        """min x*.pi - pi0 over the rows X pi - pi0 >= 0 and the box, in the shifted columns
        z = (pi + 1, pi0 + R) >= 0.  Returns (pi, pi0, value, slack rows, basis), or None if the engine did not
        solve it (iteration limit)."""
        n, R = self.n, self.R
        lp = DenseLP()
        z = lp.addVariable('z', n + 1)
        lp.variablesUpper = np.concatenate([np.full(n, 2.0), [2.0 * R]])
        coefs = np.hstack([X, -np.ones((len(X), 1))])
        lp.addConstraint(Constraint(z, coefs, lower=X.sum(axis=1) - R), name='points')
        lp.objective = np.concatenate([x_star, [-1.0]])
        if basis is not None:
            lp.setBasisStatus(*basis)
        lp.primal()
        if lp.getStatusCode() != 0 and basis is not None:   # (stalled from the warm start: once more from scratch)
            lp._var_status = lp._row_status = None
            lp.primal()
        if lp.getStatusCode() != 0:
            return None
        sol = lp.primalVariableSolution['z']
        pi, pi0 = np.clip(sol[:n] - 1.0, -1.0, 1.0), float(sol[n] - R)
        return pi, pi0, float(x_star @ pi - pi0), lp._row_status == 1, (lp._var_status.copy(), lp._row_status.copy())

    def solve(self, x_star=None):
        """The inequality pi.x >= pi0 (a CyLPArray and a float), valid for every term, that x_star (default: the
        LP solution of the subtree's root) violates most under -1 <= pi <= 1, to within tol; (None, None) if no
        term is feasible or no valid cut met is violated by x_star."""
        n = self.n
        if x_star is None:
            assert self.bb is not None, 'a separator on a bare session needs x_star'
            x_star = self._default_point()
        else:
            assert isinstance(x_star, CyLPArray), 'x_star must be a CyLPArray'
            assert x_star.shape == (n,), \
                'x_star must have the same number of variables as the LP relaxations ' \
                'in the branch and bound tree this instance was created with'
            x_star = np.asarray(x_star, np.float64)
        stats = dict(rounds=0, leaf_lps=0, pivots=0, points=0, master_rows_dropped=0, master_rows=0,
                     final_min_margin=None, violation=None, leaves=len(self.leaf_ids), dropped=0, converged=False,
                     master_failed=False, leaf_lps_not_optimal=0)
        lam = self.stabilisation
        extended = self.screen or self.retry_cold or lam is not None
        if extended:
            stats.update(screened=0, in_moves=0, retried=0, retried_optimal=0)
        self.stats = stats
        self.timing = timing = dict(separation=0.0, master=0.0)
        if self._session is None:
            return None, None
        ses = self._session
        before = ses.stats()
        # without a row the master says pi = -sign(x*), pi0 = R: the first separation starts from there
        pi_m, pi0_m = np.where(x_star > 0, -1.0, 1.0), self.R
        X = np.zeros((0, n))
        seen = set()
        basis, best = None, None
        # in-out (stabilisation = lambda): the in-point is a certified cut, a round separates between it and the master's
        inp, inp_violation, in_steps, at_master = None, None, 0, False
        for _ in range(self.max_rounds):
            at_master = at_master or lam is None or inp is None
            if at_master:
                pi, pi0 = pi_m, pi0_m
            else:
                pi, pi0 = lam * pi_m + (1.0 - lam) * inp[0], lam * pi0_m + (1.0 - lam) * inp[1]
            scale = max(1.0, abs(pi0), float(np.abs(pi).sum()))
            options = {}
            if self.screen:   # (half the tolerance: a screened leaf is never among the violated rows)
                options['screen_tol'] = self.tol * scale / 2
            if self.retry_cold:
                options['retry_cold'] = True
            t0 = time.perf_counter()
            res = ses.eval(pi, pi0, tol=self.tol * scale, max_points=self.points_per_round, **options)
            timing['separation'] += time.perf_counter() - t0
            stats['rounds'] += 1
            if extended:
                stats['screened'] += res.get('screened', 0)
                stats['retried'] += res.get('retried', 0)
                stats['retried_optimal'] += res.get('retried_optimal', 0)
            if res['leaves'] == 0:
                break
            if res['not_optimal']:   # a leaf LP hit its iteration limit: this pi has no certified pi0; the best cut so far stands
                stats['leaf_lps_not_optimal'] = res['not_optimal']
                break
            # (pi, min_t h_t) is valid whatever the master knew
            h_min = res['min_margin'] + pi0
            violation = h_min - float(x_star @ pi)
            if best is None or violation > best[0]:
                best = (violation, pi.copy(), h_min)
            if lam is not None and (inp is None or violation > inp_violation):
                inp, inp_violation = (pi.copy(), h_min), violation
                stats['in_moves'] += 1
            stats['final_min_margin'] = res['min_margin']
            if res['min_margin'] >= -self.tol * scale:
                if at_master:
                    stats['converged'] = True
                    break
                # the separation point holds on every leaf: it is the in-point now, with its certified pi0
                if inp_violation != violation:
                    inp, inp_violation = (pi.copy(), h_min), violation
                    stats['in_moves'] += 1
                v_master = float(x_star @ pi_m - pi0_m)
                if -violation - v_master <= self.tol * max(1.0, abs(v_master)):
                    stats['converged'] = True
                    break
                in_steps += 1
                at_master = in_steps >= 3   # (closer by 1 - lambda a step: then at the master's point itself)
                continue
            new = []
            for k in range(len(res['ids'])):
                if res['h'][k] - pi0 >= -self.tol * scale:
                    break
                key = res['x'][k].tobytes()
                if key not in seen:
                    seen.add(key)
                    new.append(res['x'][k])
            if not new:
                if at_master:
                    break   # (every violated point is a row already: the master cannot move; the best cut stands)
                at_master = True   # (... of this separation point: the master's own may still give new ones)
                continue
            if len(X) + len(new) > self.max_master_rows and basis is not None:
                slack = basis[1] == 1
                stats['master_rows_dropped'] += int(slack.sum())
                for row in X[slack]:
                    seen.discard(row.tobytes())
                X, basis = X[~slack], (basis[0], basis[1][~slack])
            X = np.vstack([X, np.array(new)])
            if basis is not None:   # a new row enters with its slack basic
                basis = (basis[0], np.concatenate([basis[1], np.ones(len(new), np.int8)]))
            stats['points'] += len(new)
            t0 = time.perf_counter()
            master = self._solve_master(X, x_star, basis)
            timing['master'] += time.perf_counter() - t0
            if master is None:   # the engine gave the master up: the best valid cut met so far stands
                stats['master_failed'] = True
                break
            pi_m, pi0_m, _, _, basis = master
            in_steps, at_master = 0, False
        after = ses.stats()
        self.dropped_ids = ses.leaves(dropped=True)
        stats.update(leaf_lps=after['leaf_lps'] - before['leaf_lps'], pivots=after['pivots'] - before['pivots'],
                     iterations=after['iterations'] - before['iterations'], master_rows=len(X),
                     leaves=after['leaves'], dropped=after['dropped'],
                     violation=None if best is None else best[0])
        self.best_cut = None if best is None else (best[1], float(best[2]))
        if best is None or not best[0] > 0:
            return None, None
        return CyLPArray(best[1]), float(best[2])

    def close(self):
        if self._session is not None:
            self._session.close()
            self._session = None
