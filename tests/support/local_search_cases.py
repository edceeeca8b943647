"""The inputs of the local-search tests (tests/test_local_search_abi.py, tests/test_local_search_gpu.py): per shape one
instance of the generator, its points -- the primal heuristic's outputs from LP vertices, and those vertices scaled
by 0.8 and rounded down, which satisfy every packing row with room to spare (points() has the details) -- and what
the restatement makes of them, computed once per process.  Test infrastructure only."""
import functools

import numpy as np
from scipy.optimize import linprog

from simple_mip_solver_amd.generators import random_dense_milp_arrays
from tests.support import heuristic_reference as heur
from tests.support import local_search_reference as ref

# columns x rows -> (seed, points, max_moves): the seeds and caps were chosen on the CPU so that every shape with
# n >= 8 shows a pair move, a single move, a local optimum without a move and a capped point
# (test_the_points_exercise_every_outcome)
SHAPES = {(1, 1): (0, 65, 64), (2, 1): (0, 65, 64), (8, 4): (0, 65, 4), (40, 20): (0, 65, 6), (65, 9): (0, 65, 6),
          (257, 16): (0, 65, 6), (300, 150): (0, 65, 6), (1000, 700): (0, 4, 3)}


def vertices(A, b, c, l, u, count, seed):
    """LP vertices: the root LP's, then those of the same rows under costs scaled column by column by 0.5 .. 1.5."""
    rng = np.random.default_rng(7000 + seed)
    V = np.empty((count, len(c)))
    for k in range(count):
        ck = c if k == 0 else c * rng.uniform(0.5, 1.5, len(c))
        r = linprog(ck, A_ub=-A, b_ub=-b, bounds=list(zip(l, u)), method='highs-ds')
        assert r.status == 0, r.message
        V[k] = np.clip(r.x, l, u)
    return V


def points(A, b, c, l, u, ints, count, seed):
    """Per vertex three points: H, the heuristic's output from it; F, floor(0.8 * vertex) on the integer columns
    (0.8 * vertex on the others); S, the heuristic's output stopped one move short of H (its move cap one lower: where
    the missing move was a lift, the point is feasible and a single move is open; where it was a repair, a row is still
    violated).  Behind the first vertex's three comes P: the local optimum the search reaches from the first H -- an
    integral LP vertex, that of the leaf whose box fixes every column at it, and the heuristic returns it as it is."""
    groups = 1 + max(0, -(-(count - 4) // 3))
    V = vertices(A, b, c, l, u, groups, seed)
    J = np.asarray(ints, dtype=np.int64)
    X = []
    for k in range(groups):
        h, _, _, (repair, lift) = heur.round_repair_lift_one(A, b, c, l, u, ints, V[k])
        f = 0.8 * V[k]
        f[J] = np.floor(f[J])
        X += [h, f, heur.round_repair_lift_one(A, b, c, l, u, ints, V[k], max_moves=max(0, repair + lift - 1))[0]]
        if k == 0:
            p = ref.pair_search_one(A, b, c, l, u, ints, h, max_moves=64)[0]
            again = heur.round_repair_lift_one(A, b, c, l, u, ints, p)
            if again[2] == heur.FEASIBLE:   # (H itself may have ended stuck or capped: P is then H, and not feasible)
                assert np.array_equal(again[0], p) and again[3] == (0, 0)
            X.append(p)
    return np.array(X[:count])


def instance(n, m, kind='integer'):
    seed = SHAPES[(n, m)][0]
    A, b, c, l, u, ints = random_dense_milp_arrays(n, m, seed=seed)
    if kind == 'half':      # the odd columns continuous: the sums are no longer exact
        ints = list(range(0, n, 2))
    if kind == 'dyadic':    # rows in eighths, not integers
        rng = np.random.default_rng(9000 + seed)
        A = A - rng.integers(0, 8, A.shape) / 8.0
    return A, b, c, l, u, ints


@functools.lru_cache(maxsize=None)
def case(n, m, kind='integer'):
    """(A, b, c, l, u, ints, X, max_moves, want) with want = the restatement's (X', obj, status, moves)."""
    seed, count, max_moves = SHAPES[(n, m)]
    A, b, c, l, u, ints = instance(n, m, kind)
    X = points(A, b, c, l, u, ints, count, seed)
    want = ref.pair_search(A, b, c, l, u, ints, X, max_moves=max_moves)
    for a in (A, b, c, l, u, X) + want:
        a.setflags(write=False)
    return A, b, c, l, u, ints, X, max_moves, want
