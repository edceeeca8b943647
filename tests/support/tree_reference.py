"""Plain NumPy references for the queries on a recorded search tree (test infrastructure only): a node's bounds
from the record arrays of `mipx_tree_records` alone.  Nothing here uses the engine."""
import numpy as np


def lineage_bounds(rec, root_l, root_u, node):
    """(l, u) of one node by the walk the header describes: from the node upwards, the first branching met on a
    column's side is the one that stands -- ceil of the branching value for a right branch (the lower bound),
    floor for a left branch (the upper bound)."""
    lo, up = np.array(root_l, np.float64), np.array(root_u, np.float64)
    seen_lo, seen_up = set(), set()
    i = int(node)
    while i > 0:
        var, right, val = int(rec['bvar'][i]), int(rec['bdir'][i]), float(rec['bval'][i])
        if var >= 0:
            if right and var not in seen_lo:
                seen_lo.add(var)
                lo[var] = np.ceil(val)
            elif not right and var not in seen_up:
                seen_up.add(var)
                up[var] = np.floor(val)
        parent = int(rec['parent'][i])
        assert 0 <= parent < i, (i, parent)
        i = parent
    return lo, up


def all_bounds(rec, root_l, root_u):
    """(L, U), N x n, of every record: one pass in id order (a parent's id is below its child's), each node its
    parent's row with its own branching written over it.  The branching written last on the way down is the one
    met first on the way up, so this is lineage_bounds for every node at once (the tests compare the two)."""
    parent, var, right, val = rec['parent'], rec['bvar'], rec['bdir'], rec['bval']
    N, n = len(parent), len(root_l)
    L, U = np.empty((N, n)), np.empty((N, n))
    L[0], U[0] = root_l, root_u
    lower, upper = np.ceil(val), np.floor(val)
    for i in range(1, N):
        p = parent[i]
        assert 0 <= p < i, (i, p)
        L[i] = L[p]
        U[i] = U[p]
        if var[i] >= 0:
            if right[i]:
                L[i, var[i]] = lower[i]
            else:
                U[i, var[i]] = upper[i]
    return L, U
