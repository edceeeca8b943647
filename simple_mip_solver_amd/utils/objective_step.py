"""The step of a model's objective for the objective-step cutoff of the native search (include/mipx_objstep.h): the
value by which the objectives of any two integer-feasible points differ at least."""
import math

import numpy as np

from simple_mip_solver_amd.milp_instance import MILPInstance


def objective_step_of(bb_or_model, tol=1e-9):
    """The gcd of the nonzero |c_j| of a BranchAndBound's root problem or of a MILPInstance whose objective has
    integer costs on integer columns only: the objective of every integer-feasible point is then a multiple of it.

    Raises ValueError where no step follows from the costs alone -- a column with a cost that is not an integer
    column, a cost that is not an integer to `tol`, or an objective that is zero throughout; pass the step yourself
    (objective_step=<float>) if you know one, e.g. 0.5 for costs in halves."""
    if isinstance(bb_or_model, MILPInstance):
        lp, ints = bb_or_model.lp, bb_or_model.integerIndices
    else:
        assert hasattr(bb_or_model, 'root_node') and hasattr(bb_or_model, 'model'), \
            'objective_step_of takes a BranchAndBound or a MILPInstance'
        lp, ints = bb_or_model.root_node.lp, bb_or_model.model.integerIndices
    c = np.asarray(lp.objective, dtype=np.float64).reshape(-1)
    nz = np.flatnonzero(c != 0.0)
    if nz.size == 0:
        raise ValueError('objective_step=True: the objective is zero, it has no step; pass the step as a number')
    ints = set(int(j) for j in ints)
    loose = [int(j) for j in nz if int(j) not in ints]
    if loose:
        raise ValueError('objective_step=True: column %d has a cost and is not an integer column; pass the step as a '
                         'number if the objective has one' % loose[0])
    r = np.round(c[nz])
    if not np.all(np.isfinite(r)) or np.any(np.abs(c[nz] - r) > tol) or np.any(np.abs(r) > 2.0 ** 53):
        raise ValueError('objective_step=True: the costs are not integers; pass the step as a number if the objective '
                         'has one')
    g = 0
    for v in r:
        g = math.gcd(g, abs(int(v)))
    return float(g)
