"""ctypes binding of libmipx.so (include/mipx.h).  Fails loudly: there is no CPU fallback.

The library is built in-tree by `make -C simple_mip_solver_amd/csrc` (see __graft_entry__.build).
"""
import ctypes as C
import os
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('MIPX_LIB') or os.path.join(_HERE, 'csrc', 'libmipx.so')  # MIPX_LIB: a profiling build

MIPX_OK = 0
ERRORS = {-1: 'MIPX_EINVAL', -2: 'MIPX_ENODEV', -3: 'MIPX_EHIP', -4: 'MIPX_ETOOBIG',
          -5: 'MIPX_ENOMEM', -6: 'MIPX_EHOOK', -7: 'MIPX_EPEER'}

_dp = C.POINTER(C.c_double)
_i8p = C.POINTER(C.c_int8)
_i32p = C.POINTER(C.c_int32)
_vp = C.c_void_p

_lib = None


class MipxError(RuntimeError):
    pass


class TreeStats(C.Structure):
    """mipx_tree_stats (include/mipx.h)."""
    _fields_ = [('evaluated_nodes', C.c_int64), ('lp_solved', C.c_int64),
                ('probes_solved', C.c_int64), ('pivots', C.c_int64), ('open_nodes', C.c_int64),
                ('created_nodes', C.c_int64), ('steps', C.c_int64), ('primal_bound', C.c_double),
                ('dual_bound', C.c_double), ('gap', C.c_double), ('solve_seconds', C.c_double),
                ('kernel_ms', C.c_double), ('status', C.c_int32), ('has_solution', C.c_int32),
                ('dives', C.c_int64), ('pool_exhausted', C.c_int32), ('reserved', C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class CutParams(C.Structure):
    """mipx_cut_params (include/mipx.h)."""
    _fields_ = [('max_cut_generation_iterations', C.c_int32), ('max_nonzero_coefs', C.c_int32),
                ('max_cuts_per_node', C.c_int32), ('exact_tableau', C.c_int32),
                ('cutting_plane_progress_tolerance', C.c_double), ('min_cut_depth', C.c_double),
                ('cos_parallel', C.c_double), ('max_abs_coef', C.c_double), ('max_term', C.c_double),
                ('max_dual_bound', C.c_double), ('store_capacity', C.c_int64)]


CUT_TOTAL_KEYS = ('total_cut_generation_iterations', 'total_iterations_gmic_created',
                  'total_number_gmic_created', 'total_iterations_gmic_added', 'total_number_gmic_added',
                  'total_iterations_gmic_removed', 'total_number_gmic_removed')

class GlobalStats(C.Structure):
    """mipx_tree_global_stats_t (include/mipx.h)."""
    _fields_ = [('primal_bound', C.c_double), ('dual_bound', C.c_double), ('gap', C.c_double),
                ('evaluated_nodes', C.c_int64), ('lp_solved', C.c_int64), ('probes_solved', C.c_int64),
                ('pivots', C.c_int64), ('open_nodes', C.c_int64), ('exchanges', C.c_int64),
                ('nodes_sent', C.c_int64), ('nodes_received', C.c_int64), ('world', C.c_int32),
                ('incumbent_rank', C.c_int32)]


class ExchangeDecision(C.Structure):
    """mipx_exchange_decision (include/mipx.h)."""
    _fields_ = [('primal', C.c_double), ('dual', C.c_double), ('gap', C.c_double), ('sums', C.c_int64 * 4),
                ('open_nodes', C.c_int64), ('incumbent_rank', C.c_int32), ('done', C.c_int32),
                ('reason', C.c_int32), ('n_moves', C.c_int32), ('moves', C.c_int32 * 192)]


def source_hash():
    """sha256 over the kernel / engine sources next to libmipx.so (csrc/*.hip, *.h, in name order).  The
    profiling scripts store it beside the counters they collect; bench.py flags a counter-based roofline
    figure as stale when the sources have changed since (profiles/pmc_latest.json)."""
    import hashlib
    d = os.path.dirname(LIB_PATH)
    h = hashlib.sha256()
    for f in sorted(os.listdir(d)):
        if f.endswith(('.hip', '.h')):
            h.update(f.encode())
            h.update(open(os.path.join(d, f), 'rb').read())
    return h.hexdigest()


def exchange_record_len(n):
    return lib().mipx_exchange_record_len(int(n))


def exchange_decide(records, n, mip_gap=1e-4, allow_migration=True):
    """What every rank concludes from the gathered records ((world, record_len) array): dict."""
    records = np.ascontiguousarray(records, dtype=np.float64)
    world = records.shape[0]
    assert records.shape[1] == exchange_record_len(n)
    d = ExchangeDecision()
    rc = lib().mipx_exchange_decide(world, int(n), _ptr(records), float(mip_gap), int(bool(allow_migration)), C.byref(d))
    if rc != MIPX_OK:
        raise MipxError(f'mipx_exchange_decide failed: {ERRORS.get(rc, rc)}')
    return dict(primal=d.primal, dual=d.dual, gap=None if d.gap < 0 else d.gap, sums=list(d.sums),
                open_nodes=d.open_nodes, incumbent_rank=d.incumbent_rank, done=bool(d.done), reason=d.reason,
                moves=[tuple(d.moves[3 * k:3 * k + 3]) for k in range(d.n_moves)])


class CommOps(C.Structure):
    """mipx_comm_ops: host-buffer primitives of a custom communicator."""
    ALLGATHER = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)
    SEND = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t)
    RECV = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t)
    _fields_ = [('allgather', ALLGATHER), ('send', SEND), ('recv', RECV)]


TREE_STATUS = {0: 'unsolved', 1: 'optimal', 2: 'infeasible', 3: 'unbounded',
               4: 'stopped on iterations or time'}


TREE_HOOK = C.CFUNCTYPE(C.c_int, _vp)   # mipx_tree_hook

_i, _i64, _d, _sz = C.c_int, C.c_int64, C.c_double, C.c_size_t
_fp, _pvp = C.POINTER(C.c_float), C.POINTER(_vp)

# (restype, argtypes) of every function include/mipx.h declares, in its order; lib() applies them once
# (tests/test_abi.py checks them against the header's prototypes)
_SIGNATURES = {
    'mipx_abi_version': (_i, []),
    'mipx_device_count': (_i, []),
    'mipx_ctx_create': (_i, [_i, _pvp]),
    'mipx_ctx_destroy': (None, [_vp]),
    'mipx_last_error': (C.c_char_p, [_vp]),
    'mipx_ctx_sync': (_i, [_vp]),
    'mipx_problem_create': (_i, [_vp, _i, _i, _dp, _dp, _dp, _pvp]),
    'mipx_problem_destroy': (None, [_vp]),
    'mipx_lp_dive_batch': (_i, [_vp, _i] + [_vp] * 3 + [_i, _i, _vp, _i] + [_vp] * 3 + [_d] + [_vp] * 9),
    'mipx_lp_plunge_batch': (_i, [_vp, _i, _i] + [_vp] * 3 + [_i, _i, _vp, _i] + [_vp] * 3 + [_d] + [_vp] * 9),
    'mipx_problem_set_anchor': (_i, [_vp, _vp]),
    'mipx_lp_solve_batch': (_i, [_vp, _i] + [_vp] * 3 + [_i] + [_vp] * 7),
    'mipx_lp_solve_batch_cuts': (_i, [_vp, _i] + [_vp] * 3 + [_i, _vp, _vp, _i, _vp, _vp, _i] + [_vp] * 7),
    'mipx_lp_solve_batch_dev': (_i, [_vp, _i] + [_vp] * 3 + [_i] + [_vp] * 7),
    'mipx_lp_solve_multi': (_i, [_vp, _i, _i, _i] + [_vp] * 5 + [_i] + [_vp] * 6),
    'mipx_gomory_batch': (_i, [_vp, _i] + [_vp] * 5 + [_d] + [_vp] * 6),
    'mipx_cut_select_batch': (_i, [_vp, _i, _i, _i] + [_vp] * 4 + [_i, _d, _d, _d] + [_vp] * 4),
    'mipx_safe_cut_batch': (_i, [_vp, _i, _i, _vp, _vp, _i, _i, _d] + [_vp] * 7),
    'mipx_get_fraction_batch': (_i, [_vp, _i] + [_vp] * 5),
    'mipx_branch_score_batch': (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _i] + [_vp] * 6),
    'mipx_branch_score_batch_dev': (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _i] + [_vp] * 6),
    'mipx_dev_alloc': (_i, [_vp, _sz, _pvp]),
    'mipx_dev_free': (_i, [_vp, _vp]),
    'mipx_memcpy_h2d': (_i, [_vp, _vp, _vp, _sz]),
    'mipx_memcpy_d2h': (_i, [_vp, _vp, _vp, _sz]),
    'mipx_timer_start': (_i, [_vp]),
    'mipx_timer_stop': (_i, [_vp, _fp]),
    'mipx_debug_enable': (_i, [_vp]),
    'mipx_debug_read': (_i, [_vp, _vp, _vp, _vp]),
    'mipx_tree_create': (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i64, _pvp]),
    'mipx_tree_create_ex': (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i64, C.POINTER(CutParams), _pvp]),
    'mipx_tree_cut_stats': (_i, [_vp, _vp]),
    'mipx_tree_destroy': (None, [_vp]),
    'mipx_tree_solve': (_i, [_vp, _i64, _d, _d, _i, _i64, C.POINTER(TreeStats)]),
    'mipx_tree_get_stats': (_i, [_vp, C.POINTER(TreeStats)]),
    'mipx_tree_solution': (_i, [_vp, _vp]),
    'mipx_tree_set_primal_bound': (_i, [_vp, _d]),
    'mipx_tree_set_anchor_mode': (_i, [_vp, _i]),
    'mipx_tree_pseudo_costs': (_i, [_vp] + [_vp] * 4),
    'mipx_tree_set_pseudo_costs': (_i, [_vp] + [_vp] * 4),
    'mipx_tree_reanchor': (_i, [_vp, _i64]),
    'mipx_tree_peek_anchors': (_i64, [_vp, _i64, _vp]),
    'mipx_tree_anchor_table': (_i64, [_vp, _vp, _vp, _vp]),
    'mipx_tree_set_dive': (_i, [_vp, _i]),
    'mipx_tree_set_step_hook': (_i, [_vp, TREE_HOOK, _vp, _i]),
    'mipx_tree_peek_open': (_i64, [_vp, _i64] + [_vp] * 4),
    'mipx_tree_keep_shard': (_i, [_vp, _i, _i]),
    'mipx_tree_set_trace': (_i, [_vp, _i]),
    'mipx_tree_trace': (_i64, [_vp, _i64] + [_vp] * 4),
    'mipx_tree_kernel_ms': (_i, [_vp, _vp]),
    'mipx_tree_trace_cuts': (_i64, [_vp, _i64, _vp]),
    'mipx_tree_peek_cuts': (_i64, [_vp, _i64] + [_vp] * 4),
    'mipx_tree_cut_store': (_i64, [_vp, _i64, _vp, _vp]),
    'mipx_tree_cut_rows_per_node': (_i, [_vp]),
    'mipx_comm_unique_id': (_i, [C.c_char_p]),
    'mipx_comm_create_rccl': (_i, [_vp, C.c_char_p, _i, _i, _pvp]),
    'mipx_comm_create_custom': (_i, [_vp, _i, _i, C.POINTER(CommOps), _vp, _pvp]),
    'mipx_comm_destroy': (None, [_vp]),
    'mipx_comm_rank': (_i, [_vp]),
    'mipx_comm_size': (_i, [_vp]),
    'mipx_comm_allgather': (_i, [_vp, _vp, _vp, _sz]),
    'mipx_comm_barrier': (_i, [_vp]),
    'mipx_tree_set_comm': (_i, [_vp, _vp, _i]),
    'mipx_exchange_record_len': (_i, [_i]),
    'mipx_exchange_decide': (_i, [_i, _i, _vp, _d, _i, C.POINTER(ExchangeDecision)]),
    'mipx_tree_migrate_self': (_i64, [_vp, _i64]),
    'mipx_tree_exchange_record': (_i, [_vp, _vp]),
    'mipx_tree_global_stats': (_i, [_vp, C.POINTER(GlobalStats)]),
    'mipx_last_kernel_ms': (_i, [_vp, _fp]),
    'mipx_kernel_name': (_i, [_i, _i, C.c_char_p, _sz]),
}
SYMBOLS = list(_SIGNATURES)   # (tests/test_abi.py: the header declares exactly these)

# ... and those of include/mipx_spill.h (host spill of the frontier engine), which mipx.h includes
# (tests/test_node_spill_abi.py checks them against that header)
_SPILL_SIGNATURES = {
    'mipx_node_pack_batch': (_i, [_vp, _i, _i, _i] + [_vp] * 7 + [_i, _vp, _vp, _i64, _vp]),
    'mipx_node_unpack_batch': (_i, [_vp, _i, _i, _i] + [_vp] * 9 + [_i]),
    'mipx_tree_set_host_spill': (_i, [_vp, _i64]),
    'mipx_tree_spill_stats': (_i, [_vp, _vp]),
}
SPILL_SYMBOLS = list(_SPILL_SIGNATURES)
SPILL_STATS_KEYS = ('spilled', 'reloaded', 'on_host', 'host_bytes', 'peak_host_bytes', 'events', 'spill_ms',
                    'reload_ms')

# ... and those of include/mipx_cutmig.h (node migration with cut rows), which mipx.h includes
# (tests/test_cut_migration_cpu.py checks them against that header)
_CUTMIG_SIGNATURES = {
    'mipx_tree_set_cut_migration': (_i, [_vp, _i64]),
    'mipx_tree_cut_rows': (_i, [_vp, _i64, _vp, _vp, _vp]),
    'mipx_tree_cut_migration_stats': (_i, [_vp, _vp]),
}
CUTMIG_SYMBOLS = list(_CUTMIG_SIGNATURES)
CUTMIG_STATS_KEYS = ('nodes_sent_with_cuts', 'cut_rows_sent', 'cut_rows_received', 'region_rows_used')
# rows of the migration region that cut_migration=True / set_cut_migration(True) reserve
DEFAULT_CUT_MIGRATION_ROWS = 1 << 16

# ... and those of include/mipx_dualfn.h (the dual function of a search), which mipx.h includes
# (tests/test_dual_function_abi.py checks them against that header)
_DUALFN_SIGNATURES = {
    'mipx_tree_set_dual_record': (_i, [_vp, _i64, _i, _vp, _vp]),
    'mipx_tree_dual_function': (_i, [_vp, _i, _vp, _d, _vp]),
    'mipx_tree_dual_function_stats': (_i, [_vp, _vp]),
    'mipx_tree_dual_records': (_i64, [_vp, _i64] + [_vp] * 5),
}
DUALFN_SYMBOLS = list(_DUALFN_SIGNATURES)
DUALFN_STATS_KEYS = ('records', 'bytes', 'dropped', 'infeasible_leaves', 'penalized_resolves', 'leaves_without_term',
                     'record_ms', 'eval_ms')


# ... and those of include/mipx_treerec.h (the search tree kept as records), which mipx.h includes
# (tests/test_tree_record_abi.py checks them against that header)
_TREEREC_SIGNATURES = {
    'mipx_tree_set_tree_record': (_i, [_vp, _i]),
    'mipx_tree_records': (_i64, [_vp, _i64, _i64] + [_vp] * 9),
    'mipx_tree_node_bounds': (_i, [_vp, _i64, _vp, _vp, _vp]),
    'mipx_tree_node_solve': (_i, [_vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    'mipx_tree_record_stats': (_i, [_vp, _vp]),
}
TREEREC_SYMBOLS = list(_TREEREC_SIGNATURES)
TREEREC_STATS_KEYS = ('nodes', 'host_bytes', 'device_bytes', 'materialised', 'resolved', 'query_ms')
# flags of a record (MIPX_TR_* of the header)
TR_MIP_FEASIBLE, TR_HAS_CHILDREN, TR_CLOSED_AT_POP, TR_OPEN, TR_PROBED = 1, 2, 4, 8, 16

# ... and those of include/mipx_cglp.h (disjunctive cuts by batched leaf separation), which mipx.h includes
# (tests/test_cglp_abi.py checks them against that header)
_CGLP_SIGNATURES = {
    'mipx_tree_support_open': (_i, [_vp, _vp, _i64, _vp]),
    'mipx_tree_support_eval': (_i, [_vp, _vp, _d, _d, _i, _vp, _vp]),
    'mipx_tree_support_leaves': (_i64, [_vp, _i, _i64, _vp]),
    'mipx_tree_support_stats': (_i, [_vp, _vp]),
    'mipx_tree_support_close': (None, [_vp]),
}
CGLP_SYMBOLS = list(_CGLP_SIGNATURES)
CGLP_STATS_KEYS = ('leaves', 'dropped', 'evaluations', 'leaf_lps', 'iterations', 'pivots', 'device_bytes', 'kernel_ms',
                   'select_ms')
CGLP_HEAD = 8          # doubles in front of the rows of an evaluation's output block
CGLP_MAX_POINTS = 1024

# ... and those of include/mipx_restart.h (restart of a recorded search at another right-hand side), which
# mipx.h includes (tests/test_restart_abi.py checks them against that header)
_RESTART_SIGNATURES = {
    'mipx_tree_create_restart': (_i, [_vp, _vp, _pvp]),
    'mipx_tree_restart_stats': (_i, [_vp, _vp]),
    'mipx_tree_restart_seeds': (_i64, [_vp, _i64, _vp]),
}
RESTART_SYMBOLS = list(_RESTART_SIGNATURES)
RESTART_STATS_KEYS = ('skeleton', 'seeds', 'device_bytes', 'seed_ms', 'seeds_evaluated', 'seeds_infeasible',
                      'seeds_integral')

# ... and those of include/mipx_heur.h (the primal heuristic: round, repair and lift LP points), which mipx.h
# includes (tests/test_heuristic_abi.py checks them against that header)
_HEUR_SIGNATURES = {
    'mipx_round_repair_batch': (_i, [_vp, _i] + [_vp] * 4 + [_i, _d, _i] + [_vp] * 5),
    'mipx_tree_set_heuristic': (_i, [_vp, _i, _i, _i]),
    'mipx_tree_heuristic_stats': (_i, [_vp, _vp]),
}
HEUR_SYMBOLS = list(_HEUR_SIGNATURES)
HEUR_STATS_KEYS = ('points', 'feasible', 'stuck', 'capped', 'repair_moves', 'lift_moves', 'incumbents', 'kernel_us')
HEUR_STATUS = {0: 'feasible', 1: 'stuck', 2: 'capped', 3: 'skipped'}
# points per step that primal_heuristic=True / set_heuristic(True) take
DEFAULT_HEURISTIC_POINTS = 32

# ... and those of include/mipx_prop.h (node presolve: activity-based bound propagation), which mipx.h includes
# (tests/test_propagation_abi.py checks them against that header)
_PROP_SIGNATURES = {
    'mipx_propagate_batch': (_i, [_vp, _i] + [_vp] * 3 + [_i, _d, _d, _i] + [_vp] * 5),
    'mipx_tree_set_propagation': (_i, [_vp, _i, _i]),
    'mipx_tree_propagation_stats': (_i, [_vp, _vp]),
}
PROP_SYMBOLS = list(_PROP_SIGNATURES)
PROP_STATS_KEYS = ('nodes', 'tightened', 'infeasible', 'bounds_changed', 'rounds', 'capped', 'reserved', 'kernel_us')
PROP_STATUS = {0: 'unchanged', 1: 'tightened', 2: 'infeasible'}
# rounds that propagate=True / set_propagation(True) take, and the tolerance of the engine's runs
DEFAULT_PROPAGATION_ROUNDS = 8
PROPAGATION_TOL = 1e-6

# ... and those of include/mipx_rcfix.h (reduced-cost bound tightening from the row duals), which mipx.h includes
# (tests/test_reduced_cost_abi.py checks them against that header)
_RCFIX_SIGNATURES = {
    'mipx_reduced_cost_tighten_batch': (_i, [_vp, _i] + [_vp] * 4 + [_i, _d, _d, _d] + [_vp] * 5),
    'mipx_tree_set_reduced_cost': (_i, [_vp, _i]),
    'mipx_tree_reduced_cost_stats': (_i, [_vp, _vp]),
}
RCFIX_SYMBOLS = list(_RCFIX_SIGNATURES)
RCFIX_STATS_KEYS = ('nodes', 'tightened', 'cut_off', 'no_bound', 'bounds_changed', 'launches', 'reserved', 'kernel_us')
RCFIX_STATUS = {0: 'unchanged', 1: 'tightened', 2: 'cut_off', 3: 'no_bound'}
# the tolerances of the engine's runs: tol as the propagation's, dtol the reduced cost below which a column is skipped
RCFIX_TOL = 1e-6
RCFIX_DTOL = 1e-9

# ... those of include/mipx_lsearch.h (the pair-move local search behind the primal heuristic), which mipx.h includes
# (tests/test_local_search_abi.py checks them against that header)
_LSEARCH_SIGNATURES = {
    'mipx_pair_search_batch': (_i, [_vp, _i] + [_vp] * 4 + [_i, _d, _i] + [_vp] * 5),
    'mipx_tree_set_local_search': (_i, [_vp, _i]),
    'mipx_tree_local_search_stats': (_i, [_vp, _vp]),
}
LSEARCH_SYMBOLS = list(_LSEARCH_SIGNATURES)
LSEARCH_STATS_KEYS = ('points', 'improved', 'single_moves', 'pair_moves', 'capped', 'incumbents', 'reserved', 'kernel_us')
LSEARCH_STATUS = {0: 'local_opt', 1: 'capped', 2: 'not_feasible', 3: 'skipped'}
# moves per point that local_search=True / set_local_search(True) take at most
DEFAULT_LOCAL_SEARCH_MOVES = 64

# ... and those of include/mipx_objstep.h (the objective-step cutoff), which mipx.h includes
# (tests/test_objective_step_abi.py checks them against that header)
_OBJSTEP_SIGNATURES = {
    'mipx_tree_set_objective_step': (_i, [_vp, _d]),
    'mipx_tree_objective_step_stats': (_i, [_vp, _vp]),
}
OBJSTEP_SYMBOLS = list(_OBJSTEP_SIGNATURES)
OBJSTEP_STATS_KEYS = ('closed_at_pop', 'left_unbranched', 'launches') + tuple('reserved%d' % k for k in range(3, 8))

# ... and those of include/mipx_fixprop.h (the fix-and-propagate dive behind the primal heuristic), which mipx.h
# includes (tests/test_fix_propagate_abi.py checks them against that header)
_FIXPROP_SIGNATURES = {
    'mipx_fix_propagate_batch': (_i, [_vp, _i] + [_vp] * 4 + [_i, _d, _d, _i, _i] + [_vp] * 5),
    'mipx_tree_set_fix_propagate': (_i, [_vp, _i, _i]),
    'mipx_tree_fix_propagate_stats': (_i, [_vp, _vp]),
}
FIXPROP_SYMBOLS = list(_FIXPROP_SIGNATURES)
FIXPROP_STATS_KEYS = ('points', 'feasible', 'stuck', 'capped', 'fixings', 'tries', 'incumbents', 'kernel_us')
FIXPROP_STATUS = {0: 'feasible', 1: 'stuck', 2: 'capped', 3: 'skipped', 4: 'infeasible_box', 5: 'rows'}
# propagation calls per point that fix_propagate=True / set_fix_propagate(True) take at most, and the rounds of each
DEFAULT_FIX_PROPAGATE_TRIES = 256
DEFAULT_FIX_PROPAGATE_ROUNDS = 8

# ... and those of include/mipx_wrepair.h (the weighted row repair behind the primal heuristic), which mipx.h includes
# (tests/test_weighted_repair_abi.py checks them against that header)
_WREPAIR_SIGNATURES = {
    'mipx_weighted_repair_batch': (_i, [_vp, _i] + [_vp] * 4 + [_i, _d, _i] + [_vp] * 6),
    'mipx_tree_set_weighted_repair': (_i, [_vp, _i]),
    'mipx_tree_weighted_repair_stats': (_i, [_vp, _vp]),
}
WREPAIR_SYMBOLS = list(_WREPAIR_SIGNATURES)
WREPAIR_STATS_KEYS = ('points', 'feasible', 'capped', 'moves', 'bumps', 'incumbents', 'reserved6', 'kernel_us')
WREPAIR_STATUS = {0: 'feasible', 2: 'capped', 3: 'skipped'}
# moves and bumps per point that weighted_repair=True / set_weighted_repair(True) take at most
DEFAULT_WEIGHTED_REPAIR_STEPS = 256

# ... and those of include/mipx_cube.h (the cube search beside the primal heuristic), which mipx.h includes
# (tests/test_cube_search_abi.py checks them against that header)
_CUBE_SIGNATURES = {
    'mipx_cube_search_batch': (_i, [_vp, _i] + [_vp] * 4 + [_i, _d, _d, _d, _i] + [_vp] * 5),
    'mipx_tree_set_cube_search': (_i, [_vp, _i]),
    'mipx_tree_cube_search_stats': (_i, [_vp, _vp]),
}
CUBE_SYMBOLS = list(_CUBE_SIGNATURES)
CUBE_STATS_KEYS = ('points', 'found', 'none', 'columns', 'at_cap', 'incumbents', 'reserved6', 'kernel_us')
CUBE_STATUS = {0: 'found', 1: 'none', 3: 'skipped'}
# columns that cube_search=True / set_cube_search(True) enumerate at most, and the most that can be asked for
DEFAULT_CUBE_SEARCH_COLUMNS = 16
MAX_CUBE_SEARCH_COLUMNS = 20

# ... and those of include/mipx_complete.h (heuristic points completed over the continuous columns by a batched LP),
# which mipx.h includes (tests/test_completion_abi.py checks them against that header)
_COMPLETE_SIGNATURES = {
    'mipx_complete_batch': (_i, [_vp, _i] + [_vp] * 4 + [_i, _vp, _d, _vp] + [_vp] * 4),
    'mipx_tree_set_completion': (_i, [_vp, _i]),
    'mipx_tree_completion_stats': (_i, [_vp, _vp]),
}
COMPLETE_SYMBOLS = list(_COMPLETE_SIGNATURES)
COMPLETE_STATS_KEYS = ('points', 'completed', 'infeasible', 'failed', 'rescued', 'incumbents', 'pivots', 'kernel_us')
COMPLETE_STATUS = {0: 'completed', 1: 'infeasible', 2: 'limit', 3: 'skipped', 4: 'rejected'}
# the tolerance a completed point is checked with, in the engine and by default in complete_batch
DEFAULT_COMPLETION_TOL = 1e-6

# ... and those of include/mipx_lpdive.h (LP diving: fix a column, re-solve the batch, repeat), which mipx.h includes
# (tests/test_lp_dive_abi.py checks them against that header)
_LPDIVE_SIGNATURES = {
    'mipx_lpdive_batch': (_i, [_vp, _i] + [_vp] * 4 + [_i, _vp, _vp, _d, _i, _i] + [_vp] * 7),
    'mipx_tree_set_lpdive': (_i, [_vp, _i, _i, _i]),
    'mipx_tree_lpdive_stats': (_i, [_vp, _vp]),
}
LPDIVE_SYMBOLS = list(_LPDIVE_SIGNATURES)
LPDIVE_STATS_KEYS = ('points', 'feasible', 'infeasible', 'failed', 'moves', 'incumbents', 'pivots', 'kernel_us')
LPDIVE_STATUS = {0: 'feasible', 1: 'infeasible', 2: 'limit', 3: 'skipped', 4: 'rejected', 5: 'cutoff'}
LPDIVE_RULES = {'fractional': 0, 'coefficient': 1}
DEFAULT_LP_DIVE_ROUNDS = 64
MAX_LP_DIVE_ROUNDS = 1024

# ... and those of include/mipx_finish.h (test scaffolding: the device finish of a frontier step on a caller's data),
# which mipx.h includes (tests/test_finish_abi.py checks them against that header)
_FINISH_SIGNATURES = {
    'mipx_finish_step_batch': (_i, [_vp] + [_i] * 7 + [_vp] * 7 + [_i] + [_vp] * 14),
    'mipx_pc_apply_batch': (_i, [_vp, _i, _i] + [_vp] * 7),
}
FINISH_SYMBOLS = list(_FINISH_SIGNATURES)
# the records of csrc/finish_records.h (tests/support/finish_layout_check.cpp checks the offsets against the structs)
OPEN_ENTRY_DTYPE = np.dtype([('key', '<f8'), ('bval', '<f8'), ('slot', '<i4'), ('depth', '<i4'), ('bidx_dir', '<i4'),
                             ('anchor', '<i4')])
PC_SAMPLE_DTYPE = np.dtype([('var_dir', '<i4'), ('status', '<i4'), ('obj', '<f8'), ('bound', '<f8'), ('vc', '<f8')])
FINISH_SUMMARY_DTYPE = np.dtype([('host_path', '<i4'), ('n_open', '<i4'), ('n_dead', '<i4'), ('n_samples', '<i4'),
                                 ('unbounded', '<i4'), ('incumbent_pos', '<i4'), ('n_deferred', '<i4'), ('pad0', '<i4'),
                                 ('evaluated', '<i8'), ('dives', '<i8'), ('pivots', '<i8'), ('closed_min', '<f8'),
                                 ('primal', '<f8'), ('primal_before', '<f8'), ('pad', '<i8', (6,))])

# ... and those of include/mipx_cutround.h (test scaffolding: the kernels of a cut round on a caller's data), which
# mipx.h includes (tests/test_cut_round_abi.py checks them against that header)
_CUTROUND_SIGNATURES = {
    'mipx_cut_round_begin_batch': (_i, [_vp] + [_i] * 6 + [_d] * 2 + [_i] * 3 + [_vp] * 16),
    'mipx_cut_round_generate_batch': (_i, [_vp] + [_i] * 6 + [_d, _i] + [_d] * 3 + [_vp] * 22),
}
CUTROUND_SYMBOLS = list(_CUTROUND_SIGNATURES)
# ... and those of include/mipx_cglp_screen.h (support sessions that keep their duals: the dual screen of the leaves and
# the cold retry; mipx_support_screen_batch is test scaffolding), which mipx.h includes
# (tests/test_cglp_screen_abi.py checks them against that header)
_CGLP_SCREEN_SIGNATURES = {
    'mipx_tree_support_open_ex': (_i, [_vp, _vp, _i64, _i, _vp]),
    'mipx_tree_support_eval_ex': (_i, [_vp, _vp, _d, _d, _d, _i, _i, _vp, _vp, _vp]),
    'mipx_support_screen_batch': (_i, [_vp, _i64, _vp, _d, _d] + [_vp] * 8),
}
CGLP_SCREEN_SYMBOLS = list(_CGLP_SCREEN_SIGNATURES)
# ... and that of include/mipx_mir.h (MIR cuts: batched separation of base rows), which mipx.h includes
# (tests/test_mir_abi.py checks it against that header)
_MIR_SIGNATURES = {
    'mipx_mir_separate_batch': (_i, [_vp, _i] + [_vp] * 4 + [_i, _vp, _i, _vp, _i, _d, _d, _d] + [_vp] * 6),
}
MIR_SYMBOLS = list(_MIR_SIGNATURES)
# ... and that of include/mipx_cover.h (lifted knapsack cover cuts: batched separation from the rows), which mipx.h
# includes (tests/test_cover_abi.py checks it against that header)
_COVER_SIGNATURES = {
    'mipx_cover_separate_batch': (_i, [_vp, _i] + [_vp] * 4 + [_i, _vp, _i, _d] + [_vp] * 5),
}
COVER_SYMBOLS = list(_COVER_SIGNATURES)
# ... and those of include/mipx_clique.h (clique cuts: the conflict graph of the rows and the batched separation), which
# mipx.h includes (tests/test_clique_abi.py checks them against that header)
_CLIQUE_SIGNATURES = {
    'mipx_clique_graph': (_i, [_vp] * 4 + [_i] + [_vp] * 2),
    'mipx_clique_separate_batch': (_i, [_vp, _i] + [_vp] * 4 + [_i, _vp, _vp, _i, _d] + [_vp] * 5),
}
CLIQUE_SYMBOLS = list(_CLIQUE_SIGNATURES)
# ... and those of include/mipx_dualfn_batch.h (test scaffolding: the kernels of the dual function on a caller's
# records), which mipx.h includes (tests/test_dualfn_batch_abi.py checks them against that header)
_DUALFN_BATCH_SIGNATURES = {
    'mipx_dualfn_record_batch': (_i, [_vp, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _vp]),
    'mipx_dualfn_save_batch': (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp]),
    'mipx_dualfn_eval_batch': (_i, [_vp] + [_i] * 4 + [_vp] * 6 + [_i, _vp, _i, _i] + [_vp] * 3),
}
DUALFN_BATCH_SYMBOLS = list(_DUALFN_BATCH_SIGNATURES)
# ... and those of include/mipx_noderows.h (test scaffolding: the kernels that move node rows on a caller's pools),
# which mipx.h includes (tests/test_node_rows_abi.py checks them against that header)
_NODEROWS_SIGNATURES = {
    'mipx_noderows_children': (_i, [_vp] + [_i] * 6 + [_vp] * 2 + [_i] + [_vp] * 8 + [_i] + [_vp] * 5),
    'mipx_noderows_pack': (_i, [_vp, _i, _i, _i, _vp, _i] + [_vp] * 4),
    'mipx_noderows_unpack': (_i, [_vp, _i, _i, _i, _vp, _vp, _i] + [_vp] * 3),
    'mipx_noderows_gather_plain': (_i, [_vp] + [_i] * 4 + [_vp, _i] + [_vp] * 6),
    'mipx_noderows_lineage_bounds': (_i, [_vp, _i, _i, _i64] + [_vp] * 3 + [_i] + [_vp] * 7),
    'mipx_noderows_lineage_seed': (_i, [_vp, _i, _i, _i64] + [_vp] * 3 + [_i, _vp, _vp, _i64] + [_vp] * 6),
    'mipx_noderows_cut_lists': (_i, [_vp, _i, _i, _vp, _i] + [_vp] * 3),
    'mipx_noderows_cut_gather': (_i, [_vp, _i, _i, _vp, _i64] + [_vp] * 4),
    'mipx_noderows_cut_scatter': (_i, [_vp, _i, _i, _i64, _vp, _vp, _i64, _vp, _vp]),
    'mipx_noderows_cut_unpack_lists': (_i, [_vp, _i, _i, _vp, _vp, _i64, _i, _i] + [_vp] * 3),
    'mipx_noderows_spill_pack': (_i, [_vp] + [_i] * 4 + [_vp, _vp, _i] + [_vp] * 9 + [_i64, _vp]),
    'mipx_noderows_spill_unpack': (_i, [_vp] + [_i] * 4 + [_vp] * 5 + [_i] + [_vp] * 5),
    'mipx_noderows_spill_gather_rows': (_i, [_vp, _i, _i, _i, _vp, _i] + [_vp] * 6),
}
NODEROWS_SYMBOLS = list(_NODEROWS_SIGNATURES)
# ... and those of include/mipx_supportkernels.h (test scaffolding: the kernels behind a support evaluation on a caller's
# leaves), which mipx.h includes (tests/test_support_kernels_abi.py checks them against that header)
_SUPPORTKERNELS_SIGNATURES = {
    'mipx_support_select_batch': (_i, [_vp, _i64, _i, _i, _d, _d] + [_vp] * 12),
    'mipx_support_pack_batch': (_i, [_vp, _i64, _i, _d] + [_vp] * 8),
    'mipx_support_gather_batch': (_i, [_vp, _i64, _i64, _i, _i] + [_vp] * 7),
    'mipx_support_scatter_batch': (_i, [_vp, _i64, _i64, _i, _i, _vp, _i] + [_vp] * 15),
    'mipx_support_mark_batch': (_i, [_vp, _i64, _vp, _vp]),
}
SUPPORTKERNELS_SYMBOLS = list(_SUPPORTKERNELS_SIGNATURES)
MIR_STATUS = {0: 'cut', 1: 'no_trial', 2: 'shallow', 3: 'dynamism', 4: 'skipped'}   # MIPX_MIR_* of the header
COVER_STATUS = {0: 'cut', 1: 'no_cover', 2: 'shallow', 4: 'skipped'}   # MIPX_COVER_* of include/mipx_cover.h
CLIQUE_STATUS = {0: 'cut', 1: 'no_clique', 2: 'shallow', 4: 'skipped'}   # MIPX_CLIQUE_* of include/mipx_clique.h
# the defaults of the separation: divisor candidates per row (at most MIR_MAX_DIVISORS), the window of f0, the largest
# ratio of a cut's coefficients
MIR_MAX_DIVISORS = 64
DEFAULT_MIR_DIVISORS = 16
DEFAULT_MIR_F0_MIN = 0.05
DEFAULT_MIR_DYNAMISM = 1e6
SUPPORT_KEEP_DUALS = 1   # MIPX_SUPPORT_KEEP_DUALS
CGLP_EXTRA_KEYS = ('screened', 'lp_solved', 'min_screened_margin', 'retried', 'retried_optimal', 'screen_us')
CUT_FIELDS = ('rounds', 'it_created', 'n_created', 'it_added', 'n_added', 'it_removed', 'n_removed', 'ncut_out', 'stalled',
              'pool_n', 'slab_n', 'dropped')   # CutField of csrc/tree_kernels.hip.h: the rows of a round's state array


def lib():
    """Load libmipx.so; raise MipxError if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MipxError(
            f'{LIB_PATH} is missing: the HIP extension has not been built '
            f'(run `make -C {os.path.dirname(LIB_PATH)}` or __graft_entry__.build()). '
            'simple_mip_solver_amd has no CPU fallback.')
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in (list(_SIGNATURES.items()) + list(_SPILL_SIGNATURES.items()) +
                                      list(_CUTMIG_SIGNATURES.items()) + list(_DUALFN_SIGNATURES.items()) +
                                      list(_TREEREC_SIGNATURES.items()) + list(_CGLP_SIGNATURES.items()) +
                                      list(_RESTART_SIGNATURES.items()) + list(_HEUR_SIGNATURES.items()) +
                                      list(_PROP_SIGNATURES.items()) + list(_RCFIX_SIGNATURES.items()) +
                                      list(_LSEARCH_SIGNATURES.items()) + list(_OBJSTEP_SIGNATURES.items()) +
                                      list(_FIXPROP_SIGNATURES.items()) + list(_WREPAIR_SIGNATURES.items()) +
                                      list(_CUBE_SIGNATURES.items()) + list(_COMPLETE_SIGNATURES.items()) +
                                      list(_LPDIVE_SIGNATURES.items()) + list(_FINISH_SIGNATURES.items()) +
                                      list(_CUTROUND_SIGNATURES.items()) + list(_CGLP_SCREEN_SIGNATURES.items()) +
                                      list(_MIR_SIGNATURES.items()) + list(_DUALFN_BATCH_SIGNATURES.items()) +
                                      list(_NODEROWS_SIGNATURES.items()) + list(_SUPPORTKERNELS_SIGNATURES.items()) +
                                      list(_COVER_SIGNATURES.items()) + list(_CLIQUE_SIGNATURES.items())):
        f = getattr(L, name)
        f.restype, f.argtypes = restype, argtypes
    _lib = L
    return L


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_vp)


def _arr(a, dtype, shape=-1):
    """An optional input array as a contiguous `dtype` array of `shape` (None stays None)."""
    return None if a is None else np.ascontiguousarray(a, dtype).reshape(shape)


def comm_unique_id():
    """The 128 bytes rank 0 makes (ncclGetUniqueId) and the launcher hands to every rank."""
    buf = C.create_string_buffer(128)
    rc = lib().mipx_comm_unique_id(buf)
    if rc != MIPX_OK:
        raise MipxError(f'mipx_comm_unique_id failed: {ERRORS.get(rc, rc)} (librccl.so is needed for more than one GPU)')
    return buf.raw


class Comm:
    """The communicator of a multi-GPU search (mipx_comm): RCCL over xGMI, bound in libmipx.so.

    Comm(ctx, rank, world, unique_id=...) is the product; Comm(ctx, rank, world, allgather=, send=,
    recv=) runs the same protocol over caller-supplied host-buffer primitives (tests / rehearsals:
    allgather(send_bytes) -> list of world bytes objects, send(peer, bytes), recv(peer, nbytes) ->
    bytes)."""

    def __init__(self, ctx, rank, world, unique_id=None, allgather=None, send=None, recv=None):
        self.ctx, self.rank, self.world = ctx, int(rank), int(world)
        h = _vp()
        if unique_id is not None:
            assert len(unique_id) == 128, 'the RCCL unique id has 128 bytes'
            rc = lib().mipx_comm_create_rccl(ctx._h, unique_id, self.rank, self.world, C.byref(h))
            ctx.check(rc, 'mipx_comm_create_rccl')
            self.transport = 'rccl'
        else:
            self._err = None

            def guard(fn):
                def inner(*a):
                    try:
                        fn(*a)
                        return 0
                    except BaseException as e:   # never unwind through the C frames
                        self._err = e
                        return 1
                return inner

            def c_allgather(_user, sendp, recvp, nbytes):
                parts = allgather(C.string_at(sendp, nbytes))
                assert len(parts) == self.world and all(len(p) == nbytes for p in parts)
                C.memmove(recvp, b''.join(parts), nbytes * self.world)

            def c_send(_user, peer, bufp, nbytes):
                send(int(peer), C.string_at(bufp, nbytes))

            def c_recv(_user, peer, bufp, nbytes):
                data = recv(int(peer), int(nbytes))
                assert len(data) == nbytes
                C.memmove(bufp, data, nbytes)
            self._ops = CommOps(CommOps.ALLGATHER(guard(c_allgather)), CommOps.SEND(guard(c_send)),
                                CommOps.RECV(guard(c_recv)))
            rc = lib().mipx_comm_create_custom(None if ctx is None else ctx._h, self.rank, self.world,
                                               C.byref(self._ops), None, C.byref(h))
            if rc != MIPX_OK:
                raise MipxError(f'mipx_comm_create_custom failed: {ERRORS.get(rc, rc)}')
            self.transport = 'custom'
        self._h = h

    def check(self, rc, what):
        err, self._err = getattr(self, '_err', None), None
        if err is not None:
            raise err
        if self.ctx is not None:
            self.ctx.check(rc, what)
        elif rc != MIPX_OK:
            raise MipxError(f'{what} failed: {ERRORS.get(rc, rc)}')

    def allgather(self, arr):
        """All-gather of one equally sized array per rank (host, blocking): (world, ...) array."""
        arr = np.ascontiguousarray(arr)
        out = np.zeros((self.world,) + arr.shape, arr.dtype)
        self.check(lib().mipx_comm_allgather(self._h, _ptr(arr), _ptr(out), arr.nbytes), 'mipx_comm_allgather')
        return out

    def barrier(self):
        self.check(lib().mipx_comm_barrier(self._h), 'mipx_comm_barrier')

    def close(self):
        if getattr(self, '_h', None) and (self.ctx is None or getattr(self.ctx, '_h', None)):
            lib().mipx_comm_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """One GPU + one HIP stream (mipx_ctx)."""

    def __init__(self, device=0):
        L = lib()
        h = _vp()
        rc = L.mipx_ctx_create(int(device), C.byref(h))
        if rc != MIPX_OK:
            raise MipxError(
                f'mipx_ctx_create(device={device}) failed: {ERRORS.get(rc, rc)} '
                f'({L.mipx_device_count()} HIP devices visible). '
                'simple_mip_solver_amd needs an MI355X (gfx950); there is no CPU fallback.')
        self._h = h
        self.device = device

    def check(self, rc, what):
        if rc != MIPX_OK:
            msg = lib().mipx_last_error(self._h)
            raise MipxError(f'{what} failed: {ERRORS.get(rc, rc)}: '
                            f'{msg.decode() if msg else ""}')

    def sync(self):
        self.check(lib().mipx_ctx_sync(self._h), 'mipx_ctx_sync')

    def last_kernel_ms(self):
        """Device time of the LP launch inside the last solve_multi call (mipx_last_kernel_ms)."""
        ms = C.c_float()
        self.check(lib().mipx_last_kernel_ms(self._h, C.byref(ms)), 'mipx_last_kernel_ms')
        return float(ms.value)

    def timer_start(self):
        self.check(lib().mipx_timer_start(self._h), 'mipx_timer_start')

    def timer_stop(self):
        ms = C.c_float()
        self.check(lib().mipx_timer_stop(self._h, C.byref(ms)), 'mipx_timer_stop')
        return ms.value

    def alloc(self, nbytes):
        d = _vp()
        self.check(lib().mipx_dev_alloc(self._h, nbytes, C.byref(d)), 'mipx_dev_alloc')
        return d

    def free(self, d):
        self.check(lib().mipx_dev_free(self._h, d), 'mipx_dev_free')

    def h2d(self, d, arr):
        arr = np.ascontiguousarray(arr)
        self.check(lib().mipx_memcpy_h2d(self._h, d, _ptr(arr), arr.nbytes), 'mipx_memcpy_h2d')

    def d2h(self, arr, d):
        assert arr.flags['C_CONTIGUOUS']
        self.check(lib().mipx_memcpy_d2h(self._h, _ptr(arr), d, arr.nbytes), 'mipx_memcpy_d2h')

    def to_device(self, arr):
        arr = np.ascontiguousarray(arr)
        d = self.alloc(arr.nbytes)
        self.h2d(d, arr)
        return d

    def close(self):
        if getattr(self, '_h', None):
            lib().mipx_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def select_cuts(ctx, pi, pi0, x, max_nonzero_coefs, min_cut_depth, cos_parallel, max_abs_coef):
    """K3 for ONE node: (added pool positions in order, terminator code, depths)."""
    pi0 = np.ascontiguousarray(pi0, dtype=np.float64).reshape(-1)
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    K, n = len(pi0), len(x)
    kmax = max(K, 1)
    P = np.zeros((kmax, n)); P0 = np.zeros(kmax)
    if K:
        P[:K] = np.asarray(pi, dtype=np.float64).reshape(K, n); P0[:K] = pi0
    npool = np.array([K], np.int32); nadded = np.zeros(1, np.int32); added = np.zeros(kmax, np.int32)
    term = np.zeros(1, np.int32); depth = np.zeros(kmax)
    rc = lib().mipx_cut_select_batch(ctx._h, n, 1, kmax, _ptr(npool), _ptr(P), _ptr(P0), _ptr(x),
                                     int(min(max_nonzero_coefs, 2 ** 31 - 1)), float(min_cut_depth),
                                     float(cos_parallel), float(max_abs_coef), _ptr(nadded),
                                     _ptr(added), _ptr(term), _ptr(depth))
    ctx.check(rc, 'mipx_cut_select_batch')
    return added[:nadded[0]].copy(), int(term[0]), depth[:K].copy()


_EST = {None: 0, 'over': 1, 'under': 2}


def safe_cut_batch(ctx, pi, pi0, estimate='over', make_integer=False, max_term=1e3):
    """numerically_safe_cut for a batch of cuts on the device (mipx_safe_cut_batch): dict with
    safe_pi, safe_pi0, num, den (batch x (n+1): the coefficients, then the right-hand side),
    scaled_pi, scaled_pi0, nonzero."""
    pi = np.ascontiguousarray(pi, dtype=np.float64)
    if pi.ndim == 1:
        pi = pi[None]
    B, n = pi.shape
    pi0 = np.ascontiguousarray(pi0, dtype=np.float64).reshape(B)
    spi = np.zeros((B, n)); spi0 = np.zeros(B)
    num = np.zeros((B, n + 1)); den = np.zeros((B, n + 1))
    cpi = np.zeros((B, n)); cpi0 = np.zeros(B); nz = np.zeros(B, np.int32)
    rc = lib().mipx_safe_cut_batch(ctx._h, n, B, _ptr(pi), _ptr(pi0), _EST[estimate], int(bool(make_integer)),
                                   float(max_term), _ptr(spi), _ptr(spi0), _ptr(num), _ptr(den), _ptr(cpi),
                                   _ptr(cpi0), _ptr(nz))
    ctx.check(rc, 'mipx_safe_cut_batch')
    return dict(safe_pi=spi, safe_pi0=spi0, num=num, den=den, scaled_pi=cpi, scaled_pi0=cpi0, nonzero=nz)


def get_fraction_batch(ctx, x, max_term, estimate):
    """get_fraction on the device for arrays x, max_term and a list of estimates (None/'over'/'under'):
    (numerators, denominators) as int64 arrays."""
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    mt = np.ascontiguousarray(np.broadcast_to(np.asarray(max_term, dtype=np.float64), x.shape))
    est = np.ascontiguousarray([_EST[e] for e in estimate], dtype=np.int32)
    num = np.zeros(len(x)); den = np.zeros(len(x))
    rc = lib().mipx_get_fraction_batch(ctx._h, len(x), _ptr(x), _ptr(mt), _ptr(est), _ptr(num), _ptr(den))
    ctx.check(rc, 'mipx_get_fraction_batch')
    return num.astype(np.int64), den.astype(np.int64)


def node_pack_batch(ctx, root_l, root_u, l, u, vstat, ncut=None, cut_ids=None):
    """Compact records (include/mipx_spill.h) of count rows: (offsets int64 count + 1, bytes uint8).
    Cut mode when ncut / cut_ids (count x kcut) are given."""
    l = np.ascontiguousarray(l, np.float64)
    u = np.ascontiguousarray(u, np.float64)
    vstat = np.ascontiguousarray(vstat, np.int8)
    count, n = l.shape
    nv = vstat.shape[1]
    kcut = 0
    if cut_ids is not None:
        cut_ids = np.ascontiguousarray(cut_ids, np.int32)
        ncut = np.ascontiguousarray(ncut, np.int32)
        kcut = cut_ids.shape[1]
    rl = np.ascontiguousarray(root_l, np.float64)
    ru = np.ascontiguousarray(root_u, np.float64)
    off = np.zeros(count + 1, np.int64)
    used = np.zeros(1, np.int64)
    L = lib()
    rc = L.mipx_node_pack_batch(ctx._h, n, nv, count, _ptr(rl), _ptr(ru), _ptr(l), _ptr(u), _ptr(vstat),
                                _ptr(ncut) if kcut else None, _ptr(cut_ids) if kcut else None, kcut, _ptr(off),
                                None, 0, _ptr(used))
    if rc != -5:   # (MIPX_ENOMEM with cap 0: *used says how much room the records take)
        ctx.check(rc, 'mipx_node_pack_batch')
    out = np.zeros(max(int(used[0]), 1), np.uint8)
    rc = L.mipx_node_pack_batch(ctx._h, n, nv, count, _ptr(rl), _ptr(ru), _ptr(l), _ptr(u), _ptr(vstat),
                                _ptr(ncut) if kcut else None, _ptr(cut_ids) if kcut else None, kcut, _ptr(off),
                                _ptr(out), out.size, _ptr(used))
    ctx.check(rc, 'mipx_node_pack_batch')
    return off, out[:int(used[0])]


def node_unpack_batch(ctx, root_l, root_u, offsets, records, nv, kcut=0, cut_ids=None):
    """Rows (l, u, vstat[, ncut, cut_ids]) back from compact records; cut_ids (count x kcut) gives the values
    left beyond each node's ncut."""
    rl = np.ascontiguousarray(root_l, np.float64)
    ru = np.ascontiguousarray(root_u, np.float64)
    offsets = np.ascontiguousarray(offsets, np.int64)
    records = np.ascontiguousarray(records, np.uint8)
    n, count = rl.size, offsets.size - 1
    l, u = np.zeros((count, n)), np.zeros((count, n))
    v = np.zeros((count, nv), np.int8)
    ncut = np.zeros(count, np.int32)
    ids = np.zeros((count, max(kcut, 1)), np.int32) if cut_ids is None else np.array(cut_ids, np.int32)
    rc = lib().mipx_node_unpack_batch(ctx._h, n, nv, count, _ptr(rl), _ptr(ru), _ptr(offsets), _ptr(records),
                                      _ptr(l), _ptr(u), _ptr(v), _ptr(ncut) if kcut else None,
                                      _ptr(ids) if kcut else None, kcut)
    ctx.check(rc, 'mipx_node_unpack_batch')
    return (l, u, v, ncut, ids) if kcut else (l, u, v)


def branch_score_batch(ctx, integer_indices, x, status, rule=0, cost_l=None, cost_r=None, has_entry=None):
    """K4 on host buffers (mipx_branch_score_batch): x (batch, n), status (batch,) Clp codes, rule 0 most
    fractional / 1 pseudo cost (then cost_l, cost_r, has_entry: n each).  Returns dict of batch arrays
    branch_idx (-1: none), mip_feasible (bool), n_unprobed."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    B, n = x.shape
    ii = np.ascontiguousarray(integer_indices, dtype=np.int32).reshape(-1)
    st = np.ascontiguousarray(status, dtype=np.int32).reshape(B)
    cl, cr, he = _arr(cost_l, np.float64, n), _arr(cost_r, np.float64, n), _arr(has_entry, np.uint8, n)
    bidx = np.zeros(B, np.int32); mipf = np.zeros(B, np.int32); nun = np.zeros(B, np.int32)
    rc = lib().mipx_branch_score_batch(ctx._h, n, B, len(ii), _ptr(ii), _ptr(x), _ptr(st), int(rule), _ptr(cl),
                                       _ptr(cr), _ptr(he), _ptr(bidx), _ptr(mipf), _ptr(nun))
    ctx.check(rc, 'mipx_branch_score_batch')
    return dict(branch_idx=bidx, mip_feasible=mipf.astype(bool), n_unprobed=nun)


def branch_score_batch_dev(ctx, n, B, n_int, d_int_idx, d_x, d_status, rule, d_cost_l, d_cost_r, d_has_entry,
                           d_branch_idx, d_mip_feasible, d_n_unprobed):
    """mipx_branch_score_batch_dev: device pointers, asynchronous on the context stream."""
    rc = lib().mipx_branch_score_batch_dev(ctx._h, int(n), int(B), int(n_int), d_int_idx, d_x, d_status, int(rule),
                                           d_cost_l, d_cost_r, d_has_entry, d_branch_idx, d_mip_feasible, d_n_unprobed)
    ctx.check(rc, 'mipx_branch_score_batch_dev')


def finish_step_batch(ctx, step, fill=0x5a):
    """Test scaffolding (mipx_finish_step_batch, include/mipx_finish.h): the device finish on one synthetic step.
    step: a mapping with the scalars n, m, B, dive, rule, ask_count, ask_cap, primal; the K1 / K4 outputs status, bidx,
    mipf, nprobe, npiv, dvar, ddir, obj, bval, dval ((dive + 1) * B each); vout, slot, par_i, par_d, budget; the pool
    pool_l, pool_u, pool_v; with rule 1 the table cost_l, cost_r, has, times, own.  Nothing of step is written.
    Returns dict of summary (one FINISH_SUMMARY_DTYPE record), open, dead, samples, sample_keys (whole arrays, every
    byte `fill` where the kernels wrote nothing), pool_l, pool_u, pool_v, primal and the five table arrays."""
    n, m, B, dive, rule = (int(step[k]) for k in ('n', 'm', 'B', 'dive', 'rule'))
    P, per, nv = (dive + 1) * B, 2 * (1 + dive), n + m
    out_i = np.concatenate([_arr(step[k], np.int32, P) for k in ('status', 'bidx', 'mipf', 'nprobe', 'npiv', 'dvar', 'ddir')])
    out_d = np.concatenate([_arr(step[k], np.float64, P) for k in ('obj', 'bval', 'dval')])
    vout, slot = _arr(step['vout'], np.int8, (P, nv)), _arr(step['slot'], np.int32, B)
    par_i, par_d = _arr(step['par_i'], np.int32, (4, B)), _arr(step['par_d'], np.float64, (2, B))
    budget = _arr(step['budget'], np.int32, (B, per))
    pool_l, pool_u = (np.array(step[k], dtype=np.float64, order='C').reshape(-1, n) for k in ('pool_l', 'pool_u'))
    pool_v = np.array(step['pool_v'], dtype=np.int8, order='C').reshape(-1, nv)
    rows = pool_l.shape[0]
    assert pool_u.shape[0] == rows and pool_v.shape[0] == rows
    primal = np.array([step['primal']], np.float64)
    tab = [None] * 5
    if rule == 1:
        tab = [np.array(step[k], dtype=dt, order='C').reshape(sz) for k, dt, sz in
               (('cost_l', np.float64, n), ('cost_r', np.float64, n), ('has', np.uint8, n), ('times', np.int32, 2 * n),
                ('own', np.float64, 4 * n))]
    summary = np.full(FINISH_SUMMARY_DTYPE.itemsize, fill, np.uint8).view(FINISH_SUMMARY_DTYPE)
    open_ = np.full(per * B * OPEN_ENTRY_DTYPE.itemsize, fill, np.uint8).view(OPEN_ENTRY_DTYPE)
    dead = np.full(per * B * 4, fill, np.uint8).view(np.int32)
    samples = np.full(P * PC_SAMPLE_DTYPE.itemsize, fill, np.uint8).view(PC_SAMPLE_DTYPE)
    keys = np.full(P * 4, fill, np.uint8).view(np.int32)
    rc = lib().mipx_finish_step_batch(ctx._h, n, m, B, dive, rule, int(step['ask_count']), int(step['ask_cap']), _ptr(out_i),
                                      _ptr(out_d), _ptr(vout), _ptr(slot), _ptr(par_i), _ptr(par_d), _ptr(budget), rows,
                                      _ptr(pool_l), _ptr(pool_u), _ptr(pool_v), _ptr(primal), *(_ptr(a) for a in tab),
                                      _ptr(summary), _ptr(open_), _ptr(dead), _ptr(samples) if rule == 1 else None,
                                      _ptr(keys) if rule == 1 else None)
    ctx.check(rc, 'mipx_finish_step_batch')
    return dict(summary=summary[0], open=open_, dead=dead, samples=samples, sample_keys=keys, pool_l=pool_l, pool_u=pool_u,
                pool_v=pool_v, primal=primal[0], cost_l=tab[0], cost_r=tab[1], has=tab[2], times=tab[3], own=tab[4])


def pc_apply_batch(ctx, n, samples, cost_l, cost_r, has, times, own):
    """Test scaffolding (mipx_pc_apply_batch): the pseudo-cost recurrence on host-sent samples (PC_SAMPLE_DTYPE records,
    in list order).  Returns the table after them as (cost_l, cost_r, has, times, own); the inputs are not written."""
    samples = np.ascontiguousarray(samples, dtype=PC_SAMPLE_DTYPE).reshape(-1)
    keys = np.ascontiguousarray(samples['var_dir'], dtype=np.int32)
    tab = [np.array(a, dtype=dt, order='C').reshape(sz) for a, dt, sz in
           ((cost_l, np.float64, n), (cost_r, np.float64, n), (has, np.uint8, n), (times, np.int32, 2 * n), (own, np.float64, 4 * n))]
    rc = lib().mipx_pc_apply_batch(ctx._h, int(n), len(samples), _ptr(samples) if len(samples) else None,
                                   _ptr(keys) if len(samples) else None, *(_ptr(a) for a in tab))
    ctx.check(rc, 'mipx_pc_apply_batch')
    return tuple(tab)


def _filled(shape, dtype, fill):
    """An output array whose every byte is `fill`: what a kernel left alone still holds it."""
    a = np.empty(shape, dtype)
    a.view(np.uint8).reshape(-1)[:] = fill
    return a


def cut_round_begin_batch(ctx, rnd, fill=0x5a):
    """Test scaffolding (mipx_cut_round_begin_batch, include/mipx_cutround.h): cut_gather_state (with rnd['gather']) and
    cut_round_begin on one synthetic round.  rnd: a mapping with the scalars n, m0, kc, B, round, max_rounds,
    progress_tol, max_dual_bound, have_dump, gather; status, obj, mipf, y; vstat, ncut, ids, state (12 x B), obj_before,
    active, counters; with gather slot, pool_ncut, pool_ids.  Nothing of rnd is written.  Returns dict of vstat, ncut, ids,
    state, obj_before, active, counters (copies, as the kernels left them) and resolve, need_tab (every byte `fill` where
    the kernels wrote nothing)."""
    n, m0, kc, B = (int(rnd[k]) for k in ('n', 'm0', 'kc', 'B'))
    ms = m0 + kc
    gather = int(rnd['gather'])
    slot = pool_ncut = pool_ids = None
    rows = 0
    if gather:
        slot, pool_ncut = _arr(rnd['slot'], np.int32, B), _arr(rnd['pool_ncut'], np.int32)
        rows = len(pool_ncut)
        pool_ids = _arr(rnd['pool_ids'], np.int32, (rows, kc))
    status, obj, mipf = _arr(rnd['status'], np.int32, B), _arr(rnd['obj'], np.float64, B), _arr(rnd['mipf'], np.int32, B)
    y = _arr(rnd['y'], np.float64, (B, ms))
    out = dict(vstat=np.array(rnd['vstat'], dtype=np.int8, order='C').reshape(B, n + ms),
               ncut=np.array(rnd['ncut'], dtype=np.int32, order='C').reshape(B),
               ids=np.array(rnd['ids'], dtype=np.int32, order='C').reshape(B, kc),
               state=np.array(rnd['state'], dtype=np.int32, order='C').reshape(len(CUT_FIELDS), B),
               obj_before=np.array(rnd['obj_before'], dtype=np.float64, order='C').reshape(B),
               active=np.array(rnd['active'], dtype=np.int32, order='C').reshape(B),
               counters=np.array(rnd['counters'], dtype=np.int32, order='C').reshape(4),
               resolve=_filled(B, np.int32, fill), need_tab=_filled(B, np.int32, fill))
    rc = lib().mipx_cut_round_begin_batch(
        ctx._h, n, m0, kc, B, int(rnd['round']), int(rnd['max_rounds']), float(rnd['progress_tol']), float(rnd['max_dual_bound']),
        int(rnd['have_dump']), gather, rows, _ptr(slot), _ptr(pool_ncut), _ptr(pool_ids), _ptr(status), _ptr(obj), _ptr(mipf),
        _ptr(y), *(_ptr(out[k]) for k in ('vstat', 'ncut', 'ids', 'state', 'obj_before', 'active', 'counters', 'resolve', 'need_tab')))
    ctx.check(rc, 'mipx_cut_round_begin_batch')
    return out


def cut_round_generate_batch(problem, rnd, fill=0x5a):
    """Test scaffolding (mipx_cut_round_generate_batch): K2 in its slab form, pool_append, K3 over the pool lists and
    cut_round_apply on one synthetic round of `problem` (its A and b are the shared rows).  rnd: a mapping with the
    scalars B, kc, slab_rows, chunks, group, store_cap, max_term, max_nonzero_coefs, min_cut_depth, cos_parallel,
    max_abs_coef; T, idx, x, is_int, active; vstat, ncut, ids, state, pool_list, slab_pi, slab_pi0, store_pi, store_pi0,
    store_count, resolve, counters.  Nothing of rnd is written.  Returns dict of the in/out arrays as the kernels left them,
    k2_ncuts, k3_nadded, k3_added, k3_term (every byte `fill` where the kernels wrote nothing) and the chunks and group
    the launch ran with."""
    n, m0 = problem.n, problem.m
    B, kc, SR, cap = (int(rnd[k]) for k in ('B', 'kc', 'slab_rows', 'store_cap'))
    ms = m0 + kc
    T, idx = _arr(rnd['T'], np.float64, (B, ms, n)), _arr(rnd['idx'], np.int32, (B, 2 * n + ms))
    x, is_int, active = _arr(rnd['x'], np.float64, (B, n)), _arr(rnd['is_int'], np.uint8, n), _arr(rnd['active'], np.int32, B)
    shapes = (('vstat', np.int8, (B, n + ms)), ('ncut', np.int32, (B,)), ('ids', np.int32, (B, kc)),
              ('state', np.int32, (len(CUT_FIELDS), B)), ('pool_list', np.int32, (B, SR)), ('slab_pi', np.float64, (B, SR, n)),
              ('slab_pi0', np.float64, (B, SR)), ('store_pi', np.float64, (cap, n)), ('store_pi0', np.float64, (cap,)),
              ('store_count', np.int32, (1,)), ('resolve', np.int32, (B,)), ('counters', np.int32, (4,)))
    out = {k: np.array(rnd[k], dtype=dt, order='C').reshape(sh) for k, dt, sh in shapes}
    out.update(k2_ncuts=_filled(B, np.int32, fill), k3_nadded=_filled(B, np.int32, fill), k3_added=_filled((B, SR), np.int32, fill),
               k3_term=_filled(B, np.int32, fill))
    used = np.zeros(2, np.int32)
    rc = lib().mipx_cut_round_generate_batch(
        problem._h, B, kc, SR, int(rnd['chunks']), int(rnd['group']), cap, float(rnd['max_term']), int(rnd['max_nonzero_coefs']),
        float(rnd['min_cut_depth']), float(rnd['cos_parallel']), float(rnd['max_abs_coef']), _ptr(T), _ptr(idx), _ptr(x), _ptr(is_int),
        _ptr(active), *(_ptr(out[k]) for k, _, _ in shapes), _ptr(out['k2_ncuts']), _ptr(out['k3_nadded']), _ptr(out['k3_added']),
        _ptr(out['k3_term']), _ptr(used))
    problem.ctx.check(rc, 'mipx_cut_round_generate_batch')
    out['chunks'], out['group'] = int(used[0]), int(used[1])
    return out


def _inout(rec, key, dtype, shape, fill):
    """An in-and-out array of a scaffolding call: a copy of rec[key] where the caller sends one, else every byte `fill`."""
    if rec.get(key) is None:
        return _filled(shape, dtype, fill)
    return np.array(rec[key], dtype=dtype, order='C').reshape(shape)


def dualfn_record_batch(ctx, rec, fill=0x5a):
    """Test scaffolding (mipx_dualfn_record_batch, include/mipx_dualfn_batch.h): dualfn_record on synthetic entries.
    rec: a mapping with the scalars m, n, store_rows; A (m x n), c; src, lrow, dst (one per entry); y_src (rows of m),
    l, u (rows of n); optionally store_y, store_t to start from.  Nothing of rec is written.  Returns dict of store_y
    (store_rows x m) and store_t (whole arrays, every byte `fill` where the kernel wrote nothing and none was sent)."""
    m, n, rows = (int(rec[k]) for k in ('m', 'n', 'store_rows'))
    A, c = _arr(rec['A'], np.float64, (m, n)), _arr(rec['c'], np.float64, n)
    src, lrow, dst = _arr(rec['src'], np.int32), _arr(rec['lrow'], np.int32), _arr(rec['dst'], np.int64)
    count = len(src)
    assert len(lrow) == count and len(dst) == count
    y_src, l, u = _arr(rec['y_src'], np.float64, (-1, m)), _arr(rec['l'], np.float64, (-1, n)), _arr(rec['u'], np.float64, (-1, n))
    assert len(l) == len(u)
    out = dict(store_y=_inout(rec, 'store_y', np.float64, (rows, m), fill), store_t=_inout(rec, 'store_t', np.float64, (rows,), fill))
    rc = lib().mipx_dualfn_record_batch(ctx._h, m, n, _ptr(A), _ptr(c), count, _ptr(src), _ptr(lrow), _ptr(dst), len(y_src),
                                        _ptr(y_src), len(l), _ptr(l), _ptr(u), rows, _ptr(out['store_y']), _ptr(out['store_t']))
    ctx.check(rc, 'mipx_dualfn_record_batch')
    return out


def dualfn_save_batch(ctx, rec, fill=0x5a):
    """Test scaffolding (mipx_dualfn_save_batch): dualfn_save on synthetic entries.  rec: a mapping with the scalars n, nv,
    out_rows; lrow, vpos, dst (one per entry); l, u (rows of n), vstat (rows of nv int8); optionally out_l, out_u, out_v to
    start from.  Nothing of rec is written.  Returns dict of out_l, out_u (out_rows x n) and out_v (out_rows x nv), whole
    arrays, every byte `fill` where the kernel wrote nothing and none was sent."""
    n, nv, rows = (int(rec[k]) for k in ('n', 'nv', 'out_rows'))
    lrow, vpos, dst = _arr(rec['lrow'], np.int32), _arr(rec['vpos'], np.int32), _arr(rec['dst'], np.int64)
    count = len(lrow)
    assert len(vpos) == count and len(dst) == count
    l, u, vstat = _arr(rec['l'], np.float64, (-1, n)), _arr(rec['u'], np.float64, (-1, n)), _arr(rec['vstat'], np.int8, (-1, nv))
    assert len(l) == len(u)
    out = dict(out_l=_inout(rec, 'out_l', np.float64, (rows, n), fill), out_u=_inout(rec, 'out_u', np.float64, (rows, n), fill),
               out_v=_inout(rec, 'out_v', np.int8, (rows, nv), fill))
    rc = lib().mipx_dualfn_save_batch(ctx._h, n, nv, count, _ptr(lrow), _ptr(vpos), _ptr(dst), len(l), _ptr(l), _ptr(u), len(vstat),
                                      _ptr(vstat), rows, _ptr(out['out_l']), _ptr(out['out_u']), _ptr(out['out_v']))
    ctx.check(rc, 'mipx_dualfn_save_batch')
    return out


def dualfn_eval_batch(ctx, ev, k_tile=0, fill=0x5a):
    """Test scaffolding (mipx_dualfn_eval_batch): dualfn_gemm then dualfn_lineage, tile by tile, on synthetic records.
    ev: a mapping with Y (R x m), T (R), W (K x m), prec, order (R), lvl_off (nlvl + 1), leaf and the scalar bare.
    k_tile > 0 caps the tile of right-hand sides.  Nothing of ev is written.  Returns dict of V_gemm, V_max (K x R) and
    out (K), every byte `fill` where nothing was written."""
    Y = np.ascontiguousarray(ev['Y'], dtype=np.float64)
    R, m = Y.shape
    T, W = _arr(ev['T'], np.float64, R), _arr(ev['W'], np.float64, (-1, m))
    K = len(W)
    prec, order, lvl_off = _arr(ev['prec'], np.int32, R), _arr(ev['order'], np.int32, R), _arr(ev['lvl_off'], np.int32)
    leaf = _arr(ev['leaf'], np.int32)
    out = dict(V_gemm=_filled((K, R), np.float64, fill), V_max=_filled((K, R), np.float64, fill), out=_filled(K, np.float64, fill))
    rc = lib().mipx_dualfn_eval_batch(ctx._h, R, m, K, int(k_tile), _ptr(Y), _ptr(T), _ptr(W), _ptr(prec), _ptr(order), _ptr(lvl_off),
                                      len(lvl_off) - 1, _ptr(leaf) if len(leaf) else None, len(leaf), int(ev['bare']),
                                      _ptr(out['V_gemm']), _ptr(out['V_max']), _ptr(out['out']))
    ctx.check(rc, 'mipx_dualfn_eval_batch')
    return out


# ---- test scaffolding of include/mipx_noderows.h: the kernels that move node rows, on a caller's pools ------------------
# An array that is in and out must be a C-contiguous array of its C type: it is written in place, whole (the callers
# hand in sentinel-filled copies).  Inputs are converted.  A refused call raises MipxError and writes nothing.
def _io(a, dtype):
    assert a is None or (isinstance(a, np.ndarray) and a.dtype == np.dtype(dtype) and a.flags['C_CONTIGUOUS'] and a.flags['WRITEABLE'])
    return _ptr(a)


def noderows_children(ctx, n, m, src_l, src_u, x, vstat, parent_slot, parent_pos, var, child_slot, dst_l, dst_u, dst_v,
                      mstride=0, kc=0, src_ncut=None, src_ids=None, dst_ncut=None, dst_ids=None):
    """make_children (mipx_noderows_children): dst_* are written in place."""
    src_l, src_u, x = _arr(src_l, np.float64, (-1, n)), _arr(src_u, np.float64, (-1, n)), _arr(x, np.float64, (-1, n))
    vstat = _arr(vstat, np.int8, (len(x), -1))
    ps, pp, va, cs = (_arr(a, np.int32) for a in (parent_slot, parent_pos, var, child_slot))
    src_ncut, src_ids = _arr(src_ncut, np.int32), _arr(src_ids, np.int32)
    rc = lib().mipx_noderows_children(ctx._h, n, m, mstride, kc, len(ps), len(src_l), _ptr(src_l), _ptr(src_u), len(x), _ptr(x),
                                      _ptr(vstat), _ptr(src_ncut), _ptr(src_ids), _ptr(ps), _ptr(pp), _ptr(va), _ptr(cs),
                                      len(dst_l), _io(dst_l, np.float64), _io(dst_u, np.float64), _io(dst_v, np.int8),
                                      _io(dst_ncut, np.int32), _io(dst_ids, np.int32))
    ctx.check(rc, 'mipx_noderows_children')


def noderows_pack(ctx, n, nvs, slot, pool_l, pool_u, pool_v, msg):
    """pack_nodes (mipx_noderows_pack): msg (uint8, count x rowbytes) is written in place."""
    slot = _arr(slot, np.int32)
    pool_l, pool_u, pool_v = _arr(pool_l, np.float64, (-1, n)), _arr(pool_u, np.float64, (-1, n)), _arr(pool_v, np.int8, (-1, nvs))
    rc = lib().mipx_noderows_pack(ctx._h, n, nvs, len(slot), _ptr(slot), len(pool_l), _ptr(pool_l), _ptr(pool_u), _ptr(pool_v),
                                  _io(msg, np.uint8))
    ctx.check(rc, 'mipx_noderows_pack')


def noderows_unpack(ctx, n, nvs, slot, msg, pool_l, pool_u, pool_v):
    """unpack_nodes (mipx_noderows_unpack): the pool is written in place."""
    slot, msg = _arr(slot, np.int32), _arr(msg, np.uint8)
    rc = lib().mipx_noderows_unpack(ctx._h, n, nvs, len(slot), _ptr(slot), _ptr(msg), len(pool_l), _io(pool_l, np.float64),
                                    _io(pool_u, np.float64), _io(pool_v, np.int8))
    ctx.check(rc, 'mipx_noderows_unpack')


def noderows_gather_plain(ctx, n, m, nvs_pool, slot, pool_l, pool_u, pool_v, l, u, v):
    """gather_plain_nodes (mipx_noderows_gather_plain): l, u, v are written in place."""
    slot = _arr(slot, np.int32)
    pool_l, pool_u = _arr(pool_l, np.float64, (-1, n)), _arr(pool_u, np.float64, (-1, n))
    pool_v = _arr(pool_v, np.int8, (len(pool_l), -1))
    rc = lib().mipx_noderows_gather_plain(ctx._h, n, m, nvs_pool, len(slot), _ptr(slot), len(pool_l), _ptr(pool_l), _ptr(pool_u),
                                          _ptr(pool_v), _io(l, np.float64), _io(u, np.float64), _io(v, np.int8))
    ctx.check(rc, 'mipx_noderows_gather_plain')


def _lineage_in(n, nv, parent, vd, val, ids, root_l, root_u, root_v):
    parent, vd, val = _arr(parent, np.int32), _arr(vd, np.int32), _arr(val, np.float64)
    assert len(parent) == len(vd) == len(val)
    return parent, vd, val, _arr(ids, np.int64), _arr(root_l, np.float64, n), _arr(root_u, np.float64, n), _arr(root_v, np.int8, nv)


def noderows_lineage_bounds(ctx, n, nv, parent, vd, val, ids, root_l, root_u, root_v, out_l, out_u, out_v):
    """treerec_bounds on a mirror (mipx_noderows_lineage_bounds): out_* are written in place."""
    parent, vd, val, ids, rl, ru, rv = _lineage_in(n, nv, parent, vd, val, ids, root_l, root_u, root_v)
    rc = lib().mipx_noderows_lineage_bounds(ctx._h, n, nv, len(parent), _ptr(parent), _ptr(vd), _ptr(val), len(ids), _ptr(ids),
                                            _ptr(rl), _ptr(ru), _ptr(rv), _io(out_l, np.float64), _io(out_u, np.float64),
                                            _io(out_v, np.int8))
    ctx.check(rc, 'mipx_noderows_lineage_bounds')


def noderows_lineage_seed(ctx, n, nv, parent, vd, val, ids, slots, root_l, root_u, root_v, pool_l, pool_u, pool_v):
    """restart_seed on a mirror (mipx_noderows_lineage_seed): the pool (capacity = its rows) is written in place."""
    parent, vd, val, ids, rl, ru, rv = _lineage_in(n, nv, parent, vd, val, ids, root_l, root_u, root_v)
    slots = _arr(slots, np.int32)
    assert len(slots) == len(ids)
    rc = lib().mipx_noderows_lineage_seed(ctx._h, n, nv, len(parent), _ptr(parent), _ptr(vd), _ptr(val), len(ids), _ptr(ids),
                                          _ptr(slots), len(pool_l), _ptr(rl), _ptr(ru), _ptr(rv), _io(pool_l, np.float64),
                                          _io(pool_u, np.float64), _io(pool_v, np.int8))
    ctx.check(rc, 'mipx_noderows_lineage_seed')


def noderows_cut_lists(ctx, kc, slot, pool_ncut, pool_ids, lists):
    """cutmig_lists (mipx_noderows_cut_lists): lists (count x (1 + kc) int32) is written in place."""
    slot, pool_ncut, pool_ids = _arr(slot, np.int32), _arr(pool_ncut, np.int32), _arr(pool_ids, np.int32, (-1, kc))
    rc = lib().mipx_noderows_cut_lists(ctx._h, kc, len(slot), _ptr(slot), len(pool_ncut), _ptr(pool_ncut), _ptr(pool_ids),
                                       _io(lists, np.int32))
    ctx.check(rc, 'mipx_noderows_cut_lists')


def noderows_cut_gather(ctx, n, src, store_pi, store_pi0, tab_pi, tab_pi0):
    """cutmig_gather (mipx_noderows_cut_gather): the table is written in place."""
    src, store_pi, store_pi0 = _arr(src, np.int32), _arr(store_pi, np.float64, (-1, n)), _arr(store_pi0, np.float64)
    rc = lib().mipx_noderows_cut_gather(ctx._h, n, len(src), _ptr(src), len(store_pi0), _ptr(store_pi), _ptr(store_pi0),
                                        _io(tab_pi, np.float64), _io(tab_pi0, np.float64))
    ctx.check(rc, 'mipx_noderows_cut_gather')


def noderows_cut_scatter(ctx, n, base, tab_pi, tab_pi0, store_pi, store_pi0):
    """cutmig_scatter (mipx_noderows_cut_scatter): the store is written in place."""
    tab_pi, tab_pi0 = _arr(tab_pi, np.float64, (-1, n)), _arr(tab_pi0, np.float64)
    rc = lib().mipx_noderows_cut_scatter(ctx._h, n, len(tab_pi0), int(base), _ptr(tab_pi), _ptr(tab_pi0), len(store_pi0),
                                         _io(store_pi, np.float64), _io(store_pi0, np.float64))
    ctx.check(rc, 'mipx_noderows_cut_scatter')


def noderows_cut_unpack_lists(ctx, kc, slot, lists, base, ctab, pool_ncut, pool_ids):
    """cutmig_unpack_lists (mipx_noderows_cut_unpack_lists): the pool's lists are written in place; returns bad."""
    slot, lists = _arr(slot, np.int32), _arr(lists, np.int32, (-1, 1 + kc))
    bad = np.full(1, -1, np.int32)
    rc = lib().mipx_noderows_cut_unpack_lists(ctx._h, kc, len(slot), _ptr(slot), _ptr(lists), int(base), int(ctab), len(pool_ncut),
                                              _io(pool_ncut, np.int32), _io(pool_ids, np.int32), _ptr(bad))
    ctx.check(rc, 'mipx_noderows_cut_unpack_lists')
    return int(bad[0])


def noderows_spill_pack(ctx, n, nv, kc, count, root_l, root_u, l, u, v, ncut, ids, slot, node_id, out_offsets, out_bytes):
    """spill_count, spill_scan, spill_pack (mipx_noderows_spill_pack): out_offsets (count + 1 int64) and out_bytes
    (uint8, its size is the capacity) are written in place; returns the records' total bytes."""
    rl, ru = _arr(root_l, np.float64, n), _arr(root_u, np.float64, n)
    l, u, v = _arr(l, np.float64, (-1, n)), _arr(u, np.float64, (-1, n)), _arr(v, np.int8, (-1, nv))
    ncut, ids, slot, node_id = _arr(ncut, np.int32), _arr(ids, np.int32), _arr(slot, np.int32), _arr(node_id, np.int64)
    used = np.zeros(1, np.int64)
    rc = lib().mipx_noderows_spill_pack(ctx._h, n, nv, kc, count, _ptr(rl), _ptr(ru), len(l), _ptr(l), _ptr(u), _ptr(v), _ptr(ncut),
                                        _ptr(ids), _ptr(slot), _ptr(node_id), _io(out_offsets, np.int64), _io(out_bytes, np.uint8),
                                        out_bytes.size, _ptr(used))
    ctx.check(rc, 'mipx_noderows_spill_pack')
    return int(used[0])


def noderows_spill_unpack(ctx, n, nv, kc, root_l, root_u, offsets, records, slot, l, u, v, ncut=None, ids=None):
    """spill_unpack (mipx_noderows_spill_unpack): the pool's arrays are written in place."""
    rl, ru = _arr(root_l, np.float64, n), _arr(root_u, np.float64, n)
    offsets, records, slot = _arr(offsets, np.int64), _arr(records, np.uint8), _arr(slot, np.int32)
    rc = lib().mipx_noderows_spill_unpack(ctx._h, n, nv, kc, len(offsets) - 1, _ptr(rl), _ptr(ru), _ptr(offsets), _ptr(records),
                                          _ptr(slot), len(l), _io(l, np.float64), _io(u, np.float64), _io(v, np.int8),
                                          _io(ncut, np.int32), _io(ids, np.int32))
    ctx.check(rc, 'mipx_noderows_spill_unpack')


def noderows_spill_gather_rows(ctx, n, nv, slot, src_l, src_u, src_v, l, u, v):
    """spill_gather_rows (mipx_noderows_spill_gather_rows): l, u, v are written in place."""
    slot = _arr(slot, np.int32)
    src_l, src_u, src_v = _arr(src_l, np.float64, (-1, n)), _arr(src_u, np.float64, (-1, n)), _arr(src_v, np.int8, (-1, nv))
    rc = lib().mipx_noderows_spill_gather_rows(ctx._h, n, nv, len(slot), _ptr(slot), len(src_l), _ptr(src_l), _ptr(src_u),
                                               _ptr(src_v), _io(l, np.float64), _io(u, np.float64), _io(v, np.int8))
    ctx.check(rc, 'mipx_noderows_spill_gather_rows')


# ---- test scaffolding of include/mipx_supportkernels.h: the kernels behind a support evaluation, on a caller's leaves ----
# The sizes are the caller's (T and count are handed on as given); the in-and-out arrays are written in place, as above.
def support_select_batch(ctx, T, n, P, pi0, tol, ids, status, obj, x, iters, npivots, margin, cand_m, cand_id, cand_t,
                         seg_sum, block):
    """support_select and support_select_merge (mipx_support_select_batch): margin .. block are written in place."""
    ids, status, obj, x = _arr(ids, np.int64), _arr(status, np.int32), _arr(obj, np.float64), _arr(x, np.float64)
    iters, npivots = _arr(iters, np.int32), _arr(npivots, np.int32)
    rc = lib().mipx_support_select_batch(ctx._h, T, n, P, float(pi0), float(tol), _ptr(ids), _ptr(status), _ptr(obj), _ptr(x),
                                         _ptr(iters), _ptr(npivots), _io(margin, np.float64), _io(cand_m, np.float64),
                                         _io(cand_id, np.int32), _io(cand_t, np.int32), _io(seg_sum, np.float64),
                                         _io(block, np.float64))
    ctx.check(rc, 'mipx_support_select_batch')


def support_pack_batch(ctx, T, mode, pi0, skip, status, bound, seg_count, seg_min, packed, info_count, info_min):
    """support_pack_count and support_pack (mipx_support_pack_batch): seg_count, seg_min, packed and the two one-entry
    arrays info_count (int32) and info_min (float64) are written in place."""
    skip, status, bound = _arr(skip, np.uint8), _arr(status, np.int32), _arr(bound, np.float64)
    rc = lib().mipx_support_pack_batch(ctx._h, T, mode, float(pi0), _ptr(skip), _ptr(status), _ptr(bound), _io(seg_count, np.int32),
                                       _io(seg_min, np.float64), _io(packed, np.int32), _io(info_count, np.int32),
                                       _io(info_min, np.float64))
    ctx.check(rc, 'mipx_support_pack_batch')


def support_gather_batch(ctx, count, T, n, m, packed, l, u, v, pl, pu, pv_in):
    """support_gather (mipx_support_gather_batch): pl, pu, pv_in are written in place; v = None is the cold gather."""
    packed, l, u, v = _arr(packed, np.int32), _arr(l, np.float64), _arr(u, np.float64), _arr(v, np.int8)
    rc = lib().mipx_support_gather_batch(ctx._h, count, T, n, m, _ptr(packed), _ptr(l), _ptr(u), _ptr(v), _io(pl, np.float64),
                                         _io(pu, np.float64), _io(pv_in, np.int8))
    ctx.check(rc, 'mipx_support_gather_batch')


def support_scatter_batch(ctx, count, T, n, m, packed, add, px, pobj, py, pv_out, pstatus, piters, pnpivots, x, obj, y, v,
                          status, iters, npivots, has_y):
    """support_scatter (mipx_support_scatter_batch): x .. has_y are written in place."""
    packed, px, pobj, py = _arr(packed, np.int32), _arr(px, np.float64), _arr(pobj, np.float64), _arr(py, np.float64)
    pv_out, pstatus, piters, pnpivots = _arr(pv_out, np.int8), _arr(pstatus, np.int32), _arr(piters, np.int32), _arr(pnpivots, np.int32)
    rc = lib().mipx_support_scatter_batch(ctx._h, count, T, n, m, _ptr(packed), int(add), _ptr(px), _ptr(pobj), _ptr(py),
                                          _ptr(pv_out), _ptr(pstatus), _ptr(piters), _ptr(pnpivots), _io(x, np.float64),
                                          _io(obj, np.float64), _io(y, np.float64), _io(v, np.int8), _io(status, np.int32),
                                          _io(iters, np.int32), _io(npivots, np.int32), _io(has_y, np.uint8))
    ctx.check(rc, 'mipx_support_scatter_batch')


def support_mark_batch(ctx, T, status, has_y):
    """support_mark (mipx_support_mark_batch): has_y is written in place."""
    status = _arr(status, np.int32)
    rc = lib().mipx_support_mark_batch(ctx._h, T, _ptr(status), _io(has_y, np.uint8))
    ctx.check(rc, 'mipx_support_mark_batch')


def solve_multi(ctx, A, b, c, l, u, max_iter=0):
    """Root relaxations of `batch` independent problems of one shape (cold start)."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    B, m, n = A.shape
    b = np.ascontiguousarray(b, dtype=np.float64).reshape(B, m)
    c = np.ascontiguousarray(c, dtype=np.float64).reshape(B, n)
    l = np.ascontiguousarray(l, dtype=np.float64).reshape(B, n)
    u = np.ascontiguousarray(u, dtype=np.float64).reshape(B, n)
    status = np.zeros(B, np.int32); obj = np.zeros(B); x = np.zeros((B, n))
    vout = np.zeros((B, n + m), np.int8); iters = np.zeros(B, np.int32); npiv = np.zeros(B, np.int32)
    rc = lib().mipx_lp_solve_multi(ctx._h, m, n, B, _ptr(A), _ptr(b), _ptr(c), _ptr(l), _ptr(u),
                                   int(max_iter), _ptr(status), _ptr(obj), _ptr(x), _ptr(vout),
                                   _ptr(iters), _ptr(npiv))
    ctx.check(rc, 'mipx_lp_solve_multi')
    return dict(status=status, obj=obj, x=x, vstat=vout, iters=iters, npivots=npiv)


class Problem:
    """(A, b, c) of one tree resident in HBM (mipx_problem)."""

    def __init__(self, ctx, A, b, c):
        self.ctx = ctx
        A = np.ascontiguousarray(A, dtype=np.float64)
        if A.ndim != 2:
            A = A.reshape(-1, len(c))
        self.m, self.n = A.shape
        b = np.ascontiguousarray(b, dtype=np.float64).reshape(self.m)
        c = np.ascontiguousarray(c, dtype=np.float64).reshape(self.n)
        h = _vp()
        rc = lib().mipx_problem_create(ctx._h, self.m, self.n, A.ctypes.data_as(_dp),
                                       b.ctypes.data_as(_dp), c.ctypes.data_as(_dp), C.byref(h))
        ctx.check(rc, f'mipx_problem_create(m={self.m}, n={self.n})')
        self._h = h

    def set_anchor(self, vstat):
        """Anchor warm starts at the tableau of basis `vstat` (None switches it off)."""
        v = _arr(vstat, np.int8, self.n + self.m)
        self.ctx.check(lib().mipx_problem_set_anchor(self._h, _ptr(v)), 'mipx_problem_set_anchor')

    def solve_batch(self, l, u, vstat=None, max_iter=0):
        """Host-buffer batched LP relaxation; returns dict like the oracle's."""
        n, m = self.n, self.m
        l = np.ascontiguousarray(l, dtype=np.float64).reshape(-1, n)
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(-1, n)
        B = l.shape[0]
        assert u.shape[0] == B
        vstat = _arr(vstat, np.int8, (B, n + m))
        status = np.zeros(B, np.int32)
        obj = np.zeros(B, np.float64)
        x = np.zeros((B, n), np.float64)
        y = np.zeros((B, m), np.float64)
        vout = np.zeros((B, n + m), np.int8)
        iters = np.zeros(B, np.int32)
        npiv = np.zeros(B, np.int32)
        rc = lib().mipx_lp_solve_batch(self._h, B, _ptr(l), _ptr(u), _ptr(vstat), int(max_iter),
                                       _ptr(status), _ptr(obj), _ptr(x), _ptr(y), _ptr(vout),
                                       _ptr(iters), _ptr(npiv))
        self.ctx.check(rc, 'mipx_lp_solve_batch')
        return dict(status=status, obj=obj, x=x, y=y, vstat=vout, iters=iters, npivots=npiv)

    def solve_batch_cuts(self, l, u, vstat, cut_pi, cut_pi0, cut_lists, max_iter=0, kc=64):
        """Node LPs with per-node cut rows (mipx_lp_solve_batch_cuts): cut_lists[k] = ids (rows of
        cut_pi / cut_pi0) node k carries after the m shared rows.  vstat rows: n + m + len(cut_lists[k])
        codes each (a list of arrays) or None.  Returns dict like solve_batch; y and vstat are lists of
        per-node arrays over the node's own rows."""
        n, m = self.n, self.m
        l = np.ascontiguousarray(l, dtype=np.float64).reshape(-1, n)
        B = l.shape[0]
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(B, n)
        cut_pi = np.ascontiguousarray(cut_pi, dtype=np.float64).reshape(-1, n)
        cut_pi0 = np.ascontiguousarray(cut_pi0, dtype=np.float64).reshape(-1)
        ncut = np.array([len(c) for c in cut_lists], np.int32)
        ids = np.zeros((B, kc), np.int32)
        for k, c in enumerate(cut_lists):
            ids[k, :len(c)] = c
        M = m + kc
        vin = None
        if vstat is not None:
            vin = np.zeros((B, n + M), np.int8)
            for k in range(B):
                vin[k, :n + m + ncut[k]] = vstat[k]
        status = np.zeros(B, np.int32); obj = np.zeros(B); x = np.zeros((B, n)); y = np.zeros((B, M))
        vout = np.zeros((B, n + M), np.int8); iters = np.zeros(B, np.int32); npiv = np.zeros(B, np.int32)
        rc = lib().mipx_lp_solve_batch_cuts(self._h, B, _ptr(l), _ptr(u), _ptr(vin), len(cut_pi0), _ptr(cut_pi),
                                            _ptr(cut_pi0), kc, _ptr(ncut), _ptr(ids), int(max_iter), _ptr(status),
                                            _ptr(obj), _ptr(x), _ptr(y), _ptr(vout), _ptr(iters), _ptr(npiv))
        self.ctx.check(rc, 'mipx_lp_solve_batch_cuts')
        return dict(status=status, obj=obj, x=x, iters=iters, npivots=npiv,
                    y=[y[k, :m + ncut[k]].copy() for k in range(B)],
                    vstat=[vout[k, :n + m + ncut[k]].copy() for k in range(B)])

    def dive_batch(self, l, u, vstat, rule, integer_indices, cost_l=None, cost_r=None, has_entry=None,
                   cutoff=float('inf'), max_iter=0, depth=1):
        """Node LPs with the in-place dive (mipx_lp_dive_batch; depth > 1: mipx_lp_plunge_batch): arrays
        of (depth + 1) * batch rows (nodes, then dive children level by level, status -1 where none)
        plus dive_var / dive_dir / dive_val with depth * batch entries (the decision after level p at
        p * batch + node)."""
        n, m = self.n, self.m
        l = np.ascontiguousarray(l, dtype=np.float64).reshape(-1, n)
        B = l.shape[0]
        D = int(depth)
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(B, n)
        vstat = _arr(vstat, np.int8, (B, n + m))
        ii = np.ascontiguousarray(integer_indices, dtype=np.int32)
        cl, cr, he = _arr(cost_l, np.float64), _arr(cost_r, np.float64), _arr(has_entry, np.uint8)
        R = (D + 1) * B
        status = np.zeros(R, np.int32); obj = np.zeros(R); x = np.zeros((R, n))
        vout = np.zeros((R, n + m), np.int8); iters = np.zeros(R, np.int32)
        npiv = np.zeros(R, np.int32)
        dvar = np.zeros(D * B, np.int32); ddir = np.zeros(D * B, np.int32); dval = np.zeros(D * B)
        rc = lib().mipx_lp_plunge_batch(self._h, B, D, _ptr(l), _ptr(u), _ptr(vstat), int(max_iter), int(rule),
                                        _ptr(ii), len(ii), _ptr(cl), _ptr(cr), _ptr(he), float(cutoff),
                                        _ptr(status), _ptr(obj), _ptr(x), _ptr(vout), _ptr(iters), _ptr(npiv),
                                        _ptr(dvar), _ptr(ddir), _ptr(dval))
        self.ctx.check(rc, 'mipx_lp_plunge_batch')
        return dict(status=status, obj=obj, x=x, vstat=vout, iters=iters, npivots=npiv, dive_var=dvar,
                    dive_dir=ddir, dive_val=dval)

    def gomory_batch(self, l, u, vstat, x, integer_indices, max_term=1e3):
        """GMI cuts + safe rounding for solved nodes; list (one per node) of dicts with
        row_idx, pi, pi0, safe_pi, safe_pi0 (one row per cut)."""
        n, m = self.n, self.m
        l = np.ascontiguousarray(l, dtype=np.float64).reshape(-1, n)
        B = l.shape[0]
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(B, n)
        vstat = np.ascontiguousarray(vstat, dtype=np.int8).reshape(B, n + m)
        x = np.ascontiguousarray(np.maximum(np.asarray(x, dtype=np.float64), 0)).reshape(B, n)
        is_int = np.zeros(n, np.uint8)
        is_int[np.asarray(integer_indices, dtype=int)] = 1
        ncuts = np.zeros(B, np.int32); row_idx = np.zeros((B, max(m, 1)), np.int32)
        pi = np.zeros((B, max(m, 1), n)); pi0 = np.zeros((B, max(m, 1)))
        spi = np.zeros((B, max(m, 1), n)); spi0 = np.zeros((B, max(m, 1)))
        rc = lib().mipx_gomory_batch(self._h, B, _ptr(l), _ptr(u), _ptr(vstat), _ptr(x),
                                     _ptr(is_int), float(max_term), _ptr(ncuts), _ptr(row_idx),
                                     _ptr(pi), _ptr(pi0), _ptr(spi), _ptr(spi0))
        self.ctx.check(rc, 'mipx_gomory_batch')
        return [dict(row_idx=row_idx[k, :ncuts[k]], pi=pi[k, :ncuts[k]], pi0=pi0[k, :ncuts[k]],
                     safe_pi=spi[k, :ncuts[k]], safe_pi0=spi0[k, :ncuts[k]]) for k in range(B)]

    def round_repair_batch(self, x, l, u, integer_indices, tol=1e-9, max_moves=None, skip=None):
        """The primal heuristic on host buffers (mipx_round_repair_batch, include/mipx_heur.h): x (batch, n) points,
        l, u the bounds (n each), skip an optional (batch,) mask.  Returns dict of x (batch, n), obj, status
        (HEUR_STATUS codes) and moves (batch, 2: repair, lift); max_moves None: m + n."""
        n = self.n
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, n)
        B = x.shape[0]
        l, u = _arr(l, np.float64, n), _arr(u, np.float64, n)
        ii = np.ascontiguousarray(integer_indices, dtype=np.int32).reshape(-1)
        sk = None if skip is None else np.ascontiguousarray(np.asarray(skip) != 0, dtype=np.uint8).reshape(B)
        max_moves = self.m + n if max_moves is None else int(max_moves)
        xo = np.zeros((B, n)); obj = np.zeros(B); status = np.zeros(B, np.int32); moves = np.zeros((B, 2), np.int32)
        rc = lib().mipx_round_repair_batch(self._h, B, _ptr(x), _ptr(l), _ptr(u), _ptr(ii), len(ii), float(tol), max_moves,
                                           _ptr(sk), _ptr(xo), _ptr(obj), _ptr(status), _ptr(moves))
        self.ctx.check(rc, 'mipx_round_repair_batch')
        return dict(x=xo, obj=obj, status=status, moves=moves)

    def pair_search_batch(self, x, l, u, integer_indices, tol=1e-9, max_moves=DEFAULT_LOCAL_SEARCH_MOVES, skip=None,
                          in_place=False):
        """The pair-move local search on host buffers (mipx_pair_search_batch, include/mipx_lsearch.h): x (batch, n)
        feasible integral points, l, u the bounds (n each), skip an optional (batch,) mask.  in_place: the output is
        the (converted) input itself.  Returns dict of x (batch, n), obj, status (LSEARCH_STATUS codes) and moves
        (batch, 2: singles, pairs)."""
        n = self.n
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, n)
        B = x.shape[0]
        l, u = _arr(l, np.float64, n), _arr(u, np.float64, n)
        ii = np.ascontiguousarray(integer_indices, dtype=np.int32).reshape(-1)
        sk = None if skip is None else np.ascontiguousarray(np.asarray(skip) != 0, dtype=np.uint8).reshape(B)
        if in_place:
            xo = x = x.copy()
        else:
            xo = np.zeros((B, n))
        obj = np.zeros(B); status = np.zeros(B, np.int32); moves = np.zeros((B, 2), np.int32)
        rc = lib().mipx_pair_search_batch(self._h, B, _ptr(x), _ptr(l), _ptr(u), _ptr(ii), len(ii), float(tol), int(max_moves),
                                          _ptr(sk), _ptr(xo), _ptr(obj), _ptr(status), _ptr(moves))
        self.ctx.check(rc, 'mipx_pair_search_batch')
        return dict(x=xo, obj=obj, status=status, moves=moves)

    def fix_propagate_batch(self, x, l, u, integer_indices, cutoff=None, tol=1e-9, max_rounds=DEFAULT_FIX_PROPAGATE_ROUNDS,
                            max_tries=DEFAULT_FIX_PROPAGATE_TRIES, skip=None):
        """The fix-and-propagate dive on host buffers (mipx_fix_propagate_batch, include/mipx_fixprop.h): x (batch, n)
        points, l, u the bounds (n each), cutoff None or an objective value no point above which is of interest, skip an
        optional (batch,) mask.  Returns dict of x (batch, n), obj, status (FIXPROP_STATUS codes) and counts (batch, 2:
        fixings, tries)."""
        n = self.n
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, n)
        B = x.shape[0]
        l, u = _arr(l, np.float64, n), _arr(u, np.float64, n)
        ii = np.ascontiguousarray(integer_indices, dtype=np.int32).reshape(-1)
        sk = None if skip is None else np.ascontiguousarray(np.asarray(skip) != 0, dtype=np.uint8).reshape(B)
        cutoff = np.inf if cutoff is None else float(cutoff)
        xo = np.zeros((B, n)); obj = np.zeros(B); status = np.zeros(B, np.int32); counts = np.zeros((B, 2), np.int32)
        rc = lib().mipx_fix_propagate_batch(self._h, B, _ptr(x), _ptr(l), _ptr(u), _ptr(ii), len(ii), cutoff, float(tol),
                                            int(max_rounds), int(max_tries), _ptr(sk), _ptr(xo), _ptr(obj), _ptr(status),
                                            _ptr(counts))
        self.ctx.check(rc, 'mipx_fix_propagate_batch')
        return dict(x=xo, obj=obj, status=status, counts=counts)

    def weighted_repair_batch(self, x, l, u, integer_indices, tol=1e-9, max_steps=DEFAULT_WEIGHTED_REPAIR_STEPS, skip=None,
                              gate=None):
        """The weighted row repair on host buffers (mipx_weighted_repair_batch, include/mipx_wrepair.h): x (batch, n)
        points, l, u the bounds (n each), skip an optional (batch,) mask, gate optional (batch,) statuses of the rounding
        heuristic (only its stuck and capped points are run).  Returns dict of x (batch, n), obj, status (WREPAIR_STATUS
        codes) and counts (batch, 2: moves, bumps)."""
        n = self.n
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, n)
        B = x.shape[0]
        l, u = _arr(l, np.float64, n), _arr(u, np.float64, n)
        ii = np.ascontiguousarray(integer_indices, dtype=np.int32).reshape(-1)
        sk = None if skip is None else np.ascontiguousarray(np.asarray(skip) != 0, dtype=np.uint8).reshape(B)
        gt = None if gate is None else np.ascontiguousarray(gate, dtype=np.int32).reshape(B)
        xo = np.zeros((B, n)); obj = np.zeros(B); status = np.zeros(B, np.int32); counts = np.zeros((B, 2), np.int32)
        rc = lib().mipx_weighted_repair_batch(self._h, B, _ptr(x), _ptr(l), _ptr(u), _ptr(ii), len(ii), float(tol), int(max_steps),
                                              _ptr(sk), _ptr(gt), _ptr(xo), _ptr(obj), _ptr(status), _ptr(counts))
        self.ctx.check(rc, 'mipx_weighted_repair_batch')
        return dict(x=xo, obj=obj, status=status, counts=counts)

    def support_screen_batch(self, pi, pi0, screen_tol, l, u, y, has_y):
        """The dual screen and the pack of a support evaluation on host buffers (mipx_support_screen_batch,
        include/mipx_cglp_screen.h; test scaffolding): pi (n), l, u (T, n) the leaves' boxes, y (T, m) their duals,
        has_y (T,) which of them count.  Returns dict of bound (T,), screened (T,), packed (T,: positions of the
        unscreened leaves in ascending order, then -1) and count."""
        n, m = self.n, self.m
        pi = np.ascontiguousarray(pi, np.float64).reshape(n)
        l = np.ascontiguousarray(l, np.float64).reshape(-1, n)
        T = l.shape[0]
        u = np.ascontiguousarray(u, np.float64).reshape(T, n)
        y = np.ascontiguousarray(y, np.float64).reshape(T, m)
        has_y = np.ascontiguousarray(np.asarray(has_y) != 0, dtype=np.uint8).reshape(T)
        bound = np.zeros(T); screened = np.zeros(T, np.uint8); packed = np.zeros(T, np.int32); count = np.zeros(1, np.int32)
        rc = lib().mipx_support_screen_batch(self._h, T, _ptr(pi), float(pi0), float(screen_tol), _ptr(l), _ptr(u), _ptr(y),
                                             _ptr(has_y), _ptr(bound), _ptr(screened), _ptr(packed), _ptr(count))
        self.ctx.check(rc, 'mipx_support_screen_batch')
        return dict(bound=bound, screened=screened, packed=packed, count=int(count[0]))

    def cube_search_batch(self, x, l, u, integer_indices, cutoff=np.inf, tol=1e-9, ftol=1e-4,
                          max_columns=DEFAULT_CUBE_SEARCH_COLUMNS, skip=None):
        """The cube search on host buffers (mipx_cube_search_batch, include/mipx_cube.h): x (batch, n) points, l, u the
        bounds (n each), cutoff an objective value only points below which are of interest, ftol the distance from an
        integer above which a column counts as fractional, skip an optional (batch,) mask.  Returns dict of x
        (batch, n), obj, status (CUBE_STATUS codes) and counts (batch, 2: k, code)."""
        n = self.n
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, n)
        B = x.shape[0]
        l, u = _arr(l, np.float64, n), _arr(u, np.float64, n)
        ii = np.ascontiguousarray(integer_indices, dtype=np.int32).reshape(-1)
        sk = None if skip is None else np.ascontiguousarray(np.asarray(skip) != 0, dtype=np.uint8).reshape(B)
        xo = np.zeros((B, n)); obj = np.zeros(B); status = np.zeros(B, np.int32); counts = np.zeros((B, 2), np.int32)
        rc = lib().mipx_cube_search_batch(self._h, B, _ptr(x), _ptr(l), _ptr(u), _ptr(ii), len(ii), float(cutoff), float(tol),
                                          float(ftol), int(max_columns), _ptr(sk), _ptr(xo), _ptr(obj), _ptr(status), _ptr(counts))
        self.ctx.check(rc, 'mipx_cube_search_batch')
        return dict(x=xo, obj=obj, status=status, counts=counts)

    def complete_batch(self, x, l, u, integer_indices, vstat=None, ctol=DEFAULT_COMPLETION_TOL, skip=None):
        """Completion over the continuous columns on host buffers (mipx_complete_batch, include/mipx_complete.h): x
        (batch, n) points whose integer columns are held while one batched LP is solved over the others, l, u the
        bounds (n each), vstat None (cold) or (batch, n + m) basis codes to start from, skip an optional (batch,)
        mask.  Returns dict of x (batch, n), obj, status (COMPLETE_STATUS codes) and pivots."""
        n = self.n
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, n)
        B = x.shape[0]
        l, u = _arr(l, np.float64, n), _arr(u, np.float64, n)
        ii = np.ascontiguousarray(integer_indices, dtype=np.int32).reshape(-1)
        vs = None if vstat is None else np.ascontiguousarray(vstat, dtype=np.int8).reshape(B, n + self.m)
        sk = None if skip is None else np.ascontiguousarray(np.asarray(skip) != 0, dtype=np.uint8).reshape(B)
        xo = np.zeros((B, n)); obj = np.zeros(B); status = np.zeros(B, np.int32); pivots = np.zeros(B, np.int32)
        rc = lib().mipx_complete_batch(self._h, B, _ptr(x), _ptr(l), _ptr(u), _ptr(ii), len(ii), _ptr(vs), float(ctol), _ptr(sk),
                                       _ptr(xo), _ptr(obj), _ptr(status), _ptr(pivots))
        self.ctx.check(rc, 'mipx_complete_batch')
        return dict(x=xo, obj=obj, status=status, pivots=pivots)

    def lpdive_batch(self, x, l, u, integer_indices, vstat=None, skip=None, cutoff=np.inf, max_rounds=DEFAULT_LP_DIVE_ROUNDS,
                     rule=0):
        """LP dives on host buffers (mipx_lpdive_batch, include/mipx_lpdive.h): x (batch, n) LP points, l, u (batch, n)
        the boxes they are optimal over, vstat None or (batch, n + m) basis codes of those LPs, skip an optional
        (batch,) mask, rule 0 (fractional) or 1 (coefficient).  Returns dict of x (batch, n), obj, status (LPDIVE_STATUS
        codes), rounds, fixings, flips and pivots."""
        n = self.n
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, n)
        B = x.shape[0]
        l = np.ascontiguousarray(l, dtype=np.float64).reshape(B, n)
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(B, n)
        ii = np.ascontiguousarray(integer_indices, dtype=np.int32).reshape(-1)
        vs = None if vstat is None else np.ascontiguousarray(vstat, dtype=np.int8).reshape(B, n + self.m)
        sk = None if skip is None else np.ascontiguousarray(np.asarray(skip) != 0, dtype=np.uint8).reshape(B)
        xo = np.zeros((B, n)); obj = np.zeros(B)
        status, rounds, fixings, flips, pivots = (np.zeros(B, np.int32) for _ in range(5))
        rc = lib().mipx_lpdive_batch(self._h, B, _ptr(x), _ptr(l), _ptr(u), _ptr(ii), len(ii), _ptr(vs), _ptr(sk), float(cutoff),
                                     int(max_rounds), int(rule), _ptr(xo), _ptr(obj), _ptr(status), _ptr(rounds), _ptr(fixings),
                                     _ptr(flips), _ptr(pivots))
        self.ctx.check(rc, 'mipx_lpdive_batch')
        return dict(x=xo, obj=obj, status=status, rounds=rounds, fixings=fixings, flips=flips, pivots=pivots)

    def propagate_batch(self, l, u, integer_indices, cutoff=None, tol=PROPAGATION_TOL, max_rounds=DEFAULT_PROPAGATION_ROUNDS):
        """Bound propagation on host buffers (mipx_propagate_batch, include/mipx_prop.h): l, u (batch, n) boxes,
        cutoff None or an objective value no point above which is of interest.  Returns dict of l, u (batch, n),
        status (PROP_STATUS codes), changed and rounds (batch each)."""
        n = self.n
        l = np.ascontiguousarray(l, dtype=np.float64).reshape(-1, n)
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(-1, n)
        B = l.shape[0]
        assert u.shape[0] == B, 'l and u hold the same number of boxes'
        ii = np.ascontiguousarray(integer_indices, dtype=np.int32).reshape(-1)
        cutoff = np.inf if cutoff is None else float(cutoff)
        lo = np.zeros((B, n)); uo = np.zeros((B, n))
        status = np.zeros(B, np.int32); changed = np.zeros(B, np.int32); rounds = np.zeros(B, np.int32)
        rc = lib().mipx_propagate_batch(self._h, B, _ptr(l), _ptr(u), _ptr(ii), len(ii), cutoff, float(tol), int(max_rounds),
                                        _ptr(lo), _ptr(uo), _ptr(status), _ptr(changed), _ptr(rounds))
        self.ctx.check(rc, 'mipx_propagate_batch')
        return dict(l=lo, u=uo, status=status, changed=changed, rounds=rounds)

    def mir_separate_batch(self, x, l, u, integer_indices, row_integral=None, multipliers=None,
                           max_divisors=DEFAULT_MIR_DIVISORS, f0_min=DEFAULT_MIR_F0_MIN, min_efficacy=1e-8,
                           max_dynamism=DEFAULT_MIR_DYNAMISM):
        """MIR separation on host buffers (mipx_mir_separate_batch, include/mipx_mir.h): x, l, u (batch, n) points and
        boxes, row_integral m flags or None, multipliers None (the m unit rows) or an (R, m) matrix shared by the
        points.  Returns dict of pi (batch, R, n), pi0, efficacy, delta, sign, status (MIR_STATUS codes; batch, R each)
        and kernel_us, the device time of the kernel."""
        n, m = self.n, self.m
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, n)
        B = x.shape[0]
        l = np.ascontiguousarray(l, dtype=np.float64).reshape(-1, n)
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(-1, n)
        assert l.shape[0] == B and u.shape[0] == B, 'x, l and u hold the same number of rows'
        ii = np.ascontiguousarray(integer_indices, dtype=np.int32).reshape(-1)
        ri = _arr(row_integral, np.uint8, m)
        mult = _arr(multipliers, np.float64, (-1, m))
        R = m if mult is None else mult.shape[0]
        pi = np.zeros((B, R, n)); pi0 = np.zeros((B, R)); eff = np.zeros((B, R)); delta = np.zeros((B, R))
        sign = np.zeros((B, R), np.int32); status = np.zeros((B, R), np.int32)
        rc = lib().mipx_mir_separate_batch(self._h, B, _ptr(x), _ptr(l), _ptr(u), _ptr(ii), len(ii), _ptr(ri),
                                           0 if mult is None else R, _ptr(mult), int(max_divisors), float(f0_min),
                                           float(min_efficacy), float(max_dynamism), _ptr(pi), _ptr(pi0), _ptr(eff),
                                           _ptr(delta), _ptr(sign), _ptr(status))
        self.ctx.check(rc, 'mipx_mir_separate_batch')
        ms = self.ctx.last_kernel_ms() if B else 0.0
        return dict(pi=pi, pi0=pi0, efficacy=eff, delta=delta, sign=sign, status=status,
                    kernel_us=max(ms, 0.0) * 1e3)

    def cover_separate_batch(self, x, l, u, integer_indices, rows=None, min_efficacy=1e-6):
        """Lifted cover separation on host buffers (mipx_cover_separate_batch, include/mipx_cover.h): x, l, u
        (batch, n) points and boxes, rows None (the m rows) or R distinct row indices shared by the points.  Returns
        dict of pi (batch, R, n), pi0, efficacy, cover_size, status (COVER_STATUS codes; batch, R each) and kernel_us,
        the device time of the kernel."""
        n, m = self.n, self.m
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, n)
        B = x.shape[0]
        l = np.ascontiguousarray(l, dtype=np.float64).reshape(-1, n)
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(-1, n)
        assert l.shape[0] == B and u.shape[0] == B, 'x, l and u hold the same number of rows'
        ii = np.ascontiguousarray(integer_indices, dtype=np.int32).reshape(-1)
        ro = _arr(rows, np.int32)
        R = m if ro is None else len(ro)
        pi = np.zeros((B, R, n)); pi0 = np.zeros((B, R)); eff = np.zeros((B, R))
        size = np.zeros((B, R), np.int32); status = np.zeros((B, R), np.int32)
        rc = lib().mipx_cover_separate_batch(self._h, B, _ptr(x), _ptr(l), _ptr(u), _ptr(ii), len(ii), _ptr(ro),
                                             0 if ro is None else R, float(min_efficacy), _ptr(pi), _ptr(pi0), _ptr(eff),
                                             _ptr(size), _ptr(status))
        self.ctx.check(rc, 'mipx_cover_separate_batch')
        ms = self.ctx.last_kernel_ms() if B else 0.0
        return dict(pi=pi, pi0=pi0, efficacy=eff, cover_size=size, status=status, kernel_us=max(ms, 0.0) * 1e3)

    def conflict_graph(self, l, u, integer_indices):
        """The conflict graph of the problem's rows in the box l, u (mipx_clique_graph, include/mipx_clique.h): literal
        2j is x_j - l_j, literal 2j + 1 its complement.  Returns dict of adj ((2n, Wd) uint32 words, bit k mod 32 of
        word k div 32 is literal k), row_status (0 used, 4 skipped; m) and kernel_us, the device time of the kernel."""
        n, m = self.n, self.m
        l = np.ascontiguousarray(l, dtype=np.float64).reshape(-1)
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(-1)
        assert len(l) == n and len(u) == n, 'l and u hold one box of n columns'
        ii = np.ascontiguousarray(integer_indices, dtype=np.int32).reshape(-1)
        adj = np.zeros((2 * n, (2 * n + 31) // 32), np.uint32)
        row_status = np.zeros(m, np.int32)
        rc = lib().mipx_clique_graph(self._h, _ptr(l), _ptr(u), _ptr(ii), len(ii), _ptr(adj), _ptr(row_status))
        self.ctx.check(rc, 'mipx_clique_graph')
        return dict(adj=adj, row_status=row_status, kernel_us=max(self.ctx.last_kernel_ms(), 0.0) * 1e3)

    def clique_separate_batch(self, X, l, u, integer_indices, adj, seeds=None, min_efficacy=1e-6):
        """Clique separation on host buffers (mipx_clique_separate_batch, include/mipx_clique.h): X (batch, n) points,
        l, u one box, adj the (2n, Wd) words of a conflict graph, seeds None (the 2n literals) or R distinct literals
        shared by the points.  Returns dict of pi (batch, R, n), pi0, efficacy, size, status (CLIQUE_STATUS codes;
        batch, R each) and kernel_us, the device time of the kernel."""
        n = self.n
        X = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, n)
        B = X.shape[0]
        l = np.ascontiguousarray(l, dtype=np.float64).reshape(-1)
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(-1)
        assert len(l) == n and len(u) == n, 'l and u hold one box of n columns'
        ii = np.ascontiguousarray(integer_indices, dtype=np.int32).reshape(-1)
        adj = np.ascontiguousarray(adj, dtype=np.uint32)
        assert adj.shape == (2 * n, (2 * n + 31) // 32), 'adj holds 2n rows of ceil(2n / 32) words'
        sd = _arr(seeds, np.int32)
        R = 2 * n if sd is None else len(sd)
        pi = np.zeros((B, R, n)); pi0 = np.zeros((B, R)); eff = np.zeros((B, R))
        size = np.zeros((B, R), np.int32); status = np.zeros((B, R), np.int32)
        rc = lib().mipx_clique_separate_batch(self._h, B, _ptr(X), _ptr(l), _ptr(u), _ptr(ii), len(ii), _ptr(adj), _ptr(sd),
                                              0 if sd is None else R, float(min_efficacy), _ptr(pi), _ptr(pi0), _ptr(eff),
                                              _ptr(size), _ptr(status))
        self.ctx.check(rc, 'mipx_clique_separate_batch')
        ms = self.ctx.last_kernel_ms() if B else 0.0
        return dict(pi=pi, pi0=pi0, efficacy=eff, size=size, status=status, kernel_us=max(ms, 0.0) * 1e3)

    def reduced_cost_tighten_batch(self, l, u, y, integer_indices, cutoff, tol=RCFIX_TOL, dtol=RCFIX_DTOL, in_place=False):
        """Reduced-cost bound tightening on host buffers (mipx_reduced_cost_tighten_batch, include/mipx_rcfix.h):
        l, u (batch, n) boxes, y (batch, m) row duals (any vectors), cutoff an objective value no point above which
        is of interest (None or infinite: every box ends with status no_bound).  in_place: the outputs are the
        (converted) inputs themselves.  Returns dict of l, u (batch, n), z (batch), status (RCFIX_STATUS codes) and
        changed (batch each)."""
        n, m = self.n, self.m
        l = np.ascontiguousarray(l, dtype=np.float64).reshape(-1, n)
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(-1, n)
        B = l.shape[0]
        y = np.ascontiguousarray(y, dtype=np.float64).reshape(B, m)
        assert u.shape[0] == B, 'l and u hold the same number of boxes'
        ii = np.ascontiguousarray(integer_indices, dtype=np.int32).reshape(-1)
        cutoff = np.inf if cutoff is None else float(cutoff)
        if in_place:
            lo, uo = l, u = l.copy(), u.copy()
        else:
            lo = np.zeros((B, n)); uo = np.zeros((B, n))
        z = np.zeros(B); status = np.zeros(B, np.int32); changed = np.zeros(B, np.int32)
        rc = lib().mipx_reduced_cost_tighten_batch(self._h, B, _ptr(l), _ptr(u), _ptr(y), _ptr(ii), len(ii), cutoff, float(tol),
                                                   float(dtol), _ptr(lo), _ptr(uo), _ptr(z), _ptr(status), _ptr(changed))
        self.ctx.check(rc, 'mipx_reduced_cost_tighten_batch')
        return dict(l=lo, u=uo, z=z, status=status, changed=changed)

    def solve_batch_dev(self, B, d_l, d_u, d_vstat, max_iter, d_status, d_obj, d_x, d_y, d_vout,
                        d_iters, d_npiv):
        rc = lib().mipx_lp_solve_batch_dev(self._h, int(B), d_l, d_u, d_vstat, int(max_iter),
                                           d_status, d_obj, d_x, d_y, d_vout, d_iters, d_npiv)
        self.ctx.check(rc, 'mipx_lp_solve_batch_dev')

    def close(self):
        if getattr(self, '_h', None) and getattr(self.ctx, '_h', None):
            lib().mipx_problem_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Tree:
    """Native frontier engine on one problem (mipx_tree)."""

    def __init__(self, problem, integer_indices, l, u, branch_rule='most fractional',
                 search_rule='best first', strong_branch_iters=5, max_batch=1,
                 pool_capacity=1 << 16, cut_params=None):
        """cut_params: None (no cut rounds) or a dict of mipx_cut_params fields -- Gomory cut rounds
        run inside the engine (mipx_tree_create_ex)."""
        self.problem = problem
        ints = np.ascontiguousarray(integer_indices, dtype=np.int32)
        l = np.ascontiguousarray(l, dtype=np.float64).reshape(problem.n)
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(problem.n)
        rule = {'most fractional': 0, 'pseudo cost': 1}[branch_rule]
        search = {'best first': 0, 'depth first': 1}[search_rule]
        h = _vp()
        cp = None
        if cut_params is not None:
            cp = CutParams(max_cut_generation_iterations=10, max_nonzero_coefs=1000000, max_cuts_per_node=0,
                           exact_tableau=1, cutting_plane_progress_tolerance=1e-4, min_cut_depth=1e-8,
                           cos_parallel=0.984807753012208, max_abs_coef=1e6, max_term=1e3,
                           max_dual_bound=float('inf'), store_capacity=0)
            for key, value in cut_params.items():
                assert hasattr(cp, key), f'unknown cut parameter {key}'
                setattr(cp, key, value)
        rc = lib().mipx_tree_create_ex(problem._h, _ptr(ints), len(ints), _ptr(l), _ptr(u), rule,
                                       search, int(strong_branch_iters), int(max_batch),
                                       int(pool_capacity), None if cp is None else C.byref(cp), C.byref(h))
        problem.ctx.check(rc, 'mipx_tree_create_ex')
        self.cuts = cp is not None
        self._h = h
        self.max_batch = int(max_batch)

    @classmethod
    def restart(cls, src, problem):
        """A tree on `problem` (same A, c and shape as src's, another b) that starts from src's recorded leaves
        (mipx_tree_create_restart, include/mipx_restart.h): src's creation parameters, pseudo-cost table and
        root basis, its records as the skeleton, its childless records as the open nodes."""
        h = _vp()
        rc = lib().mipx_tree_create_restart(src._h, problem._h, C.byref(h))
        problem.ctx.check(rc, 'mipx_tree_create_restart')
        self = cls.__new__(cls)
        self.problem, self.cuts, self._h, self.max_batch = problem, False, h, src.max_batch
        return self

    def restart_stats(self):
        """dict(skeleton, seeds, device_bytes, seed_ms, seeds_evaluated, seeds_infeasible, seeds_integral)
        (mipx_tree_restart_stats)."""
        out = np.zeros(8, np.int64)
        self.problem.ctx.check(lib().mipx_tree_restart_stats(self._h, _ptr(out)), 'mipx_tree_restart_stats')
        d = dict(zip(RESTART_STATS_KEYS, (int(v) for v in out)))
        d['seed_ms'] /= 1000.0
        return d

    def restart_seeds(self):
        """The ids of the seeds, ascending (mipx_tree_restart_seeds)."""
        S = lib().mipx_tree_restart_seeds(self._h, 0, None)
        if S < 0:
            self.problem.ctx.check(int(S), 'mipx_tree_restart_seeds')
        ids = np.zeros(S, np.int64)
        lib().mipx_tree_restart_seeds(self._h, S, _ptr(ids))
        return ids

    def solve(self, node_limit=0, mip_gap=1e-4, max_seconds=0.0, frontier_batch=None, max_steps=0):
        st = TreeStats()
        rc = lib().mipx_tree_solve(self._h, int(node_limit), float(mip_gap), float(max_seconds),
                                   int(frontier_batch or self.max_batch), int(max_steps),
                                   C.byref(st))
        err, self._hook_error = getattr(self, '_hook_error', None), None
        if err is not None:  # raised inside the step hook: the engine stopped, re-raise it here
            raise err
        comm = getattr(self, '_comm', None)
        if comm is not None and getattr(comm, '_err', None) is not None:   # raised inside a transport callback
            cerr, comm._err = comm._err, None
            raise cerr
        self.problem.ctx.check(rc, 'mipx_tree_solve')
        return st.as_dict()

    def reanchor(self, max_nodes):
        """Give the first max_nodes open nodes an anchor of their own (mipx_tree_reanchor)."""
        self.problem.ctx.check(lib().mipx_tree_reanchor(self._h, int(max_nodes)), 'mipx_tree_reanchor')

    def peek_anchors(self, max_nodes):
        """Anchor-table entry of each open node, in the order of peek_open (-1: the root's anchor)."""
        a = np.full(int(max_nodes), -1, np.int32)
        k = lib().mipx_tree_peek_anchors(self._h, int(max_nodes), _ptr(a))
        if k < 0:
            self.problem.ctx.check(int(k), 'mipx_tree_peek_anchors')
        return a[:k]

    def anchor_table(self):
        """(T, vec, idx) of the re-anchoring table as host arrays, or None."""
        L = lib()
        K = L.mipx_tree_anchor_table(self._h, None, None, None)
        if K <= 0:
            return None
        n, m = self.problem.n, self.problem.m
        T = np.zeros((K, m, n)); vec = np.zeros((K, n + 3 * m)); idx = np.zeros((K, 2 * n + m), np.int32)
        k = L.mipx_tree_anchor_table(self._h, _ptr(T), _ptr(vec), _ptr(idx))
        if k < 0:
            self.problem.ctx.check(int(k), 'mipx_tree_anchor_table')
        return T, vec, idx

    def set_dive(self, on=True):
        """In-place plunge on the tableau a node's workgroup holds (mipx_tree_set_dive): True / 1 one
        dive child per node, an int up to 8 that many in a row, False / 0 off."""
        self.problem.ctx.check(lib().mipx_tree_set_dive(self._h, int(on)), 'mipx_tree_set_dive')

    def set_step_hook(self, fn, every_steps=1):
        """Call fn() every `every_steps` frontier steps inside solve(), while the GPU works on the
        steps already queued (mipx_tree_set_step_hook): the place for a rank's all-reduce.  fn may
        use stats(), pseudo_cost_arrays(), set_primal_bound(), set_pseudo_cost_arrays(); a truthy
        return value or an exception stops the solve.  fn=None removes the hook."""
        if fn is None:
            self._hook = None
            rc = lib().mipx_tree_set_step_hook(self._h, TREE_HOOK(), None, 0)
        else:
            def trampoline(_user):
                try:
                    return 1 if fn() else 0
                except BaseException as e:  # never unwind through the C frames
                    self._hook_error = e
                    return 1
            self._hook = TREE_HOOK(trampoline)  # keep the thunk alive as long as it is installed
            rc = lib().mipx_tree_set_step_hook(self._h, self._hook, None, int(every_steps))
        self.problem.ctx.check(rc, 'mipx_tree_set_step_hook')

    def set_comm(self, comm, every_steps=5):
        """Attach the communicator: solve() becomes a collective call (mipx_tree_set_comm)."""
        self._comm = comm
        self.problem.ctx.check(lib().mipx_tree_set_comm(self._h, None if comm is None else comm._h, int(every_steps)),
                               'mipx_tree_set_comm')

    def migrate_self(self, amount):
        """Test hook (mipx_tree_migrate_self): up to `amount` open nodes leave and re-enter this rank through
        the communicator's point-to-point path; returns how many moved."""
        k = lib().mipx_tree_migrate_self(self._h, int(amount))
        if k < 0:
            self.problem.ctx.check(int(k), 'mipx_tree_migrate_self')
        return int(k)

    def exchange_record(self):
        """The record this rank would post right now (mipx_tree_exchange_record; needs set_comm)."""
        r = np.zeros(exchange_record_len(self.problem.n))
        self.problem.ctx.check(lib().mipx_tree_exchange_record(self._h, _ptr(r)), 'mipx_tree_exchange_record')
        return r

    def global_stats(self):
        st = GlobalStats()
        self.problem.ctx.check(lib().mipx_tree_global_stats(self._h, C.byref(st)), 'mipx_tree_global_stats')
        return {k: getattr(st, k) for k, _ in st._fields_}

    def kernel_ms(self):
        """Device time by kernel (ms): dict(node_lp, gomory, select) (mipx_tree_kernel_ms)."""
        out = (C.c_double * 4)()
        self.problem.ctx.check(lib().mipx_tree_kernel_ms(self._h, out), 'mipx_tree_kernel_ms')
        return dict(node_lp=out[0], gomory=out[1], select=out[2])

    def cut_stats(self):
        """The running GMIC totals of BaseNode._base_bound over every evaluated node (+ 'dropped')."""
        out = (C.c_int64 * 8)()
        self.problem.ctx.check(lib().mipx_tree_cut_stats(self._h, out), 'mipx_tree_cut_stats')
        d = {k: int(out[i]) for i, k in enumerate(CUT_TOTAL_KEYS)}
        d['dropped'] = int(out[7])
        return d

    def stats(self):
        st = TreeStats()
        self.problem.ctx.check(lib().mipx_tree_get_stats(self._h, C.byref(st)), 'mipx_tree_get_stats')
        return st.as_dict()

    def solution(self):
        x = np.zeros(self.problem.n)
        self.problem.ctx.check(lib().mipx_tree_solution(self._h, _ptr(x)), 'mipx_tree_solution')
        return x

    def set_primal_bound(self, bound):
        self.problem.ctx.check(lib().mipx_tree_set_primal_bound(self._h, float(bound)),
                               'mipx_tree_set_primal_bound')

    def pseudo_costs(self):
        """The table in the reference's layout {idx: {'left'|'right': {'cost', 'times'}}}."""
        n = self.problem.n
        cl, cr = np.zeros(n), np.zeros(n)
        tl, tr = np.zeros(n, np.int32), np.zeros(n, np.int32)
        self.problem.ctx.check(lib().mipx_tree_pseudo_costs(self._h, _ptr(cl), _ptr(cr), _ptr(tl),
                                                            _ptr(tr)), 'mipx_tree_pseudo_costs')
        out = {}
        for i in range(n):
            if tl[i] or tr[i]:
                out[i] = {'left': {'cost': float(cl[i]), 'times': int(tl[i])},
                          'right': {'cost': float(cr[i]), 'times': int(tr[i])}}
        return out

    def pseudo_cost_arrays(self):
        """(cost_l, cost_r, times_l, times_r) as arrays over all n variables."""
        n = self.problem.n
        cl, cr = np.zeros(n), np.zeros(n)
        tl, tr = np.zeros(n, np.int32), np.zeros(n, np.int32)
        self.problem.ctx.check(lib().mipx_tree_pseudo_costs(self._h, _ptr(cl), _ptr(cr), _ptr(tl),
                                                            _ptr(tr)), 'mipx_tree_pseudo_costs')
        return cl, cr, tl, tr

    def set_pseudo_cost_arrays(self, cl, cr, tl, tr):
        cl = np.ascontiguousarray(cl, np.float64); cr = np.ascontiguousarray(cr, np.float64)
        tl = np.ascontiguousarray(tl, np.int32); tr = np.ascontiguousarray(tr, np.int32)
        self.problem.ctx.check(lib().mipx_tree_set_pseudo_costs(self._h, _ptr(cl), _ptr(cr), _ptr(tl), _ptr(tr)),
                               'mipx_tree_set_pseudo_costs')

    def set_host_spill(self, max_bytes):
        """Spill open nodes to pinned host memory, up to max_bytes of compact records, when the pool runs
        low, instead of stopping the search (mipx_tree_set_host_spill; 0 turns it off)."""
        self.problem.ctx.check(lib().mipx_tree_set_host_spill(self._h, int(max_bytes)), 'mipx_tree_set_host_spill')

    def spill_stats(self):
        """dict(spilled, reloaded, on_host, host_bytes, peak_host_bytes, events, spill_ms, reload_ms)
        (mipx_tree_spill_stats)."""
        out = np.zeros(8, np.int64)
        self.problem.ctx.check(lib().mipx_tree_spill_stats(self._h, _ptr(out)), 'mipx_tree_spill_stats')
        d = dict(zip(SPILL_STATS_KEYS, (int(v) for v in out)))
        d['spill_ms'] /= 1000.0
        d['reload_ms'] /= 1000.0
        return d

    def set_dual_record(self, max_bytes, rows, pos, sign):
        """Record one dual term per solved node from the first step on, up to max_bytes of device memory
        (mipx_tree_set_dual_record, include/mipx_dualfn.h; -1: half of the device memory free now).  rows, pos,
        sign: the LP rows and, per engine row, its LP row and sign (the slack block of the penalised re-solve)."""
        pos = np.ascontiguousarray(pos, np.int32).reshape(-1)
        sign = np.ascontiguousarray(sign, np.float64).reshape(-1)
        assert len(pos) == len(sign) == self.problem.m, 'one (pos, sign) per engine row'
        self.problem.ctx.check(lib().mipx_tree_set_dual_record(self._h, int(max_bytes), int(rows), _ptr(pos), _ptr(sign)),
                               'mipx_tree_set_dual_record')

    def dual_function(self, W, M):
        """f(w) for every row w of W (K x m, engine rows): the dual function's lower bounds
        (mipx_tree_dual_function)."""
        W = np.ascontiguousarray(W, np.float64)
        if W.ndim == 1:
            W = W[None]
        assert W.shape[1] == self.problem.m, 'right-hand sides have one entry per engine row'
        out = np.zeros(W.shape[0])
        self.problem.ctx.check(lib().mipx_tree_dual_function(self._h, W.shape[0], _ptr(W), float(M), _ptr(out)),
                               'mipx_tree_dual_function')
        return out

    def dual_function_stats(self):
        """dict(records, bytes, dropped, infeasible_leaves, penalized_resolves, leaves_without_term, record_ms,
        eval_ms) (mipx_tree_dual_function_stats)."""
        out = np.zeros(8, np.int64)
        self.problem.ctx.check(lib().mipx_tree_dual_function_stats(self._h, _ptr(out)), 'mipx_tree_dual_function_stats')
        d = dict(zip(DUALFN_STATS_KEYS, (int(v) for v in out)))
        d['record_ms'] /= 1000.0
        d['eval_ms'] /= 1000.0
        return d

    def dual_records(self):
        """dict(node, parent, status, t, y) of every record in store order (mipx_tree_dual_records)."""
        R = self.dual_function_stats()['records']
        node, parent = np.zeros(R, np.int64), np.zeros(R, np.int64)
        status, tval = np.zeros(R, np.int32), np.zeros(R)
        y = np.zeros((R, self.problem.m))
        got = lib().mipx_tree_dual_records(self._h, R, _ptr(node), _ptr(parent), _ptr(status), _ptr(tval), _ptr(y))
        if got < 0:
            self.problem.ctx.check(int(got), 'mipx_tree_dual_records')
        return dict(node=node, parent=parent, status=status, t=tval, y=y)

    def set_tree_record(self, on=True):
        """Keep one record per node the search creates, from the first step on (mipx_tree_set_tree_record,
        include/mipx_treerec.h)."""
        self.problem.ctx.check(lib().mipx_tree_set_tree_record(self._h, int(bool(on))), 'mipx_tree_set_tree_record')

    def tree_records(self, first=0, count=None):
        """dict(parent, bvar, bdir, bval, depth, lp_status, flags, dual_bound, objective) of the records
        [first, first + count), by default all of them (mipx_tree_records)."""
        if count is None:
            count = max(self.tree_record_stats()['nodes'] - int(first), 0)
        count = int(count)
        out = dict(parent=np.zeros(count, np.int64), bvar=np.zeros(count, np.int32), bdir=np.zeros(count, np.int32),
                   bval=np.zeros(count), depth=np.zeros(count, np.int32), lp_status=np.zeros(count, np.int32),
                   flags=np.zeros(count, np.int32), dual_bound=np.zeros(count), objective=np.zeros(count))
        got = lib().mipx_tree_records(self._h, int(first), count, *(_ptr(a) for a in out.values()))
        if got < 0:
            self.problem.ctx.check(int(got), 'mipx_tree_records')
        return {k: a[:got] for k, a in out.items()}

    def node_bounds(self, ids):
        """(l, u), len(ids) x n: the bounds of the recorded nodes `ids`, rebuilt on the device from the root's
        bounds and the branchings of each node's lineage (mipx_tree_node_bounds)."""
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        l = np.zeros((len(ids), self.problem.n)); u = np.zeros((len(ids), self.problem.n))
        self.problem.ctx.check(lib().mipx_tree_node_bounds(self._h, len(ids), _ptr(ids), _ptr(l), _ptr(u)),
                               'mipx_tree_node_bounds')
        return l, u

    def node_solve(self, ids, want_x=True, want_vstat=True):
        """dict(status, obj, x, vstat) of the LPs of the recorded nodes `ids`, re-solved in one batched launch
        from the root's optimal basis (mipx_tree_node_solve)."""
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        K, n, nv = len(ids), self.problem.n, self.problem.n + self.problem.m
        status = np.zeros(K, np.int32); obj = np.zeros(K)
        x = np.zeros((K, n)) if want_x else None
        vstat = np.zeros((K, nv), np.int8) if want_vstat else None
        self.problem.ctx.check(lib().mipx_tree_node_solve(self._h, K, _ptr(ids), _ptr(status), _ptr(obj), _ptr(x), _ptr(vstat)),
                               'mipx_tree_node_solve')
        return dict(status=status, obj=obj, x=x, vstat=vstat)

    def tree_record_stats(self):
        """dict(nodes, host_bytes, device_bytes, materialised, resolved, query_ms) (mipx_tree_record_stats)."""
        out = np.zeros(6, np.int64)
        self.problem.ctx.check(lib().mipx_tree_record_stats(self._h, _ptr(out)), 'mipx_tree_record_stats')
        d = dict(zip(TREEREC_STATS_KEYS, (int(v) for v in out)))
        d['query_ms'] /= 1000.0
        return d

    def support_open(self, ids, duals=False):
        """A Support session on the recorded nodes `ids`, the terms of a disjunction (mipx_tree_support_open,
        include/mipx_cglp.h).  It is closed with the tree at the latest.  duals=True keeps the leaves' row duals and
        the buffers of a packed launch, which eval(screen_tol=..., retry_cold=...) needs (MIPX_SUPPORT_KEEP_DUALS of
        mipx_tree_support_open_ex, include/mipx_cglp_screen.h)."""
        s = Support(self, ids, duals=duals)
        self._sessions = [r for r in getattr(self, '_sessions', []) if r() is not None] + [weakref.ref(s)]
        return s

    def set_heuristic(self, points=True, every_steps=1, max_moves=None):
        """Round, repair and lift the node LP solutions of the first `points` nodes of every `every_steps`-th step on
        the GPU and take the best feasible point as the incumbent where it beats the one the tree holds
        (mipx_tree_set_heuristic, include/mipx_heur.h; True: DEFAULT_HEURISTIC_POINTS; max_moves None: m + n)."""
        points = DEFAULT_HEURISTIC_POINTS if points is True else int(points)
        max_moves = self.problem.m + self.problem.n if max_moves is None else int(max_moves)
        self.problem.ctx.check(lib().mipx_tree_set_heuristic(self._h, points, int(every_steps), max_moves),
                               'mipx_tree_set_heuristic')

    def heuristic_stats(self):
        """dict(points, feasible, stuck, capped, repair_moves, lift_moves, incumbents, kernel_us)
        (mipx_tree_heuristic_stats)."""
        out = np.zeros(8, np.int64)
        self.problem.ctx.check(lib().mipx_tree_heuristic_stats(self._h, _ptr(out)), 'mipx_tree_heuristic_stats')
        return dict(zip(HEUR_STATS_KEYS, (int(v) for v in out)))

    def set_propagation(self, max_rounds=True, use_cutoff=True):
        """Propagate the bounds of every step's nodes over the rows on the GPU before their node LPs, in place on
        their pool rows, the incumbent's objective as a cutoff row unless use_cutoff is False
        (mipx_tree_set_propagation, include/mipx_prop.h; True: DEFAULT_PROPAGATION_ROUNDS rounds)."""
        max_rounds = DEFAULT_PROPAGATION_ROUNDS if max_rounds is True else int(max_rounds)
        self.problem.ctx.check(lib().mipx_tree_set_propagation(self._h, max_rounds, 1 if use_cutoff else 0),
                               'mipx_tree_set_propagation')

    def propagation_stats(self):
        """dict(nodes, tightened, infeasible, bounds_changed, rounds, capped, reserved, kernel_us)
        (mipx_tree_propagation_stats)."""
        out = np.zeros(8, np.int64)
        self.problem.ctx.check(lib().mipx_tree_propagation_stats(self._h, _ptr(out)), 'mipx_tree_propagation_stats')
        return dict(zip(PROP_STATS_KEYS, (int(v) for v in out)))

    def set_reduced_cost(self, on=True):
        """Tighten the bounds of every step's branching parents from the row duals of their node LPs and the
        incumbent on the GPU, in place on their pool rows before their children are written
        (mipx_tree_set_reduced_cost, include/mipx_rcfix.h)."""
        self.problem.ctx.check(lib().mipx_tree_set_reduced_cost(self._h, 1 if on else 0), 'mipx_tree_set_reduced_cost')

    def reduced_cost_stats(self):
        """dict(nodes, tightened, cut_off, no_bound, bounds_changed, launches, reserved, kernel_us)
        (mipx_tree_reduced_cost_stats)."""
        out = np.zeros(8, np.int64)
        self.problem.ctx.check(lib().mipx_tree_reduced_cost_stats(self._h, _ptr(out)), 'mipx_tree_reduced_cost_stats')
        return dict(zip(RCFIX_STATS_KEYS, (int(v) for v in out)))

    def set_local_search(self, max_moves=True):
        """Run the pair-move local search behind the primal heuristic of every step, in place on its feasible points
        (mipx_tree_set_local_search, include/mipx_lsearch.h; True: DEFAULT_LOCAL_SEARCH_MOVES moves per point at
        most; 0 or False: off).  After set_heuristic."""
        max_moves = DEFAULT_LOCAL_SEARCH_MOVES if max_moves is True else int(max_moves)
        self.problem.ctx.check(lib().mipx_tree_set_local_search(self._h, max_moves), 'mipx_tree_set_local_search')

    def local_search_stats(self):
        """dict(points, improved, single_moves, pair_moves, capped, incumbents, reserved, kernel_us)
        (mipx_tree_local_search_stats)."""
        out = np.zeros(8, np.int64)
        self.problem.ctx.check(lib().mipx_tree_local_search_stats(self._h, _ptr(out)), 'mipx_tree_local_search_stats')
        return dict(zip(LSEARCH_STATS_KEYS, (int(v) for v in out)))

    def set_fix_propagate(self, max_tries=True, max_rounds=DEFAULT_FIX_PROPAGATE_ROUNDS):
        """Run the fix-and-propagate dive behind the primal heuristic of every step, on the points its rounding did not
        end feasible on (mipx_tree_set_fix_propagate, include/mipx_fixprop.h; True: DEFAULT_FIX_PROPAGATE_TRIES
        propagation calls per point at most; 0 or False: off).  After set_heuristic."""
        max_tries = DEFAULT_FIX_PROPAGATE_TRIES if max_tries is True else int(max_tries)
        self.problem.ctx.check(lib().mipx_tree_set_fix_propagate(self._h, int(max_rounds), max_tries), 'mipx_tree_set_fix_propagate')

    def fix_propagate_stats(self):
        """dict(points, feasible, stuck, capped, fixings, tries, incumbents, kernel_us) (mipx_tree_fix_propagate_stats)."""
        out = np.zeros(8, np.int64)
        self.problem.ctx.check(lib().mipx_tree_fix_propagate_stats(self._h, _ptr(out)), 'mipx_tree_fix_propagate_stats')
        return dict(zip(FIXPROP_STATS_KEYS, (int(v) for v in out)))

    def set_weighted_repair(self, max_steps=True):
        """Run the weighted row repair behind the primal heuristic of every step, on the points its rounding did not end
        feasible on (mipx_tree_set_weighted_repair, include/mipx_wrepair.h; True: DEFAULT_WEIGHTED_REPAIR_STEPS moves
        and bumps per point at most; 0 or False: off).  After set_heuristic; not together with set_fix_propagate."""
        max_steps = DEFAULT_WEIGHTED_REPAIR_STEPS if max_steps is True else int(max_steps)
        self.problem.ctx.check(lib().mipx_tree_set_weighted_repair(self._h, max_steps), 'mipx_tree_set_weighted_repair')

    def weighted_repair_stats(self):
        """dict(points, feasible, capped, moves, bumps, incumbents, reserved6, kernel_us) (mipx_tree_weighted_repair_stats)."""
        out = np.zeros(8, np.int64)
        self.problem.ctx.check(lib().mipx_tree_weighted_repair_stats(self._h, _ptr(out)), 'mipx_tree_weighted_repair_stats')
        return dict(zip(WREPAIR_STATS_KEYS, (int(v) for v in out)))

    def set_cube_search(self, max_columns=True):
        """Run the cube search beside the primal heuristic of every step, on the same LP points
        (mipx_tree_set_cube_search, include/mipx_cube.h; True: DEFAULT_CUBE_SEARCH_COLUMNS columns at most; 0 or False:
        off).  After set_heuristic."""
        max_columns = DEFAULT_CUBE_SEARCH_COLUMNS if max_columns is True else int(max_columns)
        self.problem.ctx.check(lib().mipx_tree_set_cube_search(self._h, max_columns), 'mipx_tree_set_cube_search')

    def cube_search_stats(self):
        """dict(points, found, none, columns, at_cap, incumbents, reserved6, kernel_us) (mipx_tree_cube_search_stats)."""
        out = np.zeros(8, np.int64)
        self.problem.ctx.check(lib().mipx_tree_cube_search_stats(self._h, _ptr(out)), 'mipx_tree_cube_search_stats')
        return dict(zip(CUBE_STATS_KEYS, (int(v) for v in out)))

    def set_completion(self, on=True):
        """Complete the points the heuristics of every step end on over the continuous columns, by one batched LP per
        step (mipx_tree_set_completion, include/mipx_complete.h; False: off).  After set_heuristic."""
        self.problem.ctx.check(lib().mipx_tree_set_completion(self._h, 1 if on else 0), 'mipx_tree_set_completion')

    def completion_stats(self):
        """dict(points, completed, infeasible, failed, rescued, incumbents, pivots, kernel_us) (mipx_tree_completion_stats)."""
        out = np.zeros(8, np.int64)
        self.problem.ctx.check(lib().mipx_tree_completion_stats(self._h, _ptr(out)), 'mipx_tree_completion_stats')
        return dict(zip(COMPLETE_STATS_KEYS, (int(v) for v in out)))

    def set_lpdive(self, max_rounds=DEFAULT_LP_DIVE_ROUNDS, every=0, rule=0):
        """LP dives on the LP points of a step's first nodes while the search holds no incumbent, or every `every` steps
        (mipx_tree_set_lpdive, include/mipx_lpdive.h; max_rounds 0: off).  After set_heuristic."""
        self.problem.ctx.check(lib().mipx_tree_set_lpdive(self._h, int(max_rounds), int(every), int(rule)), 'mipx_tree_set_lpdive')

    def lpdive_stats(self):
        """dict(points, feasible, infeasible, failed, moves, incumbents, pivots, kernel_us) (mipx_tree_lpdive_stats)."""
        out = np.zeros(8, np.int64)
        self.problem.ctx.check(lib().mipx_tree_lpdive_stats(self._h, _ptr(out)), 'mipx_tree_lpdive_stats')
        return dict(zip(LPDIVE_STATS_KEYS, (int(v) for v in out)))

    def set_objective_step(self, step):
        """Prune at one objective step below the incumbent (mipx_tree_set_objective_step, include/mipx_objstep.h):
        the caller guarantees that the objectives of any two integer-feasible points differ by a multiple of step."""
        self.problem.ctx.check(lib().mipx_tree_set_objective_step(self._h, float(step)), 'mipx_tree_set_objective_step')

    def objective_step_stats(self):
        """dict(closed_at_pop, left_unbranched, launches, reserved3 .. reserved7) (mipx_tree_objective_step_stats)."""
        out = np.zeros(8, np.int64)
        self.problem.ctx.check(lib().mipx_tree_objective_step_stats(self._h, _ptr(out)), 'mipx_tree_objective_step_stats')
        return dict(zip(OBJSTEP_STATS_KEYS, (int(v) for v in out)))

    def set_cut_migration(self, rows):
        """Reserve the top `rows` rows of the cut store for the cut rows of nodes received from other ranks, so
        that open nodes can migrate in cut-round mode (mipx_tree_set_cut_migration, include/mipx_cutmig.h;
        True: DEFAULT_CUT_MIGRATION_ROWS, 0 / False: off)."""
        rows = DEFAULT_CUT_MIGRATION_ROWS if rows is True else int(rows)
        self.problem.ctx.check(lib().mipx_tree_set_cut_migration(self._h, rows), 'mipx_tree_set_cut_migration')

    def cut_rows(self, ids):
        """(pi, pi0) of the cut store rows `ids`, own or migrated (mipx_tree_cut_rows)."""
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        pi = np.zeros((len(ids), self.problem.n)); pi0 = np.zeros(len(ids))
        self.problem.ctx.check(lib().mipx_tree_cut_rows(self._h, len(ids), _ptr(ids), _ptr(pi), _ptr(pi0)),
                               'mipx_tree_cut_rows')
        return pi, pi0

    def cut_migration_stats(self):
        """dict(nodes_sent_with_cuts, cut_rows_sent, cut_rows_received, region_rows_used)
        (mipx_tree_cut_migration_stats)."""
        out = np.zeros(4, np.int64)
        self.problem.ctx.check(lib().mipx_tree_cut_migration_stats(self._h, _ptr(out)), 'mipx_tree_cut_migration_stats')
        return dict(zip(CUTMIG_STATS_KEYS, (int(v) for v in out)))

    def peek_open(self, max_nodes):
        """(l, u, vstat, dual_bound) of up to max_nodes open nodes, without removing them."""
        n, nv = self.problem.n, self.problem.n + self.problem.m
        l = np.zeros((max_nodes, n)); u = np.zeros((max_nodes, n))
        v = np.zeros((max_nodes, nv), np.int8); db = np.zeros(max_nodes)
        k = lib().mipx_tree_peek_open(self._h, int(max_nodes), _ptr(l), _ptr(u), _ptr(v), _ptr(db))
        if k < 0:
            self.problem.ctx.check(int(k), 'mipx_tree_peek_open')
        return l[:k], u[:k], v[:k], db[:k]

    def keep_shard(self, rank, world):
        self.problem.ctx.check(lib().mipx_tree_keep_shard(self._h, int(rank), int(world)),
                               'mipx_tree_keep_shard')

    def set_anchor_mode(self, on=True):
        self.problem.ctx.check(lib().mipx_tree_set_anchor_mode(self._h, int(on)),
                               'mipx_tree_set_anchor_mode')

    def set_trace(self, on=True):
        self.problem.ctx.check(lib().mipx_tree_set_trace(self._h, int(on)), 'mipx_tree_set_trace')

    def trace(self):
        k = lib().mipx_tree_trace(self._h, 0, None, None, None, None)
        ids = np.zeros(k, np.int64); st = np.zeros(k, np.int32)
        bv = np.zeros(k, np.int32); obj = np.zeros(k)
        lib().mipx_tree_trace(self._h, k, _ptr(ids), _ptr(st), _ptr(bv), _ptr(obj))
        return dict(node_id=ids, status=st, branch_var=bv, objective=obj)

    def trace_cuts(self):
        """(nodes, 8) per evaluated node in trace order: cut rounds, iterations / number of GMICs created,
        added, removed, cut rows at the end (mipx_tree_trace_cuts)."""
        L = lib()
        k = L.mipx_tree_trace_cuts(self._h, 0, None)
        out = np.zeros((max(k, 0), 8), np.int32)
        L.mipx_tree_trace_cuts(self._h, k, _ptr(out))
        return out

    def peek_cuts(self, max_nodes):
        """(node ids, cut counts, cut lists, basis codes of the cut rows) of the open nodes, in the order
        of peek_open (mipx_tree_peek_cuts)."""
        L = lib()
        kc = max(0, L.mipx_tree_cut_rows_per_node(self._h))
        ids = np.zeros(max_nodes, np.int64); ncut = np.zeros(max_nodes, np.int32)
        lists = np.zeros((max_nodes, max(kc, 1)), np.int32); codes = np.zeros((max_nodes, max(kc, 1)), np.int8)
        k = L.mipx_tree_peek_cuts(self._h, int(max_nodes), _ptr(ids), _ptr(ncut), _ptr(lists), _ptr(codes))
        if k < 0:
            self.problem.ctx.check(int(k), 'mipx_tree_peek_cuts')
        return ids[:k], ncut[:k], lists[:k], codes[:k]

    def cut_store(self):
        """(pi, pi0) of every cut added so far (mipx_tree_cut_store)."""
        L = lib()
        k = L.mipx_tree_cut_store(self._h, 0, None, None)
        if k < 0:
            self.problem.ctx.check(int(k), 'mipx_tree_cut_store')
        pi = np.zeros((k, self.problem.n)); pi0 = np.zeros(k)
        if k:
            L.mipx_tree_cut_store(self._h, k, _ptr(pi), _ptr(pi0))
        return pi, pi0

    def close(self):
        for ref in getattr(self, '_sessions', []):   # (a session's buffers belong to the tree's context)
            if ref() is not None:
                ref().close()
        self._sessions = []
        if getattr(self, '_h', None) and getattr(self.problem, '_h', None):
            lib().mipx_tree_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Support:
    """The leaves of a disjunction resident on the device, and their support values for a cut direction
    (mipx_support, include/mipx_cglp.h)."""

    def __init__(self, tree, ids, duals=False):
        self.tree = tree
        self.duals = bool(duals)
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        h = _vp()
        if self.duals:
            rc = lib().mipx_tree_support_open_ex(tree._h, _ptr(ids), len(ids), SUPPORT_KEEP_DUALS, C.byref(h))
        else:
            rc = lib().mipx_tree_support_open(tree._h, _ptr(ids), len(ids), C.byref(h))
        tree.problem.ctx.check(rc, 'mipx_tree_support_open')
        self._h = h

    def eval(self, pi, pi0, tol=0.0, max_points=1, want_margins=False, screen_tol=None, retry_cold=False):
        """dict(min_margin, min_id, below, not_optimal, iterations, pivots, leaves, ids, h, x[, margins]): h_t(pi) of
        every leaf against pi0 and the (at most max_points) leaves of smallest margin h_t - pi0, in ascending
        order of (margin, node id), with a minimiser x of each (mipx_tree_support_eval).

        screen_tol (a number >= 0) screens the leaves by their stored duals first, retry_cold solves the leaves whose
        LP did not end optimal once more without a basis (mipx_tree_support_eval_ex, include/mipx_cglp_screen.h; both
        need a session opened with duals=True).  With either, the result also has screened, lp_solved,
        min_screened_margin, retried, retried_optimal and screen_us; a screened leaf among the rows carries its bound
        as h and a stale x."""
        n = self.tree.problem.n
        pi = np.ascontiguousarray(pi, np.float64).reshape(n)
        P = int(max_points)
        block = np.zeros(CGLP_HEAD + P * (n + 2))
        margins = np.zeros(self.leaves_count()) if want_margins else None
        extended = screen_tol is not None or retry_cold
        if extended:
            extra = np.zeros(len(CGLP_EXTRA_KEYS))
            rc = lib().mipx_tree_support_eval_ex(self._h, _ptr(pi), float(pi0), float(tol),
                                                 -1.0 if screen_tol is None else float(screen_tol), int(bool(retry_cold)), P,
                                                 _ptr(block), _ptr(margins), _ptr(extra))
            self.tree.problem.ctx.check(rc, 'mipx_tree_support_eval_ex')
        else:
            self.tree.problem.ctx.check(lib().mipx_tree_support_eval(self._h, _ptr(pi), float(pi0), float(tol), P, _ptr(block),
                                                                     _ptr(margins)), 'mipx_tree_support_eval')
        k = int(block[3])
        rows = block[CGLP_HEAD:CGLP_HEAD + k * (n + 2)].reshape(k, n + 2)
        out = dict(min_margin=float(block[0]), min_id=int(block[1]), below=int(block[2]), not_optimal=int(block[4]),
                   iterations=int(block[5]), pivots=int(block[6]), leaves=int(block[7]),
                   ids=rows[:, 0].astype(np.int64), h=rows[:, 1].copy(), x=rows[:, 2:].copy())
        if want_margins:
            out['margins'] = margins[:out['leaves']]
        if extended:
            out.update((key, float(v) if key in ('min_screened_margin', 'screen_us') else int(v))
                       for key, v in zip(CGLP_EXTRA_KEYS, extra))
        return out

    def leaves_count(self):
        return int(lib().mipx_tree_support_leaves(self._h, 0, 0, None))

    def leaves(self, dropped=False):
        """Node ids of the session's leaves, or of those dropped as infeasible (mipx_tree_support_leaves)."""
        k = int(lib().mipx_tree_support_leaves(self._h, int(bool(dropped)), 0, None))
        ids = np.zeros(max(k, 0), np.int64)
        lib().mipx_tree_support_leaves(self._h, int(bool(dropped)), k, _ptr(ids))
        return ids

    def stats(self):
        """dict(leaves, dropped, evaluations, leaf_lps, iterations, pivots, device_bytes, kernel_ms, select_ms)
        (mipx_tree_support_stats)."""
        out = np.zeros(9, np.int64)
        self.tree.problem.ctx.check(lib().mipx_tree_support_stats(self._h, _ptr(out)), 'mipx_tree_support_stats')
        d = dict(zip(CGLP_STATS_KEYS, (int(v) for v in out)))
        d['kernel_ms'] /= 1000.0
        d['select_ms'] /= 1000.0
        return d

    def close(self):
        if getattr(self, '_h', None) and getattr(self.tree, '_h', None):
            lib().mipx_tree_support_close(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def kernel_name(m, n):
    buf = C.create_string_buffer(128)
    rc = lib().mipx_kernel_name(int(m), int(n), buf, 128)
    if rc != MIPX_OK:
        raise MipxError(f'no on-chip kernel for m={m}, n={n}: {ERRORS.get(rc, rc)}')
    return buf.value.decode()


_default_ctx = None


def default_context():
    """Process-wide context on the GPU selected by LOCAL_RANK (one process per GPU)."""
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(int(os.environ.get('LOCAL_RANK', '0')))
    return _default_ctx


def debug_dump(problem, l, u, vstat=None, max_iter=0):
    """Test hook: solve one LP and return the kernel's final tableau state (see mipx.h)."""
    L = lib()
    problem.ctx.check(L.mipx_debug_enable(problem._h), 'mipx_debug_enable')
    res = problem.solve_batch(np.asarray(l, float)[None], np.asarray(u, float)[None],
                              None if vstat is None else np.asarray(vstat, np.int8)[None], max_iter)
    m, n = problem.m, problem.n
    T = np.zeros((m, n)); vec = np.zeros(n + 3 * m); idx = np.zeros(2 * n + m, np.int32)
    problem.ctx.check(L.mipx_debug_read(problem._h, _ptr(T), _ptr(vec), _ptr(idx)), 'mipx_debug_read')
    return res, dict(T=T, d=vec[:n], beta0=vec[n:n + m], ba=vec[n + m:n + 2 * m],
                     bb=vec[n + 2 * m:], nvar=idx[:n], bvar=idx[n:n + m], side=idx[n + m:])
