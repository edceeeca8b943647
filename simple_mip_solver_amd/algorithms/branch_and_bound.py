"""BranchAndBound driver and its tree.

Mirror of simple_mip_solver/algorithms/branch_and_bound.py:19-306: same constructor keywords,
validation messages, `solve()` semantics (re-entrant: a second call continues from the live
queue), status strings, `_kwargs` protocol and tree bookkeeping.  Nodes are duck-typed plugin
objects exactly as in the reference; the stock node classes of this package do their bounding on
the MI355X engine.

Deviations: wall-clock instead of CPU-clock time limits (GPU work does not advance
time.process_time); the root dual bound used by the gap test is tracked incrementally instead of
re-scanning every tree vertex up to four times per iteration (reference :199-213, :226-229) --
same value, O(log N) instead of O(N).
"""
import heapq
import os
from queue import PriorityQueue
import time

import numpy as np

from simple_mip_solver_amd.algorithms.base_algorithm import BaseAlgorithm
from simple_mip_solver_amd.lp import Constraint, CyLPArray, DenseLP
from simple_mip_solver_amd.nodes.base_node import BaseNode
from simple_mip_solver_amd.utils.binary_tree import BinaryTree

from simple_mip_solver_amd.nodes.branch.pseudo_cost import PseudoCostBranchNode
from simple_mip_solver_amd.nodes.search.depth_first import DepthFirstSearchNode
from simple_mip_solver_amd.nodes.nodes import PseudoCostBranchDepthFirstSearchNode

INF = float('inf')
_NATIVE_NODES = (BaseNode, PseudoCostBranchNode, DepthFirstSearchNode,
                 PseudoCostBranchDepthFirstSearchNode)


def _leaf_value(node):
    return node.objective_value if node.objective_value is not None else node.dual_bound


class BranchAndBoundTree(BinaryTree):
    """Search tree; every vertex carries its Node under attr['node'] (reference :19-108)."""

    def get_leaves(self, subtree_root_id, depth=None, keep='all'):
        """Leaves of the subtree under subtree_root_id, optionally after cutting everything more
        than `depth` edges below it.  keep: 'all' | 'feasible' | 'not infeasible'."""
        assert subtree_root_id in self, 'subtree_root_id must belong to the tree'
        assert keep in ['all', 'feasible', 'not infeasible'], \
            "keep is one of 'all', 'feasible', or 'not infeasible'"
        everyone = [v.attr['node'] for v in self.nodes.values()]
        if depth is None:
            found = [n for n in everyone if n.is_leaf and subtree_root_id in n.lineage]
        else:
            assert isinstance(depth, int) and depth >= 0, 'depth is a nonnegative integer'
            if depth == 0:
                found = self.get_node_instances([subtree_root_id])
            elif depth == 1:
                found = self.get_node_instances(self.get_children(subtree_root_id))
            else:
                shallow = [n for n in everyone
                           if n.is_leaf and subtree_root_id in n.lineage[-depth:]]
                at_depth = [n for n in everyone if len(n.lineage) >= depth + 1 and
                            n.lineage[-(depth + 1)] == subtree_root_id]
                found = shallow + at_depth
        if keep == 'feasible':
            return [n for n in found if n.lp_feasible]
        if keep == 'not infeasible':
            return [n for n in found if n.lp_feasible is not False]
        return found

    def get_disjunction(self, subtree_root_id):
        """{leaf idx: (lower bounds, upper bounds)} over the not-infeasible leaves."""
        return {n.idx: (n.lp.variablesLower.copy(), n.lp.variablesUpper.copy())
                for n in self.get_leaves(subtree_root_id, keep='not infeasible')}

    def get_node_instances(self, node_ids):
        single = isinstance(node_ids, int)
        if single:
            node_ids = [node_ids]
        else:
            assert hasattr(node_ids, '__iter__') and not isinstance(node_ids, str), \
                'node_ids must be an integer or iterable (that is not a string)'
            node_ids = list(node_ids)
        missing = set(node_ids) - set(self.nodes)
        assert not missing, f'the following node_ids are not in the tree: {missing}'
        found = [self.nodes[i].attr.get('node') for i in node_ids]
        assert all(n is not None for n in found), \
            'each vertex in the branch and bound tree must have an attribute for a node instance'
        return found[0] if single else found

    def subtree_dual_bound(self, subtree_root_id, depth=None):
        """min over the subtree's leaves of their LP objective (or inherited bound if unsolved)."""
        assert subtree_root_id in self, 'subtree_root_id must belong to the tree'
        return min(_leaf_value(n) for n in self.get_leaves(subtree_root_id, depth=depth))


class _LeafBounds:
    """Lazy min-heap over leaf values: same answer as scanning all leaves of the root."""

    def __init__(self):
        self._heap = []
        self._count = 0

    def push(self, node):
        self._count += 1
        heapq.heappush(self._heap, (_leaf_value(node), self._count, node))

    def minimum(self):
        while self._heap:
            value, _, node = self._heap[0]
            if node.is_leaf and _leaf_value(node) == value:
                return value
            heapq.heappop(self._heap)  # stale: the node was branched on or re-valued
        return INF


class BranchAndBound(BaseAlgorithm):
    """Solve a MILP by branch and bound with the bound / branch / search rules of a Node class."""

    _node_attributes = ['dual_bound', 'objective_value', 'solution', 'lp_feasible',
                        'mip_feasible', 'search_method', 'branch_method', 'idx', 'lp',
                        'is_leaf', 'lineage']
    _node_funcs = ['bound', 'branch', '__lt__', '__eq__']
    _queue_funcs = ['put', 'get', 'empty']

    def __init__(self, model, Node=BaseNode, node_queue=None, node_limit=INF, mip_gap=.0001,
                 logging=False, max_run_time=INF, initial_primal_bound=INF, frontier_batch=None,
                 lp_batch=None, pool_capacity=1 << 16, anchor=None, dive=None, comm=None, exchange_every=5,
                 host_spill=None, cut_migration=None, dual_function=None, tree_record=None, primal_heuristic=None,
                 propagate=None, reduced_cost=None, objective_step=None, local_search=None, fix_propagate=None,
                 weighted_repair=None, cube_search=None, complete_continuous=None, lp_dive=None, lp_dive_every=None,
                 root_cuts=None, root_cut_rows=None, cover_cuts=None, clique_cuts=None, **kwargs):
        """All problems are converted to minimisation with A x >= b on the way in.  **kwargs are
        handed to every bound()/branch() call and refreshed from what those calls return
        (e.g. pseudo_costs={}, strong_branch_iters=5, gomory_cuts=False).

        frontier_batch (extension, default None = the reference's one-node-at-a-time Python
        loop): run the whole search in the native frontier engine (mipx_tree_*), evaluating that
        many open nodes per GPU step with node records resident in HBM.  Only for the stock node
        classes and the default queue; frontier_batch=1 keeps the reference's exact node order.
        With gomory_cuts=True (the reference's default, base_node.py:365) every node runs the cut
        rounds of BaseNode._base_bound inside the engine (register-tile shapes: m + 64 <= 192 rows,
        n <= 256; no dive then).  In this mode `tree` holds only the root (nodes live on the device) unless
        tree_record is on.
        comm (extension; needs frontier_batch): an _ffi.Comm shared by one process per GPU
        (simple_mip_solver_amd.parallel.init_comm).  Every rank builds the same BranchAndBound and
        calls solve(): after a replicated ramp-up the open nodes are sharded over the ranks, which
        exchange incumbent (value and solution), bounds, pseudo costs and node records every
        `exchange_every` steps over RCCL; every rank ends with the same status, objective_value and
        solution; evaluated_nodes is the total over all ranks.  With gomory_cuts=True open nodes move
        between ranks only with cut_migration.
        cut_migration (extension; needs comm and gomory_cuts=True; default None = off): open nodes migrate
        between ranks in cut-round mode too, carrying their cut rows (include/mipx_cutmig.h).  The top rows
        of every rank's cut store are reserved for the rows it receives: True reserves 2**16 rows, an int
        that many (below the store's 2**20 rows); the rank's own cuts stop that much sooner.  Every rank
        must pass the same setting, or no node moves.  Counters: `cut_migration_stats`.
        anchor / dive (default: on for frontier_batch > 1, register-tile shapes): warm starts
        refactor from the root's optimal tableau instead of the slack basis; the workgroup that
        solved a node also solves one child on the tableau it holds (same optimum, another node
        order -- see DESIGN.md section 4).
        lp_batch (extension, default None): keep the one-node-at-a-time Python loop, with any Node class
        and any node_queue, but take up to lp_batch nodes from the queue per step and solve the first LP
        of all of them that their inherited bound does not prune in one engine launch per row set
        (with the integrality scan K4 beside it).  The nodes are then evaluated in the order they were
        taken, by the unchanged bound / branch methods; `lp.dual()` takes the result solved ahead for
        it only if the LP is still exactly what was solved (rows, bounds, basis, iteration limit), and
        solves as before otherwise.  Cut-round re-solves, strong-branching probes and LPs with free
        columns stay per node.  lp_batch=1 evaluates the same nodes as the default; a larger batch
        finds the same status and optimum in another order.  Counters: `lp_batch_stats`.
        host_spill (extension; needs frontier_batch, not with comm; default None = off): when the
        device node pool runs low, the open nodes the queue pops last move to pinned host memory as
        compact records and come back when they are popped, so the search goes on instead of stopping
        (include/mipx_spill.h).  The nodes evaluated and their order are those of a pool that never
        fills.  True caps the host store at half of the physical memory, an int at that many bytes; the
        search stops (RuntimeWarning, as with a full pool) only when the cap is reached.  pool_capacity
        must be at least 2 H + 1 rows, H = 3 x frontier_batch x (2 (1 + dive) + 1) (x 1 for
        frontier_batch = 1).  Counters: `spill_stats`.
        dual_function (extension; needs frontier_batch and gomory_cuts=False, not with comm; default None =
        off): the engine records one dual term per node it solves (row duals y and the bound term t, in
        device memory), so that find_parameterized_dual_bound(s) works after solve() as on the Python
        path (include/mipx_dualfn.h).  True caps the store at half of the device memory free when the
        search starts, an int at that many bytes; once the cap is reached the search goes on and later
        nodes get no term (their leaves use their ancestors' terms: a valid, weaker bound; counted as
        `dropped`, RuntimeWarning).  Every step is then finished on the host.  Counters:
        `dual_function_stats`.
        tree_record (extension; needs frontier_batch and gomory_cuts=False, not with comm; default None = off):
        True makes the engine keep one record per node it creates (parent, branching, LP verdict and
        objective: 14 bytes of host memory per node, include/mipx_treerec.h), and after every solve() `tree`
        answers the reference's queries for the whole native search -- `in`, get_children, get_leaves,
        get_disjunction, get_node_instances, subtree_dual_bound, and so CutGeneratingLP(bb, root_id).  Node
        objects are built for the nodes a query returns, their bounds rebuilt on the GPU from the records;
        get_node_instances also fills `solution` of the LP-feasible nodes it returns, by one batched re-solve
        (`tree.fill_solutions(nodes)` does so for any list of nodes).  Every step is then finished on the
        host.  Counters: `tree_record_stats`.
        primal_heuristic (extension; needs frontier_batch and gomory_cuts=False, not with comm; default None = off):
        after the node LPs of every step the engine rounds the LP solutions of the step's first nodes to integers,
        repairs the rows the rounding broke by unit moves and lifts the objective by unit moves that keep every
        row, one GPU workgroup per point (include/mipx_heur.h); the best feasible point becomes the incumbent
        where it beats the one the search holds, before the step's nodes are pruned against it.  True takes 32
        points per step, an int that many; at most m + n moves per point.  The optimum is the same; the nodes
        evaluated on the way differ.  Every step is then finished on the host.  Counters: `heuristic_stats`.
        propagate (extension; needs frontier_batch and gomory_cuts=False, not with comm, dual_function or
        tree_record; default None = off): node presolve.  Before the node LPs of every step the engine tightens
        the bounds of the step's nodes by activity-based bound propagation over the rows, the incumbent's
        objective as one more row, one GPU workgroup per node (include/mipx_prop.h), in place: the children of a
        node inherit what was tightened.  A node the propagation proves infeasible is closed as a node whose LP
        was infeasible.  True takes at most 8 rounds per node, an int that many.  The optimum is the same; the
        nodes evaluated on the way differ.  Every step is then finished on the host.  Counters:
        `propagation_stats`.
        reduced_cost (extension; needs frontier_batch and gomory_cuts=False, not with comm, dual_function or
        tree_record, so not with restart; default None = off): reduced-cost bound tightening.  The node LPs also
        write their row duals, and once the search holds an incumbent every node that branches has the bounds
        of its integer columns tightened from its reduced costs and the incumbent's objective, one GPU workgroup
        per node (include/mipx_rcfix.h), in place before its children are written: the whole subtree inherits
        them.  The optimum is the same; the nodes evaluated on the way differ.  Every step is then finished on
        the host.  Counters: `reduced_cost_stats`.
        objective_step (extension; needs frontier_batch and gomory_cuts=False, not with comm, dual_function or
        tree_record, so not with restart; default None = off): True or a positive float, the step by which the
        objective values of integer-feasible points differ (True: the gcd of the costs of a pure-integer objective,
        utils/objective_step.objective_step_of; a ValueError where that does not exist).  With an incumbent U
        the search then closes every node whose bound is above U - step (include/mipx_objstep.h) instead of only
        those at U or above, and counts such a node as a leaf of value U.  An initial_primal_bound must then be
        the objective of a feasible point.  The optimum is the same; the nodes evaluated on the way are fewer
        once an incumbent is known.  Every step is then finished on the host.  Counters: `objective_step_stats`.
        local_search (extension; needs primal_heuristic; default None = off): True or a positive number of moves.
        Every point the heuristic ends feasible on goes through a pair-move local search on the GPU right behind
        it (include/mipx_lsearch.h): unit moves of one integer column or of two at once that lower the objective
        and keep every row, the best first, at most that many per point (True: 64).  Inherited by restart()
        with primal_heuristic.  Counters: `local_search_stats`.
        fix_propagate (extension; needs primal_heuristic; default None = off): True or a positive number of tries.
        Every point the heuristic's rounding does not end feasible on goes through a fix-and-propagate dive on the
        GPU right behind it (include/mipx_fixprop.h): the integer columns are fixed one after the other, the most
        integral first, each to the value nearest the LP point that the bound propagation over the rows (the
        incumbent's objective as one more row) does not refuse, at most that many propagation calls per point
        (True: 256).  A point the dive ends feasible is lifted by the heuristic, goes through local_search when
        that is on, and competes for the step's incumbent.  Inherited by restart() with primal_heuristic.
        Counters: `fix_propagate_stats`.
        weighted_repair (extension; needs primal_heuristic; not with fix_propagate; default None = off): True or a
        positive number of steps.  Every point the heuristic's rounding does not end feasible on goes through a
        weighted row repair on the GPU right behind it (include/mipx_wrepair.h): the heuristic's own unit moves, but
        every row carries a weight, and where no move lowers the weighted violation the weights of the violated rows
        go up by one, at most that many moves and bumps per point (True: 256).  A point it ends feasible is lifted
        by the heuristic, goes through local_search when that is on, and competes for the step's incumbent.
        Inherited by restart() with primal_heuristic.  Counters: `weighted_repair_stats`.
        cube_search (extension; needs primal_heuristic; default None = off): True or a number of columns from 1 to
        20.  In every step the heuristic runs in, the same LP points go through a cube search on the GPU
        (include/mipx_cube.h): the at most that many most fractional integer columns (True: 16) are rounded down
        and up in every combination, every other integer column held where the rounding puts it, and the best
        combination that satisfies every row and lies below the cutoff is the point.  It is lifted by the
        heuristic, goes through local_search when that is on, and competes for the step's incumbent beside the
        heuristic's points and those of fix_propagate or weighted_repair.  Inherited by restart() with
        primal_heuristic.  Counters: `cube_search_stats`.
        complete_continuous (extension; needs primal_heuristic; default None = off): True.  The heuristics above move
        integer columns only and leave a continuous column at its value in the node's LP point.  With this option
        every point they end on, feasible or not, has its integer columns held and the LP over the other columns
        solved on the GPU (include/mipx_complete.h), all points of a step in one launch, warm from the basis of the
        node LP the point came from.  A completed point (every row within 1e-6) takes its source's place in the
        contest for the step's incumbent.  On a model without continuous columns nothing is launched.  Inherited by
        restart() with primal_heuristic.  Counters: `completion_stats`.
        lp_dive (extension; needs primal_heuristic; default None = off): True (64 rounds) or the round cap 1..1024.
        An LP dive on the GPU (include/mipx_lpdive.h) from the LP point of each of the step's first nodes, inside that
        node's bounds: fix one fractional integer column at its rounding, re-solve all the points' LPs in one
        warm-started launch of the node-LP kernel so that the continuous columns and the other integers adapt, flip
        the fixing once where the LP turns infeasible, and repeat until every integer column is integral; the point
        is then completed and checked as complete_continuous does.  It runs in the steps in which the search holds no
        incumbent, and with lp_dive_every=k (a positive integer; default None) in every k-th step as well.  A feasible
        point competes for the step's incumbent behind the other families.  Inherited by restart() with
        primal_heuristic.  Counters: `lp_dive_stats`.
        root_cuts (extension; needs frontier_batch and gomory_cuts=False, not with comm, dual_function or tree_record,
        so not with restart; default None = off): True (10 rounds) or a positive number of rounds.  Before the search
        starts, rounds of mixed-integer rounding cuts are separated at the root on the GPU (include/mipx_mir.h,
        utils/mir_cuts.root_cut_loop): the model's rows and the tableau rows of the fractional basic integer columns
        are the base rows, one workgroup each; the cuts kept, at most root_cut_rows (default 64) of them, are
        appended to the rows the engine searches on, so every other option sees an ordinary model with m + k rows.
        The cuts are valid by construction: the optimum is the same, the root bound is at least as good, the nodes
        evaluated differ.  `model`, `solution` and every other attribute are those of the model as given.
        `root_cuts` is then the list of (pi, pi0) kept (pi . x >= pi0); counters: `root_cut_stats`.
        cover_cuts (extension; needs root_cuts; default None = off): True.  Every round of the root cut loop also
        separates lifted knapsack cover cuts from the model's rows on the GPU (include/mipx_cover.h), one workgroup
        per row, and they compete with the MIR cuts for the round's places.  `root_cuts` then holds both kinds, and
        `root_cut_stats` counts the MIR cuts selected and kept; counters of the cover cuts: `cover_cut_stats`.
        clique_cuts (extension; needs root_cuts; default None = off): True.  Before the first round the conflict graph
        of the model's rows is built on the GPU (include/mipx_clique.h: two literals x_j - l_j or u_j - x_j of binaries
        are joined when one row alone keeps them from both being 1), and every round of the root cut loop also grows a
        clique from each literal at the round's point, one workgroup per literal; the distinct cuts compete with the
        MIR cuts (and the cover cuts, with cover_cuts) for the round's places.  `root_cuts` then holds all kinds;
        counters of the clique cuts: `clique_cut_stats`.  On a model without binaries that share rows it finds nothing
        and changes nothing."""
        assert lp_batch is None or (isinstance(lp_batch, int) and not isinstance(lp_batch, bool) and
                                    lp_batch > 0), 'lp_batch must be a positive integer'
        assert lp_batch is None or frontier_batch is None, \
            'lp_batch batches the Python loop; it cannot be combined with frontier_batch'
        assert lp_batch is None or comm is None, \
            'lp_batch runs on one GPU; it cannot be combined with comm'
        # what restart() hands to the search it makes: the options as given, the node kwargs before any call
        self._given = dict(node_limit=node_limit, mip_gap=mip_gap, logging=logging, max_run_time=max_run_time,
                           frontier_batch=frontier_batch, pool_capacity=pool_capacity, anchor=anchor, dive=dive,
                           host_spill=host_spill, tree_record=tree_record, primal_heuristic=primal_heuristic,
                           local_search=local_search, fix_propagate=fix_propagate, weighted_repair=weighted_repair,
                           cube_search=cube_search, complete_continuous=complete_continuous, lp_dive=lp_dive,
                           lp_dive_every=lp_dive_every)
        self._given_kwargs = dict(kwargs)
        self.restart_stats = None
        self.lp_batch = lp_batch
        self.lp_batch_stats = None if lp_batch is None else \
            dict(launches=0, prefetched=0, consumed=0, wasted=0)
        self._pending = []   # nodes taken from the queue in this lp_batch step, not yet evaluated
        self._native = None
        self._native_stats = None
        assert comm is None or frontier_batch is not None, 'comm needs frontier_batch'
        assert host_spill is None or host_spill is True or (
            isinstance(host_spill, int) and not isinstance(host_spill, bool) and host_spill > 0), \
            'host_spill is None, True or a positive number of bytes'
        assert host_spill is None or frontier_batch is not None, 'host_spill needs frontier_batch'
        assert host_spill is None or comm is None, 'host_spill cannot be combined with comm'
        assert cut_migration is None or cut_migration is True or (
            isinstance(cut_migration, int) and not isinstance(cut_migration, bool) and cut_migration > 0), \
            'cut_migration is None, True or a positive number of rows'
        assert cut_migration is None or comm is not None, 'cut_migration needs comm'
        assert cut_migration is None or kwargs.get('gomory_cuts', True) is True, 'cut_migration needs gomory_cuts=True'
        self._cut_migration = cut_migration
        self.cut_migration_stats = None
        assert dual_function is None or dual_function is True or (
            isinstance(dual_function, int) and not isinstance(dual_function, bool) and dual_function > 0), \
            'dual_function is None, True or a positive number of bytes'
        assert dual_function is None or frontier_batch is not None, \
            'dual_function needs frontier_batch (the Python loop keeps every node LP)'
        assert dual_function is None or comm is None, 'dual_function cannot be combined with comm'
        assert dual_function is None or kwargs.get('gomory_cuts', True) is False, \
            'dual_function needs gomory_cuts=False: the dual function does not cover nodes with cut rows'
        self._dual_function = dual_function
        self.dual_function_stats = None
        assert tree_record is None or tree_record is True, 'tree_record is None or True'
        assert tree_record is None or frontier_batch is not None, \
            'tree_record needs frontier_batch (the Python loop keeps every node in its tree)'
        assert tree_record is None or comm is None, 'tree_record cannot be combined with comm'
        assert tree_record is None or kwargs.get('gomory_cuts', True) is False, \
            'tree_record needs gomory_cuts=False: recorded nodes carry no cut rows'
        self._tree_record = tree_record
        self.tree_record_stats = None
        assert primal_heuristic is None or primal_heuristic is True or (
            isinstance(primal_heuristic, int) and not isinstance(primal_heuristic, bool) and primal_heuristic > 0), \
            'primal_heuristic is None, True or a positive number of points per step'
        assert primal_heuristic is None or frontier_batch is not None, \
            'primal_heuristic needs frontier_batch (it runs on the node LP solutions of the native engine)'
        assert primal_heuristic is None or comm is None, 'primal_heuristic cannot be combined with comm'
        assert primal_heuristic is None or kwargs.get('gomory_cuts', True) is False, \
            'primal_heuristic needs gomory_cuts=False: the heuristic does not run on nodes with cut rows'
        self._primal_heuristic = primal_heuristic
        self.heuristic_stats = None
        assert propagate is None or propagate is True or (
            isinstance(propagate, int) and not isinstance(propagate, bool) and propagate > 0), \
            'propagate is None, True or a positive number of rounds'
        assert propagate is None or frontier_batch is not None, \
            'propagate needs frontier_batch (it runs on the pool rows of the native engine)'
        assert propagate is None or comm is None, 'propagate cannot be combined with comm'
        assert propagate is None or kwargs.get('gomory_cuts', True) is False, \
            'propagate needs gomory_cuts=False: the propagation does not see the cut rows of a node'
        assert propagate is None or not dual_function, \
            'propagate cannot be combined with dual_function: a propagated bound depends on the right-hand side'
        assert propagate is None or not tree_record, \
            'propagate cannot be combined with tree_record: bounds rebuilt from a lineage would miss the propagated ones'
        self._propagate = propagate
        self.propagation_stats = None
        assert reduced_cost is None or reduced_cost is True, 'reduced_cost is None or True'
        assert reduced_cost is None or frontier_batch is not None, \
            'reduced_cost needs frontier_batch (it runs on the pool rows of the native engine)'
        assert reduced_cost is None or comm is None, 'reduced_cost cannot be combined with comm'
        assert reduced_cost is None or kwargs.get('gomory_cuts', True) is False, \
            'reduced_cost needs gomory_cuts=False: the tightening does not see the cut rows of a node'
        assert reduced_cost is None or not dual_function, \
            'reduced_cost cannot be combined with dual_function: a tightened bound depends on the right-hand side'
        assert reduced_cost is None or not tree_record, \
            'reduced_cost cannot be combined with tree_record (and so with restart): bounds rebuilt from a lineage ' \
            'would miss the tightened ones'
        self._reduced_cost = reduced_cost
        self.reduced_cost_stats = None
        assert objective_step is None or objective_step is True or (
            isinstance(objective_step, (int, float)) and not isinstance(objective_step, bool) and
            0 < objective_step < INF), 'objective_step is None, True or a positive finite step'
        assert objective_step is None or frontier_batch is not None, \
            'objective_step needs frontier_batch (it is a cutoff of the native engine)'
        assert objective_step is None or comm is None, 'objective_step cannot be combined with comm'
        assert objective_step is None or kwargs.get('gomory_cuts', True) is False, \
            'objective_step needs gomory_cuts=False: cut-round trees are finished another way'
        assert objective_step is None or not dual_function, \
            'objective_step cannot be combined with dual_function: a recorded bound would depend on the incumbent'
        assert objective_step is None or not tree_record, \
            'objective_step cannot be combined with tree_record (and so with restart): a recorded bound would ' \
            'depend on the incumbent'
        self._objective_step = objective_step
        self.objective_step_stats = None
        assert local_search is None or local_search is True or (
            isinstance(local_search, int) and not isinstance(local_search, bool) and local_search > 0), \
            'local_search is None, True or a positive number of moves per point'
        assert local_search is None or primal_heuristic is not None, \
            'local_search needs primal_heuristic (it runs on the points the heuristic ends feasible on)'
        self._local_search = local_search
        self.local_search_stats = None
        assert fix_propagate is None or fix_propagate is True or (
            isinstance(fix_propagate, int) and not isinstance(fix_propagate, bool) and fix_propagate > 0), \
            'fix_propagate is None, True or a positive number of tries per point'
        assert fix_propagate is None or primal_heuristic is not None, \
            'fix_propagate needs primal_heuristic (it runs on the points the heuristic does not end feasible on)'
        self._fix_propagate = fix_propagate
        self.fix_propagate_stats = None
        assert weighted_repair is None or weighted_repair is True or (
            isinstance(weighted_repair, int) and not isinstance(weighted_repair, bool) and weighted_repair > 0), \
            'weighted_repair is None, True or a positive number of steps per point'
        assert weighted_repair is None or primal_heuristic is not None, \
            'weighted_repair needs primal_heuristic (it runs on the points the heuristic does not end feasible on)'
        assert weighted_repair is None or fix_propagate is None, \
            'weighted_repair cannot be combined with fix_propagate (both take the points the heuristic does not end ' \
            'feasible on, and running one behind the other is not built: choose one)'
        self._weighted_repair = weighted_repair
        self.weighted_repair_stats = None
        if not (cube_search is None or cube_search is True or (
                isinstance(cube_search, int) and not isinstance(cube_search, bool) and 1 <= cube_search <= 20)):
            raise ValueError('cube_search is None, True or a number of columns from 1 to 20')
        if cube_search is not None and primal_heuristic is None:
            raise ValueError('cube_search needs primal_heuristic (it runs on the LP points the heuristic takes)')
        self._cube_search = cube_search
        self.cube_search_stats = None
        if not (complete_continuous is None or complete_continuous is True):
            raise ValueError('complete_continuous is None or True')
        if complete_continuous is not None and primal_heuristic is None:
            raise ValueError('complete_continuous needs primal_heuristic (it completes the points the heuristics end on)')
        self._complete_continuous = complete_continuous
        self.completion_stats = None
        if not (lp_dive is None or lp_dive is True or (isinstance(lp_dive, int) and not isinstance(lp_dive, bool) and
                                                        1 <= lp_dive <= 1024)):
            raise ValueError('lp_dive is None, True or a round cap from 1 to 1024')
        if not (lp_dive_every is None or (isinstance(lp_dive_every, int) and not isinstance(lp_dive_every, bool) and
                                          lp_dive_every > 0)):
            raise ValueError('lp_dive_every is None or a positive integer')
        if lp_dive is not None and primal_heuristic is None:
            raise ValueError('lp_dive needs primal_heuristic (it dives from the LP points the heuristic takes)')
        if lp_dive_every is not None and lp_dive is None:
            raise ValueError('lp_dive_every needs lp_dive')
        self._lp_dive = lp_dive
        self._lp_dive_every = lp_dive_every
        self.lp_dive_stats = None
        assert root_cuts is None or root_cuts is True or (
            isinstance(root_cuts, int) and not isinstance(root_cuts, bool) and root_cuts > 0), \
            'root_cuts is None, True or a positive number of rounds'
        assert root_cut_rows is None or (isinstance(root_cut_rows, int) and not isinstance(root_cut_rows, bool) and
                                         root_cut_rows > 0), 'root_cut_rows is None or a positive number of rows'
        assert root_cut_rows is None or root_cuts is not None, 'root_cut_rows needs root_cuts'
        assert root_cuts is None or frontier_batch is not None, \
            'root_cuts needs frontier_batch (the cut rows are appended to the rows of the native engine)'
        assert root_cuts is None or comm is None, 'root_cuts cannot be combined with comm'
        assert root_cuts is None or kwargs.get('gomory_cuts', True) is False, \
            'root_cuts needs gomory_cuts=False: the cut rounds of a node keep their own rows'
        assert root_cuts is None or not dual_function, \
            'root_cuts cannot be combined with dual_function: a cut depends on the right-hand side'
        assert root_cuts is None or not tree_record, \
            'root_cuts cannot be combined with tree_record (and so with restart): a cut depends on the right-hand side'
        assert cover_cuts is None or cover_cuts is True, 'cover_cuts is None or True'
        assert cover_cuts is None or root_cuts is not None, 'cover_cuts needs root_cuts'
        assert clique_cuts is None or clique_cuts is True, 'clique_cuts is None or True'
        assert clique_cuts is None or root_cuts is not None, 'clique_cuts needs root_cuts'
        self._root_cuts = 10 if root_cuts is True else root_cuts
        self._cover_cuts = cover_cuts is True
        self.cover_cut_stats = None
        self._clique_cuts = clique_cuts is True
        self.clique_cut_stats = None
        self._root_cut_rows = 64 if root_cut_rows is None else root_cut_rows
        self.root_cuts = None
        self.root_cut_stats = None
        if host_spill is True:
            host_spill = os.sysconf('SC_PAGE_SIZE') * os.sysconf('SC_PHYS_PAGES') // 2
        self._host_spill = host_spill
        self.spill_stats = None
        self._comm, self._exchange_every, self._sharded = comm, exchange_every, False
        if frontier_batch is not None:
            assert isinstance(frontier_batch, int) and frontier_batch > 0, \
                'frontier_batch must be a positive integer'
            assert node_queue is None, 'frontier_batch needs the default node queue'
            assert Node in _NATIVE_NODES, \
                'frontier_batch is only available for the stock node classes'
            assert isinstance(kwargs.get('gomory_cuts', True), bool), 'gomory_cuts is boolean'
        self.frontier_batch = frontier_batch
        batched = frontier_batch is not None and frontier_batch > 1
        native_cuts = frontier_batch is not None and kwargs.get('gomory_cuts', True)
        self._anchor = batched if anchor is None else bool(anchor)
        # dive: False / 0 off, True / 1 one dive child per node, an int up to 8 that many in a row
        self._dive = int(batched and not native_cuts) if dive is None else int(dive)
        assert 0 <= self._dive <= 8, 'dive is a depth between 0 and 8'
        assert not (self._dive and native_cuts), 'dive is not available with gomory_cuts=True'
        assert not (self._dive and not batched), 'dive needs frontier_batch > 1'
        self._pool_capacity = pool_capacity
        node_queue = node_queue or PriorityQueue()
        super().__init__(model=model, Node=Node, node_attributes=self._node_attributes,
                         node_funcs=self._node_funcs, **kwargs)

        for func in self._queue_funcs:
            assert callable(getattr(node_queue, func, None)), f'node_queue needs a {func} function'
        assert node_limit == INF or (isinstance(node_limit, int) and node_limit > 0), \
            "node limit must be positive integer or infinity"
        assert 0 <= mip_gap < 1, 'mip_gap is a ratio between 0 and 1'
        assert isinstance(logging, bool), 'logging is boolean'
        assert max_run_time > 0, 'max_run_time is positive value'
        assert initial_primal_bound > -INF, 'initial_primal_bound is real or infinite'
        special_keys = {'right', 'left', 'cuts'}
        assert set(kwargs.keys()).isdisjoint(special_keys), \
            f'keys {special_keys} are saved for later use'
        assert all(isinstance(k, str) for k in kwargs), 'kwargs keys must be strings'

        self._node_queue = node_queue
        self._unbounded = None
        self._best_solution = None
        self.solution = None
        self.status = 'unsolved'
        self.objective_value = None
        self.primal_bound = initial_primal_bound
        self.node_limit = node_limit
        self.tree = BranchAndBoundTree()
        self.tree.add_root(self.root_node.idx, node=self.root_node)
        self._leaf_bounds = _LeafBounds()
        self._leaf_bounds.push(self.root_node)
        self.solve_time = 0
        self.mip_gap = mip_gap
        self.logging = logging
        self.max_run_time = max_run_time
        if self._objective_step is True:   # (the gcd of the costs, or a ValueError that asks for the step)
            from simple_mip_solver_amd.utils.objective_step import objective_step_of
            self._objective_step = objective_step_of(self)

    @property
    def dual_bound(self):
        if self._native_stats is not None:
            return self._native_stats['dual_bound']
        return self._leaf_bounds.minimum()

    @property
    def current_gap(self):
        """|primal - dual| / |primal|; None until an incumbent exists (reference :203-213)."""
        primal, dual = self.primal_bound, self.dual_bound
        if primal == dual == 0:
            return 0
        if primal == 0:
            return INF
        if primal == INF:
            return None
        return abs(primal - dual) / abs(primal)

    def _gap_closed(self):
        gap = self.current_gap
        return gap is not None and gap <= self.mip_gap

    def solve(self):
        """Run (or continue) the search until the queue empties, the problem proves unbounded, or
        the node / gap / time limit is hit (reference :215-241)."""
        if self.frontier_batch is not None:
            return self._solve_native()
        start = time.perf_counter()
        if self.status == 'unsolved':
            self._node_queue.put(self.root_node)

        while not (self._node_queue.empty() or self._unbounded or
                   self.evaluated_nodes >= self.node_limit or self._gap_closed() or
                   time.perf_counter() - start > self.max_run_time):
            if self.logging and self.evaluated_nodes % 100 == 0:
                print(f'{self.evaluated_nodes} nodes evaluated gap: {self.current_gap}')
            if self.lp_batch is None:
                self._evaluate_node(self._node_queue.get())
            else:
                self._evaluate_batch(start)

        self.solve_time += time.perf_counter() - start
        if self._unbounded:
            self.status = 'unbounded'
        elif self._node_queue.empty() and self.primal_bound == INF:
            self.status = 'infeasible'
        elif self.primal_bound < INF and self.current_gap <= self.mip_gap:
            self.status = 'optimal'
        else:
            self.status = 'stopped on iterations or time'
        self.solution = self._best_solution
        self.objective_value = self.primal_bound

    def _solve_native(self):
        """The same search, run by the native frontier engine (include/mipx.h mipx_tree_*)."""
        from simple_mip_solver_amd import _ffi
        from simple_mip_solver_amd.lp import get_backend, HipBackend
        if self._native is None:
            self._native_totals0 = {k: self._kwargs.get(k, 0) for k in _ffi.CUT_TOTAL_KEYS}
            backend = get_backend()
            assert isinstance(backend, HipBackend), 'frontier_batch needs the HIP backend'
            lp = self.root_node.lp
            rs = lp._engine_form()
            l, u = lp._bounds()
            if self._root_cuts:
                # the rows the engine searches on: the model's and the cuts the root loop keeps; everything behind
                # this point sees an ordinary model (the key names the cut rows, so another row set is another problem)
                from simple_mip_solver_amd.utils.mir_cuts import root_cut_loop
                loop = root_cut_loop(rs.A, rs.b, rs.c, l, u, self.model.integerIndices, rounds=self._root_cuts,
                                     max_rows=self._root_cut_rows, cover=self._cover_cuts, clique=self._clique_cuts)
                self.root_cuts = loop['cuts']
                self.root_cut_stats = loop['stats']
                self.cover_cut_stats = loop.get('cover_stats')
                self.clique_cut_stats = loop.get('clique_stats')
                problem = backend._problem(loop['A'], loop['b'], rs.c, ('root_cuts', rs.key, loop['A'][rs.A.shape[0]:].tobytes(),
                                                                      loop['b'][rs.A.shape[0]:].tobytes()))
            else:
                problem = backend._problem(rs.A, rs.b, rs.c, rs.key)
            pseudo = issubclass(self._Node, PseudoCostBranchNode)
            cut_params = None
            if self._kwargs.get('gomory_cuts', True):
                # the keyword defaults of BaseNode._base_bound / _cut_generation_iteration / _select_cuts
                # (base_node.py:137, :292, :387), overridable through **kwargs as there
                from math import cos, radians
                from simple_mip_solver_amd.utils import tolerance as tol
                kw = self._kwargs
                rounds = kw.get('max_cut_generation_iterations', tol.max_cut_generation_iterations)
                cut_params = dict(
                    max_cut_generation_iterations=int(min(rounds, 2 ** 31 - 1)),
                    max_nonzero_coefs=int(min(kw.get('max_nonzero_coefs', tol.max_nonzero_coefs), 2 ** 31 - 1)),
                    cutting_plane_progress_tolerance=kw.get('cutting_plane_progress_tolerance',
                                                            tol.cutting_plane_progress_tolerance),
                    min_cut_depth=kw.get('min_cut_depth', tol.min_cut_depth),
                    cos_parallel=cos(radians(kw.get('parallel_cut_tolerance', tol.parallel_cut_tolerance))),
                    max_abs_coef=kw.get('max_relative_cut_term_ratio', tol.max_relative_cut_term_ratio) *
                    float(self.root_node.max_term),
                    max_term=tol.max_term, max_dual_bound=kw.get('max_dual_bound', INF),
                    exact_tableau=0 if self._anchor else 1)
            self._native = _ffi.Tree(
                problem, self.model.integerIndices, l, u,
                branch_rule='pseudo cost' if pseudo else 'most fractional',
                search_rule=self.root_node.search_method,
                strong_branch_iters=self._kwargs.get('strong_branch_iters', 5),
                max_batch=self.frontier_batch, pool_capacity=self._pool_capacity, cut_params=cut_params)
            if self.primal_bound < INF:
                self._native.set_primal_bound(self.primal_bound)
            table = self._kwargs.get('pseudo_costs')
            if pseudo and table:
                # a table handed in by the caller (pseudo_cost.py:22: `pseudo_costs` is an input of
                # bound) seeds the engine's; an entry counts as present once either side was visited
                n = problem.n
                cl, cr = np.zeros(n), np.zeros(n)
                tl, tr = np.zeros(n, np.int32), np.zeros(n, np.int32)
                for i, rec in table.items():
                    cl[i], tl[i] = rec['left']['cost'], rec['left']['times']
                    cr[i], tr[i] = rec['right']['cost'], rec['right']['times']
                self._native.set_pseudo_cost_arrays(cl, cr, tl, tr)
            if self._anchor:
                self._native.set_anchor_mode(True)
            if self._dive:
                self._native.set_dive(self._dive)
            if self._host_spill:
                self._native.set_host_spill(self._host_spill)
            if self._cut_migration:
                self._native.set_cut_migration(self._cut_migration)
            if self._dual_function:
                pos, plus = lp._row_index()   # (True: -1, half of the device memory free now)
                self._native.set_dual_record(-1 if self._dual_function is True else self._dual_function,
                                             lp.nConstraints, pos, np.where(plus, 1.0, -1.0))
            if self._tree_record:
                self._native.set_tree_record(True)
            if self._primal_heuristic:
                self._native.set_heuristic(self._primal_heuristic)
            if self._local_search:
                self._native.set_local_search(self._local_search)
            if self._fix_propagate:
                self._native.set_fix_propagate(self._fix_propagate)
            if self._weighted_repair:
                self._native.set_weighted_repair(self._weighted_repair)
            if self._cube_search:
                self._native.set_cube_search(self._cube_search)
            if self._complete_continuous:
                self._native.set_completion(True)
            if self._lp_dive:
                self._native.set_lpdive(64 if self._lp_dive is True else self._lp_dive,
                                        self._lp_dive_every or 0)
            if self._objective_step:
                self._native.set_objective_step(self._objective_step)
            if self._propagate:
                self._native.set_propagation(self._propagate)
            if self._reduced_cost:
                self._native.set_reduced_cost(True)
        st = None
        if self._comm is not None and not self._sharded:
            from simple_mip_solver_amd.parallel import shard_and_attach
            ramp = shard_and_attach(self._native, self._comm, self.frontier_batch, self._exchange_every)
            self._sharded = True
            if ramp['status'] not in (0, 4) or ramp['open_nodes'] == 0:
                st = ramp      # finished inside the replicated ramp-up: every rank holds the result
                self._comm = None
        if st is None:
            st = self._native.solve(node_limit=0 if self.node_limit == INF else self.node_limit,
                                    mip_gap=self.mip_gap,
                                    max_seconds=0.0 if self.max_run_time == INF else self.max_run_time,
                                    frontier_batch=self.frontier_batch)
        if self._comm is not None:
            g = self._native.global_stats()
            st = dict(st, evaluated_nodes=g['evaluated_nodes'])
            self._native_global = g
        self._native_stats = st
        if self._host_spill:
            self.spill_stats = self._native.spill_stats()
        if self._cut_migration:
            self.cut_migration_stats = self._native.cut_migration_stats()
        if self._dual_function:
            self.dual_function_stats = self._native.dual_function_stats()
            if self.dual_function_stats['dropped']:
                import warnings
                warnings.warn('the dual function store is full (%d bytes in use): %d nodes have no dual term; their '
                              'leaves use their ancestors\' terms (a valid, weaker bound); pass a larger dual_function'
                              % (self.dual_function_stats['bytes'], self.dual_function_stats['dropped']), RuntimeWarning)
        if st['pool_exhausted']:
            import warnings
            if self._host_spill:
                warnings.warn('the GPU node pool and the host spill store are full (pool_capacity=%d, host_spill=%d '
                              'bytes): the search stopped with the bounds found so far; pass a larger host_spill'
                              % (self._pool_capacity, self._host_spill), RuntimeWarning)
            else:
                warnings.warn('the GPU node pool is full (pool_capacity=%d): the search stopped with the bounds '
                              'found so far; pass a larger pool_capacity' % self._pool_capacity, RuntimeWarning)
        self.solve_time = st['solve_seconds']
        self.evaluated_nodes = st['evaluated_nodes']
        self.primal_bound = st['primal_bound']
        self.status = _ffi.TREE_STATUS[st['status']]
        self._unbounded = True if st['status'] == 3 else self._unbounded
        self._best_solution = self._native.solution() if st['has_solution'] else None
        self.solution = self._best_solution
        self.objective_value = self.primal_bound
        self._kwargs['next_node_idx'] = st['created_nodes']
        if issubclass(self._Node, PseudoCostBranchNode):
            self._kwargs['pseudo_costs'] = self._native.pseudo_costs()
        if self._tree_record:   # `tree` on the engine's records, the nodes already handed out brought up to date
            from simple_mip_solver_amd.algorithms.recorded_tree import RecordedTree
            if not isinstance(self.tree, RecordedTree):
                self.tree = RecordedTree(self)
            self.tree.refresh()
            self.tree_record_stats = self._native.tree_record_stats()
        if self.restart_stats is not None:
            self.restart_stats = self._native.restart_stats()
        if self._primal_heuristic:
            self.heuristic_stats = self._native.heuristic_stats()
        if self._propagate:
            self.propagation_stats = self._native.propagation_stats()
        if self._reduced_cost:
            self.reduced_cost_stats = self._native.reduced_cost_stats()
        if self._objective_step:
            self.objective_step_stats = self._native.objective_step_stats()
        if self._local_search:
            self.local_search_stats = self._native.local_search_stats()
        if self._fix_propagate:
            self.fix_propagate_stats = self._native.fix_propagate_stats()
        if self._weighted_repair:
            self.weighted_repair_stats = self._native.weighted_repair_stats()
        if self._cube_search:
            self.cube_search_stats = self._native.cube_search_stats()
        if self._complete_continuous:
            self.completion_stats = self._native.completion_stats()
        if self._lp_dive:
            self.lp_dive_stats = self._native.lpdive_stats()
        if self._native.cuts:   # the running GMIC totals bound() threads through the kwargs
            totals = self._native.cut_stats()
            self._native_cuts_dropped = totals.pop('dropped')
            for key, value in totals.items():
                self._kwargs[key] = self._native_totals0.get(key, 0) + value

    _restart_overrides = ('node_limit', 'mip_gap', 'max_run_time', 'frontier_batch', 'anchor', 'dive', 'primal_heuristic',
                          'local_search', 'fix_propagate', 'weighted_repair', 'cube_search', 'complete_continuous', 'lp_dive',
                          'lp_dive_every')

    def restart(self, b, **overrides):
        """A new, unsolved BranchAndBound for the same A, c, bounds and integer indices at the right-hand side
        b, whose native search starts from the leaves of this one (include/mipx_restart.h): this search's records
        are its skeleton, every childless node an open node with its bounds rebuilt on the GPU, warm-started
        from the root's basis; the pseudo-cost table is carried over.  The childless nodes partition the integer
        points of the root box at every b, so the restarted search is exact.  b follows the convention of
        find_parameterized_dual_bound (a CyLPArray of the constraint's shape, negated with the same warning if
        the constraints were flipped at instantiation).  Same Node class and keyword options; overrides may
        change node_limit, mip_gap, max_run_time, frontier_batch (at most this search's), anchor, dive,
        primal_heuristic, local_search, fix_propagate, weighted_repair, cube_search, complete_continuous and lp_dive
        with lp_dive_every (all but the first run on the heuristic's points: an override that turns primal_heuristic
        off turns the inherited ones off with it).
        Needs frontier_batch and tree_record=True and a solve() before; not with comm; the restarted search
        records no dual function.  `restart_stats` of the new search reports the seeding."""
        assert self.frontier_batch is not None and self._tree_record, \
            'restart needs a search run with frontier_batch and tree_record=True'
        assert self.status != 'unsolved', 'must solve this instance before using this method'
        assert self._comm is None and 'comm' not in overrides, 'restart cannot be combined with comm'
        assert not overrides.get('dual_function'), \
            'dual_function is not available for a restarted search: the dual function keeps its own tree'
        unknown = set(overrides) - set(self._restart_overrides) - {'dual_function'}
        assert not unknown, f'restart overrides are {self._restart_overrides}, not {sorted(unknown)}'
        assert isinstance(b, CyLPArray), 'this function only works with CyLP arrays'
        lp = self.root_node.lp
        assert len(lp.constraints) == 1 and b.shape == lp.constraints[0].lower.shape, \
            'the shape of the RHS being added should match that of each node'
        opts = dict(self._given)
        opts.update({k: v for k, v in overrides.items() if k != 'dual_function'})
        if not opts.get('primal_heuristic') and 'local_search' not in overrides:
            opts['local_search'] = None   # (the local search runs on the heuristic's points: it leaves with it)
        if not opts.get('primal_heuristic') and 'fix_propagate' not in overrides:
            opts['fix_propagate'] = None   # (and so does the dive)
        if not opts.get('primal_heuristic') and 'weighted_repair' not in overrides:
            opts['weighted_repair'] = None   # (and the weighted repair)
        if not opts.get('primal_heuristic') and 'cube_search' not in overrides:
            opts['cube_search'] = None   # (and the cube search)
        if not opts.get('primal_heuristic') and 'complete_continuous' not in overrides:
            opts['complete_continuous'] = None   # (and the completion)
        if not opts.get('primal_heuristic') and 'lp_dive' not in overrides:
            opts['lp_dive'] = None   # (and the LP dive)
        if not opts.get('lp_dive') and 'lp_dive_every' not in overrides:
            opts['lp_dive_every'] = None
        assert isinstance(opts['frontier_batch'], int) and 0 < opts['frontier_batch'] <= self.frontier_batch, \
            'a restarted search steps with at most the frontier_batch of its source'
        if self._swapped_constraint_direction:
            b = -b
            print('WARNING: your rhs was made negative to reflect constraints'
                  ' flipping direction at instantiation')
        from simple_mip_solver_amd.milp_instance import MILPInstance
        m = self.model   # (already min c'x, A x >= b: base_algorithm._convert_constraints_to_greq)
        model = MILPInstance(A=np.asarray(m.A), b=np.asarray(b, dtype=np.float64), c=m.lp.objective, l=m.l, u=m.u,
                             integerIndices=m.integerIndices, sense=['Min', '>='], numVars=m.numVars)
        kwargs = dict(self._given_kwargs)
        if 'pseudo_costs' in kwargs:
            kwargs['pseudo_costs'] = {}   # (the engine carries its table over)
        new = BranchAndBound(model, self._Node, **opts, **kwargs)
        new._swapped_constraint_direction = self._swapped_constraint_direction   # (b of a further restart: as here)
        new._seed_native(self)
        return new

    def _seed_native(self, source):
        """The native tree of a restarted search: made from the source's, not from the root."""
        from simple_mip_solver_amd import _ffi
        from simple_mip_solver_amd.lp import get_backend, HipBackend
        backend = get_backend()
        assert isinstance(backend, HipBackend), 'frontier_batch needs the HIP backend'
        rs = self.root_node.lp._engine_form()
        problem = backend._problem(rs.A, rs.b, rs.c, rs.key)
        self._native_totals0 = {k: self._kwargs.get(k, 0) for k in _ffi.CUT_TOTAL_KEYS}
        self._native = _ffi.Tree.restart(source._native, problem)
        if self._anchor:
            self._native.set_anchor_mode(True)
        if self._dive:
            self._native.set_dive(self._dive)
        if self._host_spill:
            self._native.set_host_spill(self._host_spill)
        if self._primal_heuristic:
            self._native.set_heuristic(self._primal_heuristic)
        if self._local_search:
            self._native.set_local_search(self._local_search)
        if self._fix_propagate:
            self._native.set_fix_propagate(self._fix_propagate)
        if self._weighted_repair:
            self._native.set_weighted_repair(self._weighted_repair)
        if self._cube_search:
            self._native.set_cube_search(self._cube_search)
        if self._complete_continuous:
            self._native.set_completion(True)
        if self._lp_dive:
            self._native.set_lpdive(64 if self._lp_dive is True else self._lp_dive,
                                    self._lp_dive_every or 0)
        self.restart_stats = self._native.restart_stats()
        self._kwargs['next_node_idx'] = source._kwargs['next_node_idx']

    def _evaluate_node(self, node):
        """Bound the node unless its inherited bound already prunes it; record an incumbent or
        branch (reference :243-266)."""
        if not node.dual_bound < self.primal_bound:
            return
        self.evaluated_nodes += 1
        self._process_bound_rtn(node.bound(**self._kwargs))
        self._leaf_bounds.push(node)  # the node now carries its own LP objective

        # like the reference, an unbounded relaxation is taken to mean an unbounded MILP
        if node.unbounded:
            self._unbounded = True

        if node.lp_feasible and node.objective_value < self.primal_bound:
            if node.mip_feasible:
                self._best_solution = node.solution
                self.primal_bound = node.objective_value
            else:
                self._process_branch_rtn(node.idx, node.branch(**self._kwargs))

    def _stopping(self, start):
        """The test of solve()'s loop, less the empty queue."""
        return bool(self._unbounded or self.evaluated_nodes >= self.node_limit or self._gap_closed() or
                    time.perf_counter() - start > self.max_run_time)

    def _evaluate_batch(self, start):
        """One lp_batch step: take up to lp_batch nodes off the queue, solve their first LPs ahead in
        one launch per row set, then evaluate them one by one as solve()'s loop would have."""
        popped, live = [], 0
        while len(popped) < self.lp_batch and not self._node_queue.empty():
            if popped and (self.evaluated_nodes + live >= self.node_limit or
                           time.perf_counter() - start > self.max_run_time):
                break
            node = self._node_queue.get()
            popped.append(node)
            live += node.dual_bound < self.primal_bound
        ahead = self._prefetch(popped)
        try:
            for i, node in enumerate(popped):
                if i and self._stopping(start):
                    # where the per-node loop stops: the rest go back to the queue, unsolved
                    for rest in reversed(popped[i:]):
                        self._drop_prefetch(rest, ahead)
                        self._node_queue.put(rest)
                    break
                self._pending = popped[i + 1:]
                self._evaluate_node(node)
                self._drop_prefetch(node, ahead)
        finally:
            self._pending = []

    def _drop_prefetch(self, node, ahead):
        """Count a result solved ahead for node that dual() never took, and detach it."""
        pre = ahead.pop(id(node), None)
        if pre is not None and not pre.used:
            pre.used = True
            self.lp_batch_stats['wasted'] += 1
            if getattr(node.lp, '_prefetched', None) is pre:
                node.lp._prefetched = None

    def _prefetch(self, popped):
        """Solve the first LP of every popped node its inherited bound does not prune, one
        backend.solve per (row set, iteration limit, cold / warm) group, and attach each result to the
        node's LP as a Prefetch (with the engine's integrality scan when the backend has one).
        Returns {id(node): Prefetch}."""
        from simple_mip_solver_amd.lp import Prefetch, get_backend
        from simple_mip_solver_amd.utils import tolerance as tol
        groups, ahead = {}, {}
        for node in popped:
            lp = getattr(node, 'lp', None)
            if not node.dual_bound < self.primal_bound or not isinstance(lp, DenseLP) or \
                    (lp._solved_sig is not None and lp._status == 0):
                continue   # pruned on arrival, not an engine LP, or dual() would keep its solution
            rs = lp._engine_form()
            l, u = lp._bounds()
            if not np.all(np.isfinite(l)):
                continue   # free columns: DenseLP._dual_with_free_columns, per node
            max_iter = int(lp.maxNumIteration) if lp.maxNumIteration else 0
            warm = lp._warm_start(rs)
            groups.setdefault((rs.key, max_iter, warm is None), []).append((node, rs, l, u, warm))
        if not groups:
            return ahead
        backend = get_backend()
        stats = self.lp_batch_stats
        for (key, max_iter, cold), group in groups.items():
            rs = group[0][1]
            vstat = None if cold else np.concatenate([g[4] for g in group])
            res = backend.solve(rs.A, rs.b, rs.c, np.stack([g[2] for g in group]),
                                np.stack([g[3] for g in group]), vstat, max_iter, key)
            stats['launches'] += 1
            stats['prefetched'] += len(group)
            ints = group[0][0]._integer_indices
            # K4's tolerance is the compiled-in variable_epsilon
            scan = backend.branch_score(ints, res['x'], res['status']) \
                if tol.variable_epsilon == 1e-4 else None
            for k, (node, _, l, u, warm) in enumerate(group):
                score = None
                if scan is not None and (node._integer_indices is ints or
                                         list(node._integer_indices) == list(ints)):
                    j = int(scan['branch_idx'][k])
                    score = (j if j >= 0 else None, bool(scan['mip_feasible'][k]))
                pre = Prefetch(res, k, key, max_iter, None if warm is None else warm, l, u, score, stats)
                node.lp._prefetched = pre
                ahead[id(node)] = pre
        return ahead

    def _process_branch_rtn(self, parent_id, rtn):
        """Queue the two children ('left' = down, 'right' = up), hang them in the tree, merge the
        remaining keys into the kwargs (reference :268-289)."""
        assert isinstance(rtn, dict), 'rtn must be a dictionary'
        assert isinstance(parent_id, int), 'parent_id must be integer'
        assert parent_id in self.tree, 'parent must already exist in tree'
        for direction in ['left', 'right']:
            assert direction in rtn, f'{direction} must be in the returned dict'
            child = rtn.pop(direction)
            assert isinstance(child, self._Node), \
                f'{direction} value must be type {type(self._Node)}'
            assert child.idx not in self.tree, 'please give unique node ID'
            self._node_queue.put(child)
            getattr(self.tree, f'add_{direction}_child')(child.idx, parent_id, node=child)
            self._leaf_bounds.push(child)
        self._process_rtn(rtn)

    def _process_bound_rtn(self, rtn):
        """Share returned 'cuts' with every queued node's cut pool, merge the rest into the
        kwargs (reference :291-306)."""
        assert isinstance(rtn, dict), 'rtn must be a dictionary'
        cuts = rtn.get('cuts')
        if cuts:
            for name, (pi, pi0) in cuts.items():
                for queued in self._node_queue.queue:
                    queued.cut_pool[name] = (pi, pi0)
                for pending in self._pending:   # taken off the queue by this lp_batch step, not yet evaluated
                    pending.cut_pool[name] = (pi, pi0)
            del rtn['cuts']
        self._process_rtn(rtn)

    def find_parameterized_dual_bound(self, b):
        """Lower bound on the optimal value of the MILP at a new right-hand side b, from the dual
        solutions stored along every leaf's lineage (reference :314-360): per leaf the best of
        `y.b + max(d, 0).l + min(d, 0).u` over its solved ancestors and itself, then the worst
        leaf.  Infeasible leaves are first re-solved with penalised slacks so that they carry a
        finite dual solution (`_bound_parameterized_dual`).  Nodes that were never solved (pruned
        by their inherited bound) contribute through their ancestors only.  With frontier_batch the
        engine must have recorded the terms (dual_function=True or a byte cap; include/mipx_dualfn.h):
        the same function, evaluated on the GPU from the records, the infeasible leaves re-solved once in
        one batched launch."""
        assert isinstance(b, CyLPArray), 'this function only works with CyLP arrays'
        assert self.status != 'unsolved', 'must solve this instance before using this method'
        if self.frontier_batch is not None and self._dual_function:
            return float(self._native_dual_bounds([b])[0])
        assert self.frontier_batch is None, \
            'the native frontier engine keeps no per-node duals; solve with frontier_batch=None'
        terminal_nodes = self.tree.get_leaves(self.root_node.idx)
        multi_const_nodes = [n.idx for n in terminal_nodes if len(n.lp.constraints) != 1]
        assert not multi_const_nodes, \
            f'This feature expects the root node to have a single constraint object and ' \
            f'all nodes to branch by bounding variables instead of by adding constraints. ' \
            f'It does not currently handle cuts being added after bounding. The following ' \
            f'IDs belong to nodes that do not conform to these rules: {multi_const_nodes}'
        assert all(b.shape == n.lp.constraints[0].lower.shape for n in terminal_nodes), \
            'the shape of the RHS being added should match that of each node'
        if self._swapped_constraint_direction:
            b = -b
            print('WARNING: your rhs was made negative to reflect constraints'
                  ' flipping direction at instantiation')
        for n in terminal_nodes:
            if n.lp._status == 1:  # primal infeasible: bound its dual ray (once)
                n.lp = self._bound_parameterized_dual(n.lp)
        assert all(n.lp._status in [None, 0] for n in terminal_nodes)

        def evaluate(lp):
            d = np.concatenate(list(lp.dualVariableSolution.values()))
            return float(np.inner(lp.dualConstraintSolution[lp.constraints[0].name], b) +
                         np.inner(np.maximum(d, 0), lp.variablesLower) +
                         np.inner(np.minimum(d, 0), lp.variablesUpper))

        bounds = {}
        for leaf in terminal_nodes:
            solved = [n.lp for n in self.tree.get_node_instances(leaf.lineage) if n.lp._status == 0]
            bounds[leaf.idx] = max(evaluate(lp) for lp in solved)
        return min(bounds.values())

    def find_parameterized_dual_bounds(self, B):
        """find_parameterized_dual_bound for each of K right-hand sides (a K x m array or a sequence of
        CyLP arrays): one GPU call with dual_function, a loop over the single call otherwise."""
        rows = [r if isinstance(r, CyLPArray) else CyLPArray(np.asarray(r, dtype=np.float64)) for r in B]
        if self.frontier_batch is not None and self._dual_function:
            assert self.status != 'unsolved', 'must solve this instance before using this method'
            return self._native_dual_bounds(rows)
        return np.array([self.find_parameterized_dual_bound(r) for r in rows], dtype=np.float64)

    def _native_dual_bounds(self, rows):
        """The dual function on the engine's records (mipx_tree_dual_function): the same checks as the
        Python path, b mapped to the engine rows as DenseLP._store maps the duals (w_e = sign_e b[pos_e])."""
        lp = self.root_node.lp
        assert len(lp.constraints) == 1, \
            f'This feature expects the root node to have a single constraint object and ' \
            f'all nodes to branch by bounding variables instead of by adding constraints. ' \
            f'It does not currently handle cuts being added after bounding. The following ' \
            f'IDs belong to nodes that do not conform to these rules: {[self.root_node.idx]}'
        for b in rows:
            assert isinstance(b, CyLPArray), 'this function only works with CyLP arrays'
            assert b.shape == lp.constraints[0].lower.shape, \
                'the shape of the RHS being added should match that of each node'
        W = np.array([np.asarray(b, dtype=np.float64) for b in rows], dtype=np.float64).reshape(len(rows), -1)
        if self._swapped_constraint_direction:
            W = -W
            print('WARNING: your rhs was made negative to reflect constraints'
                  ' flipping direction at instantiation')
        pos, plus = lp._row_index()
        We = np.where(plus, 1.0, -1.0)[None, :] * W[:, pos]
        out = self._native.dual_function(We, float(self._M))
        self.dual_function_stats = self._native.dual_function_stats()
        return out

    def _bound_parameterized_dual(self, cur_lp):
        """The same LP with a slack block `s_i >= 0` on every constraint block i, priced at a
        large M: its dual is the original dual with the multipliers capped at M, so a node with
        an infeasible relaxation gets a finite (very large) dual solution to evaluate at other
        right-hand sides (reference :362-417).  Solved before it is returned."""
        assert isinstance(cur_lp, DenseLP), 'must give CyClpSimplex instance'
        for i, constr in enumerate(cur_lp.constraints):
            assert f's_{i}' not in [v.name for v in cur_lp.variables], \
                f"variable 's_{i}' is a reserved name. please name your variable something else"
        new_lp = DenseLP()
        var_map = {v: new_lp.addVariable(v.name, v.dim) for v in cur_lp.variables}
        n0 = cur_lp.nVariables
        new_lp.variablesLower[:n0] = cur_lp.variablesLower
        new_lp.variablesUpper[:n0] = cur_lp.variablesUpper
        slacks = [new_lp.addVariable(f's_{i}', constr.rows) for i, constr in enumerate(cur_lp.constraints)]
        for constr, s_i in zip(cur_lp.constraints, slacks):
            extra = {var_map[v]: a for v, a in constr.varCoefs.items() if v is not constr.variables[0]}
            extra[s_i] = np.identity(constr.rows)
            new_lp.addConstraint(Constraint(var_map[constr.variables[0]], constr._coefs, constr.lower,
                                            constr.upper, constr.name, extra))
        new_lp.objective = np.concatenate([cur_lp.objective, np.full(new_lp.nVariables - n0, float(self._M))])
        var_status, row_status = cur_lp.getBasisStatus()
        # every s_i enters at its lower bound of 0 (status 3)
        new_lp.setBasisStatus(np.concatenate([var_status, np.full(new_lp.nVariables - n0, 3)]), row_status)
        new_lp.dual()
        return new_lp
