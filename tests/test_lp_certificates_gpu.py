"""What the HIP library returns through _ffi, under the independent checker of
tests/support/lp_certificate.py: optimality certificates, dual bounds of truncated solves and exact Farkas
certificates for K1 (register tiles), K1b (HBM-streamed), K1c (one LP over the chip), the multi-problem
launch, LPs with cut rows, plunge levels and the engine's dual records.

Independent of the CPU oracle on purpose: nothing here calls it.  Instances come from the generators and
tests/golden/.  Asserted: the contract tolerances; printed (-s): the worst residual of each family.
"""
import numpy as np
import pytest

from simple_mip_solver_amd import _ffi
from simple_mip_solver_amd.generators import random_dense_milp_arrays
from tests.support import harvest as H
from tests.support import lp_certificate as C
from tests.test_lp_certificates import (certify, certify_dive_levels, children, mixed_instance, raised_children)

pytestmark = pytest.mark.gpu
INF = np.inf

KERNELS = {'lp_dual_simplex<1,8,4>', 'lp_dual_simplex<3,6,8>', 'lp_dual_simplex<7,5,16>', 'lp_dual_simplex<7,7,16>',
           'lp_dual_simplex_big'}
TILE_SHAPES = [(1, 1), (2, 1), (5, 0), (3, 40), (63, 31), (64, 32), (65, 33), (40, 33), (128, 64), (129, 64), (100, 65),
               (255, 127), (256, 128), (256, 129), (200, 192), (256, 193), (257, 100)]
BOXED_SHAPES = [(64, 32, 0), (128, 64, 1), (256, 128, 0), (200, 150, 3), (300, 150, 0), (512, 256, 1)]


def test_every_kernel(gpu_ctx, monkeypatch):
    """Problem.solve_batch for every kernel name _ffi.kernel_name can return: boxed roots, children, children
    whose raised bounds close the box, probes; the tile-boundary shapes with fixed variables, infinite bounds
    and an empty row; and K1c (a single cold LP above the register tiles) with MIPX_ROOT_WG 32 / 256."""
    names = set()
    for m in list(range(1, 200, 7)) + [256, 300, 512, 1000]:
        for n in (1, 8, 64, 65, 128, 129, 256, 257, 512, 1024):
            try:
                names.add(_ffi.kernel_name(m, n))
            except _ffi.MipxError:
                pass
    assert names == KERNELS
    covered = set()
    rep = C.Report('gpu solve_batch, boxed')
    for n, m, seed in BOXED_SHAPES:
        A, b, c, l, u, _ = random_dense_milp_arrays(n, m, seed=seed)
        covered.add(_ffi.kernel_name(m, n))
        p = _ffi.Problem(gpu_ctx, A, b, c)
        root = p.solve_batch(l[None], u[None])                      # (above the tiles: K1c)
        assert root['status'][0] == 0
        certify(A, b, c, l[None], u[None], root, rep, f'{n}x{m} root')
        L, U, V = children(l, u, root, 8 if n <= 256 else 3)
        if n <= 256:
            L3, U3, V3 = raised_children(l, u, root, range(2, 34, 4), seed)
            L, U, V = np.vstack([L, L3]), np.vstack([U, U3]), np.vstack([V, V3])
        full = p.solve_batch(L, U, V)
        certify(A, b, c, L, U, full, rep, f'{n}x{m} children')
        for max_iter in (1, 5, 33):
            certify(A, b, c, L, U, p.solve_batch(L, U, V, max_iter=max_iter), rep, f'{n}x{m} max_iter {max_iter}',
                    optimum=full['obj'])
        if n > 256:
            for wg in ('32', '256'):
                monkeypatch.setenv('MIPX_ROOT_WG', wg)
                q = _ffi.Problem(gpu_ctx, A, b, c)
                certify(A, b, c, l[None], u[None], q.solve_batch(l[None], u[None]), rep, f'{n}x{m} K1c, {wg} workgroups')
                certify(A, b, c, l[None], u[None], q.solve_batch(l[None], u[None], max_iter=33), rep,
                        f'{n}x{m} K1c, {wg} workgroups, 33 pivots', optimum=root['obj'])
                q.close()
            monkeypatch.delenv('MIPX_ROOT_WG')
        p.close()
    print(rep)
    assert rep.count[1] >= 8 and rep.farkas_verified == rep.count[1] and rep.count[3] >= 8 and rep.status3_vacuous == 0
    rep = C.Report('gpu solve_batch, tile boundaries (mixed)')
    for n, m in TILE_SHAPES:
        A, b, c, l, u = mixed_instance(n, m, seed=n + m)
        covered.add(_ffi.kernel_name(m, n))
        p = _ffi.Problem(gpu_ctx, A, b, c)
        root = p.solve_batch(l[None], u[None])
        certify(A, b, c, l[None], u[None], root, rep, f'{n}x{m} root', boxed=False)
        if root['status'][0] == 0:
            L, U, V = children(l, u, {'x': np.minimum(root['x'], 1e6), 'vstat': root['vstat']}, 4)
            if len(L):
                full = p.solve_batch(L, U, V)
                certify(A, b, c, L, U, full, rep, f'{n}x{m} children', boxed=False)
                certify(A, b, c, L, U, p.solve_batch(L, U, V, max_iter=3), rep, f'{n}x{m} probes', boxed=False,
                        optimum=full['obj'])
        if m > 2:
            A2, b2 = A.copy(), b.copy()
            A2[1] = -1.0; b2[1] = 1.0
            p2 = _ffi.Problem(gpu_ctx, A2, b2, c)
            bad = p2.solve_batch(np.zeros((1, n)), u[None])
            assert bad['status'][0] == 1
            certify(A2, b2, c, np.zeros((1, n)), u[None], bad, rep, f'{n}x{m} infeasible', boxed=False)
            p2.close()
        p.close()
    print(rep)
    assert rep.farkas_verified >= len([1 for n, m in TILE_SHAPES if m > 2])
    assert covered == KERNELS


def test_c2_batch_of_1024_roots_all_certified(gpu_ctx):
    """solve_multi on the 1 024 C2 roots: every one certified.  The entry reports no duals, so y is derived
    from each reported basis in f64 (B^T y = c_B) and judged by the certificate like a reported one."""
    probs = [random_dense_milp_arrays(64, 32, seed=s) for s in range(1024)]
    A = np.stack([p[0] for p in probs]); b = np.stack([p[1] for p in probs]); c = np.stack([p[2] for p in probs])
    l = np.stack([p[3] for p in probs]); u = np.stack([p[4] for p in probs])
    g = _ffi.solve_multi(gpu_ctx, A, b, c, l, u)
    assert np.all(g['status'] == 0)
    rep = C.Report('gpu solve_multi, 1024 roots')
    for k in range(1024):
        one = {key: val[k:k + 1] for key, val in g.items()}
        one['y'] = C.duals_from_basis(A[k], c[k], g['vstat'][k])[None]
        C.certify_batch(A[k], b[k], c[k], l[k][None], u[k][None], one, rep, f'instance {k}')
    print(rep)
    assert rep.count[0] == 1024


def test_bench_shaped_plunge_batch(gpu_ctx):
    """256 x 128 seed 0: the children and grandchildren of the root, a few thousand node LPs in one anchored
    launch, dive_batch(depth=8): the nodes and every level of every chain certified as the LP with the
    accumulated bounds, in vectorised longdouble."""
    n, m = 256, 128
    A, b, c, l, u, ints = random_dense_milp_arrays(n, m, seed=0)
    p = _ffi.Problem(gpu_ctx, A, b, c)
    root = p.solve_batch(l[None], u[None])
    p.set_anchor(root['vstat'][0])
    L1, U1, V1 = children(l, u, root, 24)
    kids = p.solve_batch(L1, U1, V1)
    Ls, Us, Vs = [L1], [U1], [V1]
    for k in np.flatnonzero(kids['status'] == 0):
        L2, U2, V2 = children(L1[k], U1[k], {key: val[k:k + 1] for key, val in kids.items()}, 24)
        Ls.append(L2); Us.append(U2); Vs.append(V2)
    L, U, V = np.vstack(Ls), np.vstack(Us), np.vstack(Vs)
    assert len(L) >= 2000
    rng = np.random.default_rng(0)
    cost_l, cost_r = rng.uniform(0.5, 4.0, n), rng.uniform(0.5, 4.0, n)
    res = p.dive_batch(L, U, V, 1, ints, cost_l, cost_r, np.ones(n, np.uint8), depth=8)
    rep = C.Report(f'gpu plunge, {len(L)} nodes x depth 8')
    certify_dive_levels(A, b, c, L, U, res, 8, rep, 'plunge')
    print(rep)
    assert rep.count[0] >= 2 * len(L) and np.any(res['status'][8 * len(L):] >= 0)
    p.close()


@pytest.mark.parametrize('n,m,seed', [(64, 32, 1), (256, 128, 0), (300, 150, 0)])
def test_lps_with_cut_rows(n, m, seed, gpu_ctx):
    """Problem.solve_batch_cuts: each node certified as the LP vstack(A, its cut rows); the cuts are the
    root's Gomory cuts from the cut kernel, raw and rounded."""
    A, b, c, l, u, ints = random_dense_milp_arrays(n, m, seed=seed)
    p = _ffi.Problem(gpu_ctx, A, b, c)
    root = p.solve_batch(l[None], u[None])
    g = p.gomory_batch(l[None], u[None], root['vstat'], root['x'], ints)[0]
    store_pi = np.vstack([g['pi'], g['safe_pi']]); store_pi0 = np.concatenate([g['pi0'], g['safe_pi0']])
    K = len(store_pi0)
    assert K >= 4
    kc = 64 if n > 256 else (min(64, 192 - m) if m + 64 > 128 else 64)
    rng = np.random.default_rng(seed)
    sizes = [0, 1, 2, min(5, K), min(kc, K), min(kc // 2, K), 0, 3]
    lists = [sorted(rng.choice(K, size=s, replace=False).tolist()) if s else [] for s in sizes]
    B = len(lists)
    L = np.repeat(l[None], B, axis=0); U = np.repeat(u[None], B, axis=0)
    x = root['x'][0]
    j = int(np.argmax(np.minimum(x - np.floor(x), np.ceil(x) - x)))
    U[1::2, j] = np.floor(x[j])
    V = [np.concatenate([root['vstat'][0], np.ones(len(ids), np.int8)]) for ids in lists]
    rep = C.Report(f'gpu cut rows {n}x{m}')
    full = p.solve_batch_cuts(L, U, V, store_pi, store_pi0, lists, kc=kc)
    runs = [('warm', full, None), ('cold', p.solve_batch_cuts(L, U, None, store_pi, store_pi0, lists, kc=kc), None),
            ('probe', p.solve_batch_cuts(L, U, V, store_pi, store_pi0, lists, max_iter=5, kc=kc), full['obj'])]
    for what, got, optimum in runs:
        for k, ids in enumerate(lists):
            Ak = np.vstack([A, store_pi[ids]]) if ids else A
            bk = np.concatenate([b, store_pi0[ids]]) if ids else b
            one = dict(status=got['status'][k:k + 1], obj=got['obj'][k:k + 1], x=got['x'][k:k + 1],
                       y=got['y'][k][None], vstat=got['vstat'][k][None])
            certify(Ak, bk, c, L[k:k + 1], U[k:k + 1], one, rep, f'{what} node {k} ({len(ids)} cuts)',
                    optimum=None if optimum is None else optimum[k:k + 1])
    print(rep)
    assert rep.count[0] >= 2 * B
    p.close()


def test_harvested_search_nodes(gpu_ctx):
    """The node LPs and probes of real searches (tests/golden/harvested_nodes.npz, kept equal to a fresh
    harvest by tests/test_lp_certificates.py): the marginally infeasible leaves get their exact certificate
    from what the kernels report."""
    rep = C.Report('gpu harvested searches')
    for name, rs in sorted(H.load().items()):
        A, b, c = rs['A'], rs['b'], rs['c']
        boxed = bool(np.all(np.isfinite(rs['l'])) and np.all(np.isfinite(rs['u'])))
        p = _ffi.Problem(gpu_ctx, A, b, c)
        for rows, max_iter, V in H.groups(rs):
            L, U = rs['l'][rows], rs['u'][rows]
            res = p.solve_batch(L, U, V, max_iter=max_iter)
            optimum = p.solve_batch(L, U, V)['obj'] if max_iter else None
            certify(A, b, c, L, U, res, rep, f'{name} max_iter {max_iter}', boxed=boxed, optimum=optimum)
        p.close()
    print(rep)
    assert rep.count[1] >= 8 and rep.farkas_verified >= 8 and rep.count[3] >= 1


def test_engine_dual_records(gpu_ctx):
    """The frontier engine's dual records in the configuration of test_determinism_and_traced_records
    (B = 64, anchor, dive 4).  Every status-0 record has y >= 0.  The trace names nodes and branching
    variables, not bounds, so the node whose bounds are known is the root (parent -1): there
    t == sum(max(d, 0) l + min(d, 0) u) to the tolerance of test_dual_function_gpu.py::check_parity, and
    b.y + t is the root optimum.  For every other record the root box gives what weak duality alone
    says: the term over the root box is at most the recorded one (the node's box lies inside it), and
    b.y plus it is a lower bound of the root LP."""
    A, b, c, l, u, ints = random_dense_milp_arrays(60, 30, seed=2)
    p = _ffi.Problem(gpu_ctx, A, b, c)
    t = _ffi.Tree(p, ints, l, u, branch_rule='pseudo cost', max_batch=64, pool_capacity=1 << 16)
    t.set_anchor_mode(True)
    t.set_dive(4)
    t.set_dual_record(1 << 30, 30, np.arange(30), np.ones(30))
    t.set_trace(True)
    t.solve(mip_gap=0.0, frontier_batch=64, max_steps=12)
    recs = t.dual_records()
    own = np.flatnonzero(recs['status'] == 0)
    assert len(own) >= 64
    assert np.all(recs['y'][own] >= 0.0)
    roots = [r for r in own if recs['parent'][r] == -1]
    assert len(roots) == 1
    root = p.solve_batch(l[None], u[None])
    for r in roots:
        d = c - A.T @ recs['y'][r]
        terms = np.maximum(d, 0) * l + np.minimum(d, 0) * u
        assert abs(recs['t'][r] - terms.sum()) <= 1e-12 * max(1.0, np.abs(terms).sum())
        assert abs(b @ recs['y'][r] + recs['t'][r] - root['obj'][0]) <= 1e-9 * max(1.0, abs(root['obj'][0]))
    # a record's term is computed with the node's own (tighter) bounds: with the root's box it can only be
    # lower, and b.y + (that) is a valid bound of the root LP -- below the root optimum
    D = c[None] - recs['y'][own] @ A
    t_root_box = (np.maximum(D, 0) * l + np.minimum(D, 0) * u).sum(axis=1)
    slack = 4 * 90 * C.EPS * (np.abs(recs['y'][own]) @ np.abs(b) + (np.abs(D) * u).sum(axis=1))
    assert np.all(t_root_box <= recs['t'][own] + slack)
    assert np.all(recs['y'][own] @ b + t_root_box <= root['obj'][0] + slack)
    t.close()
    p.close()
