"""pytorch3d's knn_points on the GPU (gsr_knn.hip through autovfx_amd.knn.knn_points): bit for bit the contract of autovfx_amd/knn.py --
against the numpy restatement at every size and slot count at which the tree or the kernel changes shape, on ties and non-finite
points, against a brute force in eager torch ops on large clouds; the gradients against float64 autograd; and the plumbing a caller
relies on.  Every GPU result is read after ``torch.cuda.synchronize()``, which raises if a kernel faulted: a fault fails the test
that caused it."""
from __future__ import annotations

import ctypes
import functools
import sys
import types

import numpy as np
import pytest
import torch

from autovfx_amd import hook, scenes
from autovfx_amd.knn import FLT_MAX, knn_points, knn_points_host

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
SIZES = ["K", "K+1", 63, 64, 65, 1024, 1025, 16385]     # the leaf, first-level and second-level boundaries of a 64 x 16 x 16 tree
KS = [1, 3, 4, 5, 8, 9, 16]                              # the slot counts 4, 8, 16: full, one short, one over


def _points(kind: str, P: int, seed: int = 0) -> np.ndarray:
    """The six distributions of tests/test_knn_gpu.py."""
    g = np.random.default_rng(seed)
    if kind == "cube":
        pts = g.uniform(-1, 1, (P, 3))
    elif kind == "clusters":   # Gaussian blobs and a few far outliers that stretch the bounds, as in a COLMAP cloud
        k = max(1, P // 5000)
        centres = g.uniform(-5, 5, (k, 3))
        pts = centres[g.integers(0, k, P)] + g.normal(0, 0.05, (P, 3))
        n_out = max(1, P // 10000)
        pts[g.choice(P, n_out, replace=False)] = g.uniform(-1, 1, (n_out, 3)) * 1e4
    elif kind == "plane":
        pts = np.c_[g.uniform(-1, 1, (P, 2)), np.full(P, 0.5)]
    elif kind == "line":
        pts = np.c_[g.uniform(-1, 1, P), np.full(P, -0.25), np.full(P, 2.0)]
    elif kind == "duplicates":   # a handful of distinct positions, each many times
        pts = g.uniform(-1, 1, (max(1, P // 200), 3))[g.integers(0, max(1, P // 200), P)]
    elif kind == "c3":
        pts = scenes.config_c3(P=P, seed=2).means3D.numpy()
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(pts, dtype=F)


def _around(pts: np.ndarray, P1: int, seed: int) -> np.ndarray:
    """Queries drawn around the points, as SuGaR samples around its Gaussians."""
    g = np.random.default_rng(seed)
    return np.ascontiguousarray(pts[g.integers(0, len(pts), P1)] + g.normal(0, 0.02, (P1, 3)), dtype=F)


def _run(p1, p2, K: int, **kw):
    """One batch element through knn_points; ``p2 is None``: the self query (the same tensor twice).  numpy in, numpy out."""
    t1 = torch.from_numpy(np.ascontiguousarray(p1)).to(DEV)[None]
    t2 = t1 if p2 is None else torch.from_numpy(np.ascontiguousarray(p2)).to(DEV)[None]
    out = knn_points(t1, t2, K=K, **kw)
    torch.cuda.synchronize()
    assert out.dists.shape == out.idx.shape == (1, len(p1), K)
    assert out.dists.dtype == torch.float32 and out.idx.dtype == torch.int64
    return out.dists[0].cpu().numpy(), out.idx[0].cpu().numpy()


def _same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _assert_rows(got, want, rows=None):
    (gd, gi), (wd, wi) = got, want
    if rows is not None:
        gd, gi = gd[rows], gi[rows]
    bad = np.flatnonzero((gd.view(np.uint32) != wd.view(np.uint32)).any(1) | (gi != wi).any(1))
    assert _same_bits(gd, wd) and np.array_equal(gi, wi), (bad[:10], gd[bad[:2]], wd[bad[:2]], gi[bad[:2]], wi[bad[:2]])


@functools.lru_cache(maxsize=None)
def _sized_case(P2: int):
    """A cloud of that size, 1 000 queries around it, and both restatements at min(16, P2) slots, computed once: a row of K slots is
    the first K of a row of 16, since rows are in (d, j) order.  The self query of the largest cloud is restated on a third of its
    rows and its last two leaves."""
    pts = _points("clusters" if P2 % 2 else "cube", P2, seed=P2)
    queries = _around(pts, 1000, seed=P2 + 1)
    k = min(16, P2)
    rows = np.arange(P2) if P2 <= 4096 else np.unique(np.r_[0:P2:3, P2 - 130:P2])
    return pts, queries, rows, knn_points_host(pts[rows], pts, k), knn_points_host(queries, pts, k)


def _size(size, K: int) -> int:
    return {"K": K, "K+1": K + 1}.get(size, size)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("size", SIZES)
def test_self_query_equals_the_restatement(size, K):
    pts, _queries, rows, (wd, wi), _cross = _sized_case(_size(size, K))
    _assert_rows(_run(pts, None, K), (wd[:, :K], wi[:, :K]), rows)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("size", SIZES)
def test_cross_query_equals_the_restatement(size, K):
    pts, queries, _rows, _self, (wd, wi) = _sized_case(_size(size, K))
    _assert_rows(_run(queries, pts, K), (wd[:, :K], wi[:, :K]))


@pytest.mark.parametrize("P1", [1, 63, 65, 1000])
def test_cross_query_shapes(P1):
    pts, _queries, _rows, (sd, si), _cross = _sized_case(1025)
    g = np.random.default_rng(P1)
    far = (g.uniform(-1, 1, (P1, 3)) * 3e4 + 5e4).astype(F)                      # all far outside p2's bounds, on every side of it
    far[::2] *= F(-1)
    one_cell = (pts[17] + g.uniform(-1, 1, (P1, 3)) * 1e-7).astype(F)            # all in one cell of p2's grid
    for queries in (far, one_cell, _around(pts, P1, seed=P1)):
        for K in (5, 16):
            _assert_rows(_run(queries, pts, K), knn_points_host(queries, pts, K))
    clone = pts[:P1].copy()                                                       # another buffer: the cross path, the self query's rows
    for K in (4, 16):
        _assert_rows(_run(clone, pts, K), (sd[:P1, :K], si[:P1, :K]))


@pytest.mark.parametrize("kind", ["lattice", "half_duplicates"])
def test_ties_go_by_the_lower_index(kind):
    g = np.random.default_rng(31)
    if kind == "lattice":       # 13^3 integer positions, shuffled: every distance is one of a few integers
        pts = np.stack(np.meshgrid(*[np.arange(13)] * 3, indexing="ij"), -1).reshape(-1, 3)[g.permutation(13 ** 3)].astype(F)
    else:                       # every second point is a copy of another one
        pts = _points("cube", 3000, seed=31)
        pts[1::2] = pts[g.integers(0, 1500, 1500) * 2]
    queries = pts[g.integers(0, len(pts), 500)].copy()
    for K in (3, 8, 16):
        _assert_rows(_run(pts, None, K), knn_points_host(pts, pts, K))
        _assert_rows(_run(queries, pts, K), knn_points_host(queries, pts, K))


def test_non_finite_points_and_queries():
    pts = _points("cube", 2000, seed=3)
    pts[::7] = np.nan
    pts[3::11, 1] = -np.inf
    bad = np.flatnonzero(~np.isfinite(pts).all(1))
    for K in (4, 16):
        d, i = _run(pts, None, K)
        _assert_rows((d, i), knn_points_host(pts, pts, K))
        assert not np.isin(i, bad).any()
        assert np.all(np.isposinf(d[bad])) and np.all(i[bad] == -1)
    queries = _around(_points("cube", 2000, seed=3), 300, seed=4)
    queries[::5, 2] = np.nan
    queries[1::9, 0] = np.inf
    d, i = _run(queries, pts, 16)
    _assert_rows((d, i), knn_points_host(queries, pts, 16))
    qbad = np.flatnonzero(~np.isfinite(queries).all(1))
    assert np.all(np.isposinf(d[qbad])) and np.all(i[qbad] == -1) and not np.isin(i, bad).any()
    few = _points("cube", 40, seed=5)          # fewer candidates than K: the rows end in (inf, -1)
    few[10:] = np.nan
    d, i = _run(few, None, 16)
    _assert_rows((d, i), knn_points_host(few, few, 16))
    assert np.all(i[:10, :10] >= 0) and np.all(i[:, 10:] == -1) and np.all(np.isposinf(d[:, 10:]))


def _torch_brute(p2: torch.Tensor, q: torch.Tensor, K: int, chunk: int):
    """The contract's distances in eager torch ops, one op per elementwise step: the K + 1 smallest of every row, ascending, and
    their indices (whose order among equal distances is torch's, not the contract's)."""
    inf = torch.tensor(float("inf"), dtype=torch.float32, device=p2.device)
    x, y, z = p2[:, 0], p2[:, 1], p2[:, 2]
    vals, idxs = [], []
    for a in range(0, q.shape[0], chunk):
        c = q[a:a + chunk]
        dx = x[None, :] - c[:, 0:1]
        d = dx * dx
        dy = y[None, :] - c[:, 1:2]
        d = d + dy * dy
        dz = z[None, :] - c[:, 2:3]
        d = d + dz * dz
        d = torch.where(d < FLT_MAX, d, inf)
        top = torch.topk(d, K + 1, dim=1, largest=False, sorted=True)
        vals.append(top.values.cpu().numpy())
        idxs.append(top.indices.cpu().numpy())
    return np.concatenate(vals), np.concatenate(idxs)


def _assert_against_brute(got, brute, K: int, queries: np.ndarray, pts: np.ndarray):
    """``dists`` bit-equal on every row; ``idx`` equal on every row whose K + 1 smallest distances are pairwise distinct (only there
    does the brute force determine them).  The other rows are not left out: up to 4 096 of them are held to the restatement's
    ``(d, j)`` order instead, and at most 1 % of all rows may then remain unchecked (DESIGN.md 7f has the tie rates)."""
    (gd, gi), (bv, bi) = got, brute
    assert _same_bits(gd, np.ascontiguousarray(bv[:, :K])), np.flatnonzero((gd != bv[:, :K]).any(1))[:10]
    distinct = (np.diff(bv, axis=1) > 0).all(1)
    assert np.array_equal(gi[distinct], bi[distinct, :K]), np.flatnonzero(distinct)[(gi[distinct] != bi[distinct, :K]).any(1)][:10]
    tied = np.flatnonzero(~distinct)
    checked = tied[:4096]
    if len(checked):
        _assert_rows((gd[checked], gi[checked]), knn_points_host(queries[checked], pts, K))
    print(f"rows with a tie among their {K + 1} smallest: {len(tied) / len(gd):.4%}; left unchecked: {(len(tied) - len(checked)) / len(gd):.4%}")
    assert (len(tied) - len(checked)) / len(gd) <= 0.01


@pytest.mark.parametrize("kind", ["cube", "clusters", "plane", "line", "c3"])
def test_50k_equal_the_brute_force(kind):
    pts = _points(kind, 50_000, seed=11)
    dev = torch.from_numpy(pts).to(DEV)
    _assert_against_brute(_run(pts, None, 16), _torch_brute(dev, dev, 16, chunk=2048), 16, pts, pts)


def test_50k_duplicates_equal_the_restatement_on_sampled_queries():
    pts = _points("duplicates", 50_000, seed=11)
    rows = np.sort(np.random.default_rng(12).choice(50_000, 4096, replace=False))
    _assert_rows(_run(pts, None, 16), knn_points_host(pts[rows], pts, 16), rows)


@pytest.mark.parametrize("kind", ["cube", "clusters"])
def test_a_million_points_on_sampled_queries(kind):
    P = 1_000_000
    pts = _points(kind, P, seed=5)
    dev = torch.from_numpy(pts).to(DEV)
    rows = np.sort(np.random.default_rng(P).choice(P, 4096, replace=False))
    gd, gi = _run(pts, None, 16)
    _assert_against_brute((gd[rows], gi[rows]), _torch_brute(dev, dev[torch.from_numpy(rows).to(DEV)], 16, chunk=128), 16, pts[rows], pts)
    queries = _around(pts, 4096, seed=6)
    _assert_against_brute(_run(queries, pts, 16), _torch_brute(dev, torch.from_numpy(queries).to(DEV), 16, chunk=128), 16, queries, pts)


def test_batches_of_two():
    a, b = _points("cube", 1500, seed=1), _points("clusters", 1500, seed=2)
    qa, qb = _around(a, 700, seed=3), _around(b, 700, seed=4)
    p2 = torch.from_numpy(np.stack([a, b])).to(DEV)
    p1 = torch.from_numpy(np.stack([qa, qb])).to(DEV)
    cross, own = knn_points(p1, p2, K=9), knn_points(p2, p2, K=9)
    torch.cuda.synchronize()
    assert cross.dists.shape == (2, 700, 9) and own.idx.shape == (2, 1500, 9) and cross.knn is None
    for n, (q, p) in enumerate(((qa, a), (qb, b))):
        _assert_rows((cross.dists[n].cpu().numpy(), cross.idx[n].cpu().numpy()), knn_points_host(q, p, 9))
        _assert_rows((own.dists[n].cpu().numpy(), own.idx[n].cpu().numpy()), knn_points_host(p, p, 9))


@pytest.mark.parametrize("K", [1, 3, 5, 9])
def test_batches_whose_rows_start_off_16_bytes(K):
    """N = 2 with an odd P1: the second element's ``dists`` and ``idx`` start at P1 K 4 and P1 K 8 bytes, which is no multiple of 16
    for these K (the 16-byte row stores are for K = 4, 8, 16 alone)."""
    a, b = _points("cube", 1501, seed=1), _points("clusters", 1501, seed=2)
    qa, qb = _around(a, 701, seed=3), _around(b, 701, seed=4)
    p2 = torch.from_numpy(np.stack([a, b])).to(DEV)
    p1 = torch.from_numpy(np.stack([qa, qb])).to(DEV)
    cross, own = knn_points(p1, p2, K=K), knn_points(p2, p2, K=K)
    torch.cuda.synchronize()
    assert (701 * K * 4) % 16 != 0 and (1501 * K * 4) % 16 != 0
    for n, (q, p) in enumerate(((qa, a), (qb, b))):
        _assert_rows((cross.dists[n].cpu().numpy(), cross.idx[n].cpu().numpy()), knn_points_host(q, p, K))
        _assert_rows((own.dists[n].cpu().numpy(), own.idx[n].cpu().numpy()), knn_points_host(p, p, K))


def test_side_stream_fed_by_a_kernel_without_sync():
    pts = _points("cube", 200_000, seed=8)
    want = _run(pts, None, 16)
    host = torch.from_numpy(pts).pin_memory()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        x = host.to(DEV, non_blocking=True)
        for _ in range(40):      # a queue of kernels in front, each exact (x * 1 == x)
            x = x * 1.0
        out = knn_points(x[None], x[None], K=16)
        d = torch.empty(out.dists.shape, dtype=torch.float32, pin_memory=True)
        i = torch.empty(out.idx.shape, dtype=torch.int64, pin_memory=True)
        d.copy_(out.dists, non_blocking=True)
        i.copy_(out.idx, non_blocking=True)
    side.synchronize()
    torch.cuda.synchronize()
    _assert_rows((d[0].numpy(), i[0].numpy()), want)


def test_non_contiguous_input():
    wide = _points("cube", 3 * 5000, seed=2).reshape(5000, 9)
    dev = torch.from_numpy(wide).to(DEV)
    p2, p1 = dev[None, :, 3:6], dev[None, :800, 6:9]
    assert not p2.is_contiguous() and not p1.is_contiguous()
    own, cross = knn_points(p2, p2, K=5), knn_points(p1, p2, K=5)
    torch.cuda.synchronize()
    _assert_rows((own.dists[0].cpu().numpy(), own.idx[0].cpu().numpy()), knn_points_host(wide[:, 3:6], wide[:, 3:6], 5))
    _assert_rows((cross.dists[0].cpu().numpy(), cross.idx[0].cpu().numpy()), knn_points_host(wide[:800, 6:9], wide[:, 3:6], 5))


def test_return_nn_gathers_p2():
    pts = _points("clusters", 3000, seed=9)
    p2 = torch.from_numpy(pts).to(DEV)[None]
    p1 = torch.from_numpy(_around(pts, 500, seed=10)).to(DEV)[None]
    out = knn_points(p1, p2, K=8, return_nn=True, return_sorted=False, version=3)
    torch.cuda.synchronize()
    assert out._fields == ("dists", "idx", "knn") and out.knn.shape == (1, 500, 8, 3)
    assert torch.equal(out.knn[0], p2[0][out.idx[0]])
    assert knn_points(p1, p2, K=8).knn is None


def test_permuting_p2_permutes_the_indices():
    pts = _points("clusters", 20_000, seed=4)
    queries = _around(pts, 3000, seed=5)
    perm = np.random.default_rng(9).permutation(len(pts))
    d0, i0 = _run(queries, pts, 16)
    d1, i1 = _run(queries, pts[perm], 16)
    assert _same_bits(d0, d1)
    no_tie = (np.diff(d0, axis=1) > 0).all(1)
    assert no_tie.mean() > 0.99
    assert np.array_equal(perm[i1[no_tie]], i0[no_tie])


def test_two_calls_are_byte_identical():
    pts = _points("duplicates", 100_000, seed=6)
    a, b = _run(pts, None, 16), _run(pts, None, 16)
    assert _same_bits(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_gradients_against_float64_autograd():
    P1, P2, K = 1000, 1025, 16
    pts, queries, _rows, _self, (wd, wi) = _sized_case(P2)
    p1 = torch.from_numpy(queries.copy()).to(DEV)[None].requires_grad_(True)
    p2 = torch.from_numpy(pts.copy()).to(DEV)[None].requires_grad_(True)
    out = knn_points(p1, p2, K=K)
    assert out.dists.requires_grad and not out.idx.requires_grad
    g = torch.from_numpy(np.random.default_rng(1).normal(0, 1, (1, P1, K)).astype(F)).to(DEV)
    out.dists.backward(g)
    torch.cuda.synchronize()
    _assert_rows((out.dists[0].detach().cpu().numpy(), out.idx[0].cpu().numpy()), (wd, wi))      # the forward bits are unchanged

    a = torch.from_numpy(queries.astype(np.float64)).requires_grad_(True)
    b = torch.from_numpy(pts.astype(np.float64)).requires_grad_(True)
    idx = torch.from_numpy(wi)
    g64 = g[0].cpu().double()
    (((a[:, None] - b[idx]) ** 2).sum(-1) * g64).sum().backward()
    # every element is a sum of n terms 2 g (p1 - p2[idx]): each term carries three roundings, the sum n - 1 more at most
    mag = (2 * g64.abs()[..., None] * (a.detach()[:, None] - b.detach()[idx]).abs())             # [P1, K, 3]
    sum1, n1 = mag.sum(1), torch.full((P1, 1), float(K), dtype=torch.float64)
    sum2 = torch.zeros(P2, 3, dtype=torch.float64).index_add_(0, idx.reshape(-1), mag.reshape(-1, 3))
    n2 = torch.zeros(P2, dtype=torch.float64).index_add_(0, idx.reshape(-1), torch.ones(P1 * K, dtype=torch.float64))[:, None]
    for got, want, total, n in ((p1.grad[0], a.grad, sum1, n1), (p2.grad[0], b.grad, sum2, n2)):
        err = (got.cpu().double() - want).abs()
        bound = (n + 3) * 2.0 ** -24 * total
        print(f"largest error / bound: {(err / bound.clamp_min(1e-300)).max().item():.3f}")
        assert torch.all(err <= bound)
    assert torch.all(p2.grad[0][n2[:, 0].to(DEV) == 0] == 0)                                      # nobody's neighbour: no gradient

    # the indices alone, from inputs that require gradients, need no backward
    only = knn_points(p1, p2, K=K).idx[0]
    assert not only.requires_grad and (p2.detach()[0][only] ** 2).sum().item() > 0
    torch.cuda.synchronize()


def test_missing_slots_add_no_gradient():
    few = _points("cube", 40, seed=5)
    few[10:] = np.nan
    p = torch.from_numpy(few).to(DEV)[None].requires_grad_(True)
    out = knn_points(p, p, K=16)
    finite = torch.isfinite(out.dists)
    torch.where(finite, out.dists, torch.zeros_like(out.dists)).sum().backward()
    torch.cuda.synchronize()
    assert torch.isfinite(p.grad[0, :10]).all() and (out.idx[0, :, 10:] == -1).all()


@pytest.fixture
def hooked_pytorch3d():
    """A stub pytorch3d whose knn_points must never run, a module that imported it as sugar_model.py does, the hook installed."""
    names = ("pytorch3d", "pytorch3d.ops", "pytorch3d.ops.knn", "stub_sugar_model_importer")
    saved = {k: sys.modules.pop(k) for k in names if k in sys.modules}

    def knn_points(*args, **kwargs):
        raise AssertionError("the original ran")

    def knn_gather(*args, **kwargs):
        raise AssertionError("not called")

    root, ops, leaf, user = (types.ModuleType(n) for n in names)
    leaf.knn_points, leaf.knn_gather = knn_points, knn_gather
    ops.knn, ops.knn_points, root.ops, user.knn_points = leaf, knn_points, ops, knn_points
    sys.modules.update(zip(names, (root, ops, leaf, user)))
    path = list(sys.path)
    try:
        hook.install(path=False)
        yield user
    finally:
        hook.uninstall()
        sys.path[:] = path
        for k in names:
            sys.modules.pop(k, None)
        sys.modules.update(saved)


def test_sugars_calls_through_the_hook(hooked_pytorch3d):
    call = hooked_pytorch3d.knn_points                       # from pytorch3d.ops import knn_points
    pts = _points("clusters", 5000, seed=13)
    points = torch.nn.Parameter(torch.from_numpy(pts).to(DEV))
    # sugar_model.py:233
    knns = call(points[None], points[None], K=16)
    knn_dists, knn_idx = knns.dists[0], knns.idx[0]
    torch.cuda.synchronize()
    _assert_rows((knn_dists.detach().cpu().numpy(), knn_idx.cpu().numpy()), knn_points_host(pts, pts, 16))
    # :914
    edge_centers = (points[knn_idx[:, 1]] + points).detach() / 2
    edge_knn = call(edge_centers[None], edge_centers[None], K=8)
    edge_knn_idx = edge_knn.idx[0]
    torch.cuda.synchronize()
    ec = edge_centers.cpu().numpy()
    _assert_rows((edge_knn.dists[0].cpu().numpy(), edge_knn_idx.cpu().numpy()), knn_points_host(ec, ec, 8))
    # :1213, the points requiring a gradient
    x = torch.from_numpy(_around(pts, 2000, seed=14)).to(DEV)
    closest_gaussians_idx = call(x[None], points[None], K=16).idx[0]
    torch.cuda.synchronize()
    assert np.array_equal(closest_gaussians_idx.cpu().numpy(), knn_points_host(x.cpu().numpy(), pts, 16)[1])
    (points[closest_gaussians_idx] ** 2).sum().backward()     # what the caller goes on to do with them
    assert points.grad is not None


@pytest.mark.parametrize("K", [5, 16])
def test_every_output_element_is_written(K):
    from autovfx_amd import _lib
    pts, queries, _rows, (sd, si), (cd, ci) = _sized_case(1025)
    p2, p1 = torch.from_numpy(pts).to(DEV), torch.from_numpy(queries).to(DEV)
    for q, (wd, wi) in ((p2, (sd, si)), (p1, (cd, ci))):
        n1 = q.shape[0]
        dists = torch.full((n1 * K * 4,), 0xFF, dtype=torch.uint8, device=DEV)
        idx = torch.full((n1 * K * 8,), 0xFF, dtype=torch.uint8, device=DEV)
        nbytes = int(_lib.lib.gsr_knn_points_scratch_bytes(n1, 1025, int(q is p2)))
        scratch = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = _lib.lib.gsr_knn_points(n1, q.data_ptr(), 1025, p2.data_ptr(), K, dists.data_ptr(), idx.data_ptr(), scratch.data_ptr(), nbytes, stream)
        assert rc == 0, _lib.last_error()
        torch.cuda.synchronize()
        d, i = dists.view(torch.float32).view(n1, K).cpu().numpy(), idx.view(torch.int64).view(n1, K).cpu().numpy()
        assert not (d.view(np.uint32) == 0xFFFFFFFF).any() and not (i == -1).any()       # (finite input, P2 >= K: no empty slot)
        _assert_rows((d, i), (wd[:, :K], wi[:, :K]))
