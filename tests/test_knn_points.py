"""pytorch3d's knn_points without a GPU: the numpy restatement of the contract (autovfx_amd/knn.py: knn_points_host) against a float64
truth and against hand-built rows, which calls the kernels take, the hook's patch of a stub pytorch3d, and the C ABI's refusals."""
from __future__ import annotations

import sys
import types

import numpy as np
import pytest
import torch

from autovfx_amd import hook, knn
from autovfx_amd.knn import knn_points_host, knn_points_takes
from helpers import fake_gpu as _gpu

F = np.float32
REL = 16 * 2.0 ** -24          # the bound tests/test_knn.py holds the same expression to


def _cloud(kind: str, P: int = 2000) -> np.ndarray:
    g = np.random.default_rng(21)
    if kind == "uniform":
        pts = g.uniform(-3, 3, (P, 3))
    elif kind == "clustered":
        pts = np.concatenate([g.normal(c, 0.05, (P // 8, 3)) for c in g.uniform(-10, 10, (8, 3))])
    elif kind == "collinear":
        pts = np.c_[g.uniform(-1, 1, P), np.full(P, -0.25), np.full(P, 2.0)]
    elif kind == "lattice":
        pts = g.integers(0, 13, (P, 3))
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(pts, dtype=F)


@pytest.mark.parametrize("K", [1, 5, 16])
@pytest.mark.parametrize("kind", ["uniform", "clustered", "collinear", "lattice"])
def test_restatement_against_float64_truth(kind, K):
    pts = _cloud(kind)
    q = pts[::3] if kind == "lattice" else _cloud(kind)[::3] + F(0.01)
    got_d, got_i = knn_points_host(q, pts, K)
    d64 = ((pts.astype(np.float64)[None, :, :] - q.astype(np.float64)[:, None, :]) ** 2).sum(-1)
    order = np.argsort(d64, axis=1, kind="stable")
    s64 = np.take_along_axis(d64, order, axis=1)
    assert np.all(np.abs(got_d.astype(np.float64) - s64[:, :K]) <= REL * s64[:, :K])
    # the sets of indices are the truth's wherever slots K and K + 1 are further apart than the rounding could bridge
    clear = s64[:, K] - s64[:, K - 1] > REL * s64[:, K]
    assert clear.sum() > (0 if kind == "lattice" else len(q) // 2)
    assert np.array_equal(np.sort(got_i[clear], axis=1), np.sort(order[clear, :K], axis=1))


def test_restatement_is_chunk_independent():
    pts = _cloud("lattice", 333)
    ref = knn_points_host(pts[:100], pts, 7)
    for chunk in (1, 333, 5 * 333 + 7):
        got = knn_points_host(pts[:100], pts, 7, chunk_elems=chunk)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])


def test_lattice_with_duplicates_is_in_d_then_j_order():
    grid = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), -1).reshape(-1, 3).astype(F)
    pts = np.concatenate([grid, grid[::5], grid[:7]])            # every distance an integer, many of them equal
    K = 16
    d, i = knn_points_host(pts, pts, K)
    exact = ((pts[None, :, :].astype(np.int64) - pts[:, None, :].astype(np.int64)) ** 2).sum(-1)
    for row in range(len(pts)):
        want = sorted((int(exact[row, j]), j) for j in range(len(pts)))[:K]
        assert [(int(a), int(b)) for a, b in zip(d[row], i[row])] == want, row
    # the self, or a duplicate of it with a lower index, comes first at 0
    assert np.all(d[:, 0] == 0) and np.all(i[:, 0] <= np.arange(len(pts)))
    assert np.array_equal(i[:64, 0], np.arange(64))


def test_a_nan_point_is_in_nobodys_row_and_has_an_empty_row():
    pts = _cloud("uniform", 40)
    pts[7, 1] = np.nan
    pts[9, 0] = np.inf
    d, i = knn_points_host(pts, pts, 16)
    assert not np.isin(i, (7, 9)).any()
    for bad in (7, 9):
        assert np.all(np.isposinf(d[bad])) and np.all(i[bad] == -1)
    ok = np.setdiff1d(np.arange(40), (7, 9))
    assert np.all(np.isfinite(d[ok])) and np.all(i[ok] >= 0) and np.array_equal(i[ok, 0], ok)
    # fewer candidates than K: the rest of the row is (inf, -1)
    d, i = knn_points_host(pts[:12], pts[:12], 16)
    assert np.all(np.isfinite(d[0, :10])) and np.all(np.isposinf(d[0, 10:])) and np.all(i[0, 10:] == -1)


def test_which_calls_the_kernels_take():
    a, b = _gpu(1, 50, 3), _gpu(1, 40, 3)
    assert knn_points_takes(a, b, K=16)
    assert knn_points_takes(a, a, K=1)
    assert knn_points_takes(_gpu(2, 50, 3), _gpu(2, 40, 3), K=8)                                   # N = 2
    with torch.enable_grad():
        assert knn_points_takes(_gpu(1, 50, 3, requires_grad=True), _gpu(1, 40, 3, requires_grad=True), K=16)
    assert knn_points_takes(a, b, None, None, 2, 4, -1, True, False)                                 # pytorch3d's positional order
    assert not knn_points_takes(torch.zeros(1, 50, 3), torch.zeros(1, 40, 3), K=4)                   # CPU tensors
    assert not knn_points_takes(a, torch.zeros(1, 40, 3), K=4)
    assert not knn_points_takes(_gpu(1, 50, 3, dtype=torch.float16), _gpu(1, 40, 3, dtype=torch.float16), K=4)
    assert not knn_points_takes(_gpu(1, 50, 2), _gpu(1, 40, 2), K=2)                                 # D = 2
    assert not knn_points_takes(_gpu(50, 3), _gpu(40, 3), K=2)
    assert not knn_points_takes(a, b, K=0)
    assert not knn_points_takes(a, b, K=17)
    assert not knn_points_takes(a, _gpu(1, 3, 3), K=4)                                               # P2 < K
    assert knn_points_takes(a, _gpu(1, 4, 3), K=4)
    assert not knn_points_takes(a, b, lengths1=torch.tensor([50]), K=4)
    assert not knn_points_takes(a, b, lengths2=torch.tensor([40]), K=4)
    assert not knn_points_takes(a, b, norm=1, K=4)
    assert not knn_points_takes(_gpu(2, 50, 3), b, K=4)                                              # batch sizes differ
    assert not knn_points_takes(_gpu(0, 50, 3), _gpu(0, 40, 3), K=4)
    with pytest.raises(ValueError, match="GPU"):
        knn.knn_points(torch.zeros(1, 50, 3), torch.zeros(1, 40, 3), K=4)
    with pytest.raises(ValueError, match="norm"):
        knn.knn_points(a, b, norm=1, K=4)
    with pytest.raises(ValueError, match="K must be"):
        knn.knn_points(a, b, K=17)


@pytest.fixture
def stub_pytorch3d():
    """pytorch3d / pytorch3d.ops / pytorch3d.ops.knn as far as the hook looks at them, and a module that imported knn_points."""
    names = ("pytorch3d", "pytorch3d.ops", "pytorch3d.ops.knn", "stub_sugar_importer")
    saved = {k: sys.modules.pop(k) for k in names if k in sys.modules}
    calls = []

    def knn_points(p1, p2, lengths1=None, lengths2=None, norm=2, K=1, version=-1, return_nn=False, return_sorted=True):
        calls.append((tuple(p1.shape), tuple(p2.shape), K))
        return "the original's result"

    def knn_gather(x, idx, lengths=None):
        raise AssertionError("not called")

    root, ops, leaf, user = (types.ModuleType(n) for n in names)
    knn_points.__module__ = knn_gather.__module__ = leaf.__name__
    leaf.knn_points, leaf.knn_gather = knn_points, knn_gather
    ops.knn, ops.knn_points, ops.knn_gather = leaf, knn_points, knn_gather
    root.ops = ops
    user.knn_points = knn_points                               # from pytorch3d.ops import knn_points
    sys.modules.update(zip(names, (root, ops, leaf, user)))
    try:
        yield leaf, ops, user, knn_points, calls
    finally:
        hook.uninstall()
        for k in names:
            sys.modules.pop(k, None)
        sys.modules.update(saved)


def test_hook_replaces_every_binding_and_uninstall_restores_them(stub_pytorch3d):
    leaf, ops, user, original, calls = stub_pytorch3d
    path = list(sys.path)
    try:
        hook.install(path=False)
        ours = leaf.knn_points
        assert ours is not original and ours.fallback is original
        assert ops.knn_points is ours and user.knn_points is ours
        assert leaf.reference_knn_points is original
        assert leaf.knn_gather is ops.knn_gather                       # nothing else moved
        assert "pytorch3d.ops.knn" in hook.patched_modules
        hook.install(path=False)                                       # a second install changes nothing
        assert leaf.knn_points is ours and ops.knn_points is ours and user.knn_points is ours
        assert leaf.reference_knn_points is original
        # what the kernels do not take reaches the original: a CPU call, and refined_mesh.py's 2-D call
        assert user.knn_points(torch.zeros(1, 9, 3), torch.zeros(1, 8, 3), K=4) == "the original's result"
        assert ops.knn_points(_gpu(1, 9, 2), _gpu(1, 8, 2), K=2) == "the original's result"
        assert calls == [((1, 9, 3), (1, 8, 3), 4), ((1, 9, 2), (1, 8, 2), 2)]
        hook.uninstall()
        assert leaf.knn_points is original and ops.knn_points is original and user.knn_points is original
        assert not hasattr(leaf, "reference_knn_points")
        assert hook.patched_modules == []
    finally:
        sys.path[:] = path


def test_cabi_version_and_refusals_need_no_device():
    from autovfx_amd import _lib
    L = _lib.lib
    assert L.gsr_abi_version() == 20 == _lib.ABI_VERSION
    need = L.gsr_knn_points_scratch_bytes(1000, 2000, 0)
    assert 0 < need <= 48 * 3000 + 32768
    assert L.gsr_knn_points_scratch_bytes(2000, 2000, 1) < L.gsr_knn_points_scratch_bytes(2000, 2000, 0)
    for bad in ((-1, 5), (5, -1), (1 << 30, 5), (5, 1 << 30)):
        assert L.gsr_knn_points_scratch_bytes(*bad, 0) == 0
    p1, p2, dists, idx, scratch = 4096, 8192, 1 << 16, 1 << 17, 1 << 20      # addresses that are never read: every call is refused

    def refused(*args, word):
        return L.gsr_knn_points(*args, None) != 0 and word in _lib.last_error()

    assert L.gsr_knn_points(0, None, 0, None, 1, None, None, None, 0, None) == 0                 # n1 == 0: nothing to do
    assert L.gsr_knn_points(0, None, 2000, p2, 16, None, None, None, 0, None) == 0
    assert refused(1000, p1, 2000, p2, 0, dists, idx, scratch, need, word="K = 0")
    assert refused(1000, p1, 2000, p2, 17, dists, idx, scratch, need, word="K = 17")
    assert refused(1000, p1, 15, p2, 16, dists, idx, scratch, need, word="less than K")
    assert refused(-1, p1, 2000, p2, 4, dists, idx, scratch, need, word="negative")
    assert refused(1000, p1, -2000, p2, 4, dists, idx, scratch, need, word="negative")
    assert refused(1 << 30, p1, 2000, p2, 4, dists, idx, scratch, 1 << 40, word="2^30")
    assert refused(1000, p1, 1 << 30, p2, 4, dists, idx, scratch, 1 << 40, word="2^30")
    for hole in range(5):
        ptrs = [p1, p2, dists, idx, scratch]
        ptrs[hole] = None
        assert refused(1000, ptrs[0], 2000, ptrs[1], 4, ptrs[2], ptrs[3], ptrs[4], need, word="null"), hole
    assert refused(1000, p1 + 2, 2000, p2, 4, dists, idx, scratch, need, word="aligned")
    assert refused(1000, p1, 2000, p2 + 1, 4, dists, idx, scratch, need, word="aligned")
    assert refused(1000, p1, 2000, p2, 4, dists + 4, idx, scratch, need, word="aligned")
    assert refused(1000, p1, 2000, p2, 4, dists, idx + 8, scratch, need, word="aligned")
    assert refused(1000, p1, 2000, p2, 16, dists + 4, idx, scratch, need, word="aligned")
    assert refused(1000, p1, 2000, p2, 5, dists + 2, idx, scratch, need, word="aligned")      # other K: 4 and 8 bytes
    assert refused(1000, p1, 2000, p2, 5, dists, idx + 4, scratch, need, word="aligned")
    assert refused(1000, p1, 2000, p2, 5, dists + 4, idx + 8, scratch, need - 1, word="scratch")  # ... which this one meets
    assert refused(1000, p1, 2000, p2, 4, dists, idx, scratch + 128, need, word="aligned")
    assert refused(1000, p1, 2000, p2, 4, dists, idx, scratch, need - 1, word="scratch too small")
    same = L.gsr_knn_points_scratch_bytes(2000, 2000, 1)
    assert refused(2000, p2, 2000, p2, 4, dists, idx, scratch, same - 1, word="scratch too small")
