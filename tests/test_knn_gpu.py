"""simple_knn's distCUDA2 on the GPU (gsr_knn.hip through autovfx_amd.knn.mean_dist3): bit for bit the contract of
autovfx_amd/knn.py, against the numpy restatement on small inputs and a brute force in eager torch ops on large ones, on the
distributions a COLMAP cloud resembles and the degenerate ones; and the properties a caller relies on."""
from __future__ import annotations

import importlib
import sys

import numpy as np
import pytest
import torch

from autovfx_amd import knn, scenes
from autovfx_amd.knn import FLT_MAX, mean_dist3, mean_dist3_host

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32


def _points(kind: str, P: int, seed: int = 0) -> np.ndarray:
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


def _torch_brute(pts: torch.Tensor, queries: torch.Tensor, chunk: int) -> np.ndarray:
    """The contract in eager torch ops on the GPU, one op per elementwise step; the last division in numpy float32."""
    big = torch.tensor(FLT_MAX, dtype=torch.float32, device=pts.device)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    out = []
    for a in range(0, queries.numel(), chunk):
        qi = queries[a:a + chunk]
        m = qi.numel()
        q = pts[qi]
        dx = x[None, :] - q[:, 0:1]
        d = dx * dx
        dy = y[None, :] - q[:, 1:2]
        d = d + dy * dy
        dz = z[None, :] - q[:, 2:3]
        d = d + dz * dz
        d[torch.arange(m, device=pts.device), qi] = big
        d = torch.where(d < big, d, big)
        d = torch.cat([d, big.expand(m, 3)], 1)
        s = torch.topk(d, 3, dim=1, largest=False).values.sort(dim=1).values
        out.append(s.cpu().numpy())
    s = np.concatenate(out) if out else np.zeros((0, 3), F)
    return ((s[:, 0] + s[:, 1]) + s[:, 2]) / F(3.0)


def _gpu(pts: np.ndarray) -> np.ndarray:
    out = mean_dist3(torch.from_numpy(pts).to(DEV))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 4096])
@pytest.mark.parametrize("kind", ["cube", "clusters"])
def test_small_inputs_equal_the_restatement(kind, P):
    pts = _points(kind, P, seed=P)
    got, want = _gpu(pts), mean_dist3_host(pts)
    assert _same_bits(got, want), np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:10]


def test_hand_built_cases():
    inf = F(np.inf)
    assert _same_bits(_gpu(np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0]], F)), np.full(3, 1.1342745e38, F))
    pts = np.array([[0, 0, 0], [np.nan, 0, 0], [0, 0, 0], [1, 0, 0], [0, np.inf, 0], [2e19, 0, 0], [2e19, 1, 0], [0, 2, 0]], F)
    got = _gpu(pts)
    assert _same_bits(got, mean_dist3_host(pts))
    assert got[1] == inf and got[4] == inf and got[5] == inf and got[6] == inf
    assert _same_bits(_gpu(np.full((300, 3), -1.5, F)), np.zeros(300, F))
    mixed = _points("cube", 2000, seed=3)
    mixed[::7] = np.nan
    mixed[3::11, 1] = -np.inf
    assert _same_bits(_gpu(mixed), mean_dist3_host(mixed))


@pytest.mark.parametrize("kind", ["cube", "clusters", "plane", "line", "duplicates", "c3"])
def test_50k_equal_the_brute_force_everywhere(kind):
    pts = _points(kind, 50_000, seed=11)
    dev = torch.from_numpy(pts).to(DEV)
    got = mean_dist3(dev).cpu().numpy()
    want = _torch_brute(dev, torch.arange(50_000, device=DEV), chunk=2048)
    assert _same_bits(got, want), np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:10]


@pytest.mark.parametrize("P,kind", [(1_000_000, "cube"), (1_000_000, "clusters"), (3_000_000, "cube"), (3_000_000, "clusters"),
                                    (3_000_000, "c3")])
def test_millions_on_sampled_queries(P, kind):
    pts = _points(kind, P, seed=5)
    dev = torch.from_numpy(pts).to(DEV)
    got = mean_dist3(dev).cpu().numpy()
    q = np.sort(np.random.default_rng(P).choice(P, 4096, replace=False))
    want = _torch_brute(dev, torch.from_numpy(q).to(DEV), chunk=64)
    assert _same_bits(got[q], want), q[np.flatnonzero(got[q].view(np.uint32) != want.view(np.uint32))[:10]]


@pytest.mark.parametrize("repeats", [1, 4])
def test_three_slot_search_equals_the_four_slot_self_query(repeats):
    """The two searches answer for each other, not for a restatement: the self query's row is
    [0, d1, d2, d3], so mean_dist3 is ((d1 + d2) + d3) / 3 bit for bit.  20 000 clustered points are 313 leaves under 20 boxes under
    2: the descent, the prune and the re-test of a popped leaf all run.  repeats = 4: every point four times, ties at 0 the rule."""
    pts = np.repeat(_points("clusters", 20_000, seed=13), repeats, axis=0)
    dev = torch.from_numpy(pts).to(DEV)
    d = knn.knn_points(dev[None], dev[None], K=4).dists[0].cpu().numpy()
    got = mean_dist3(dev).cpu().numpy()
    assert d.shape == (len(pts), 4) and np.all(d[:, 0] == 0)
    want = ((d[:, 1] + d[:, 2]) + d[:, 3]) / F(3.0)   # (numpy float32: an IEEE division, as the kernel's)
    assert _same_bits(got, want), np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:10]


def test_permuting_the_input_permutes_the_output():
    pts = _points("clusters", 200_000, seed=4)
    perm = np.random.default_rng(9).permutation(len(pts))
    assert _same_bits(_gpu(pts[perm]), _gpu(pts)[perm])


def test_two_calls_are_byte_identical():
    pts = _points("duplicates", 300_000, seed=6)
    dev = torch.from_numpy(pts).to(DEV)
    a, b = mean_dist3(dev), mean_dist3(dev)
    torch.cuda.synchronize()
    assert _same_bits(a.cpu().numpy(), b.cpu().numpy())


def test_side_stream_fed_by_a_kernel_without_sync():
    pts = _points("cube", 1_000_000, seed=8)
    want = _gpu(pts)
    host = torch.from_numpy(pts).pin_memory()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        x = host.to(DEV, non_blocking=True)
        for _ in range(40):      # a queue of kernels in front, each exact (x * 1 == x)
            x = x * 1.0
        out = mean_dist3(x)
        res = torch.empty(out.shape, dtype=out.dtype, pin_memory=True)
        res.copy_(out, non_blocking=True)
    side.synchronize()
    assert _same_bits(res.numpy(), want)


def test_non_contiguous_input():
    wide = _points("cube", 3 * 5000, seed=2).reshape(5000, 9)
    dev = torch.from_numpy(wide).to(DEV)
    view = dev[:, 3:6]
    assert not view.is_contiguous()
    got = mean_dist3(view)
    torch.cuda.synchronize()
    assert _same_bits(got.cpu().numpy(), mean_dist3_host(wide[:, 3:6]))
    t = torch.from_numpy(_points("cube", 3000, seed=1)).to(DEV).t().contiguous().t()   # [P,3] with strides (1, P)
    assert _same_bits(mean_dist3(t).cpu().numpy(), mean_dist3_host(t.cpu().numpy()))


def test_refusals_before_any_launch():
    with pytest.raises(ValueError):
        mean_dist3(torch.zeros(10, 3))
    with pytest.raises(RuntimeError):
        mean_dist3(torch.zeros(10, 3, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):
        mean_dist3(torch.zeros(10, 4, device=DEV))
    with pytest.raises(ValueError):
        mean_dist3(torch.zeros(30, device=DEV))
    torch.cuda.synchronize()


def test_empty_input():
    out = mean_dist3(torch.zeros(0, 3, device=DEV))
    assert out.shape == (0,) and out.dtype == torch.float32 and out.is_cuda


def test_the_reference_call_shape_end_to_end():
    """create_from_pcd: dist2 = clamp_min(distCUDA2(torch.from_numpy(pts).float().cuda()), 1e-7); scales = log(sqrt(dist2))."""
    saved = {k: sys.modules.pop(k) for k in ("simple_knn", "simple_knn._C") if k in sys.modules}
    try:
        distCUDA2 = importlib.import_module("simple_knn._C").distCUDA2
        pts = _points("clusters", 20_000, seed=12).astype(np.float64)
        pts[:5] = pts[5]                                   # duplicates: the clamp matters
        dist2 = torch.clamp_min(distCUDA2(torch.from_numpy(pts).float().cuda()), 0.0000001)
        scales = torch.log(torch.sqrt(dist2))[..., None].repeat(1, 3)
        want = torch.log(torch.sqrt(torch.clamp_min(torch.from_numpy(mean_dist3_host(pts.astype(F))).cuda(), 0.0000001)))
        torch.cuda.synchronize()
        assert _same_bits(scales[:, 0].cpu().numpy(), want.cpu().numpy())
        assert knn.mean_dist3 is importlib.import_module("simple_knn._C").mean_dist3
    finally:
        for k in ("simple_knn", "simple_knn._C"):
            sys.modules.pop(k, None)
        sys.modules.update(saved)
