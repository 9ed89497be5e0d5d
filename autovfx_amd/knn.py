"""The mean squared distance of every point to its three nearest neighbours: simple_knn's ``distCUDA2`` on the GPU.

The reference's 3DGS initialisation (``GaussianModel.create_from_pcd``, ``gaussian_model.py:144``) gives every Gaussian the scale
``log(sqrt(clamp_min(distCUDA2(points), 1e-7)))``; ``simple_knn._C`` at the root of this repository exposes :func:`mean_dist3`
under that name.  The contract ("Nearest neighbours"), pointwise:

* ``d(i, j) = fl(fl(fl(dx*dx) + fl(dy*dy)) + fl(dz*dz))`` with ``dx = fl(x_j - x_i)``, plain fp32 left to right;
* three slots start at ``FLT_MAX``; a distance enters only if it is strictly below a slot, so NaN, inf and ``FLT_MAX`` never do
  (a point with a non-finite coordinate is nobody's neighbour); the self is excluded by index, a duplicate is a neighbour at 0;
* ``out[i] = fl(fl(fl(s0 + s1) + s2) / 3)`` with ``s0 <= s1 <= s2``: ``+inf`` for ``P <= 2`` and for non-finite points,
  ``(s0 + s1 + FLT_MAX) / 3`` for ``P = 3``.

:func:`mean_dist3` runs the HIP kernels of ``gsr_knn.hip`` (C ABI ``gsr_knn3_mean_dist``); :func:`mean_dist3_host` restates the
contract in numpy by brute force, the checker of the tests and a CPU comparator.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

FLT_MAX = float(np.finfo(np.float32).max)
MAX_POINTS = (1 << 30) - 1


def _check(points) -> None:
    if not isinstance(points, torch.Tensor):
        raise TypeError(f"points must be a torch.Tensor, not {type(points).__name__}")
    if points.device.type != "cuda":
        raise ValueError(f"points must be on a GPU (got a tensor on {points.device}); there is no CPU path, see mean_dist3_host")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be [P, 3] (got {list(points.shape)})")
    if points.dtype != torch.float32:
        raise RuntimeError(f"expected a float32 tensor of points, got {points.dtype}")
    if points.shape[0] > MAX_POINTS:
        raise ValueError(f"{points.shape[0]} points: at most 2^30 - 1")


def mean_dist3(points: torch.Tensor) -> torch.Tensor:
    """``points`` float32 ``[P, 3]`` on a GPU -> float32 ``[P]`` on the same device, queued on the current stream (no host
    synchronisation).  Refused before anything is launched: a CPU tensor, a shape other than ``[P, 3]`` (``ValueError``), a dtype other
    than float32 (``RuntimeError``, as the reference's ``data<float>()``).  No autograd."""
    from . import _lib

    _check(points)
    pts = points.detach().contiguous()
    P = int(pts.shape[0])
    out = torch.empty(P, dtype=torch.float32, device=pts.device)
    if P == 0:
        return out
    with torch.cuda.device(pts.device):
        nbytes = int(_lib.lib.gsr_knn3_scratch_bytes(P))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=pts.device)
        stream = ctypes.c_void_p(torch.cuda.current_stream(pts.device).cuda_stream)
        rc = _lib.lib.gsr_knn3_mean_dist(P, pts.data_ptr(), out.data_ptr(), scratch.data_ptr(), nbytes, stream)
    if rc != 0:
        raise RuntimeError(f"gsr_knn3_mean_dist failed ({rc}): {_lib.last_error()}")
    return out


def mean_dist3_host(points, chunk_elems: int = 1 << 23) -> np.ndarray:
    """The contract restated in numpy: every distance in fp32 elementwise operations (no fused multiply-add), the three smallest by
    partition, chunked over the queries.  ``points``: anything ``np.asarray`` takes, reshaped to ``[P, 3]`` float32."""
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.float32).reshape(-1, 3))
    P = pts.shape[0]
    out = np.empty(P, np.float32)
    big = np.float32(FLT_MAX)
    xs, ys, zs = pts[:, 0], pts[:, 1], pts[:, 2]
    step = max(1, chunk_elems // max(P, 1))
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(0, P, step):
            b = min(P, a + step)
            dx = xs[None, :] - xs[a:b, None]
            d = dx * dx
            dy = ys[None, :] - ys[a:b, None]
            d = d + dy * dy
            dz = zs[None, :] - zs[a:b, None]
            d = d + dz * dz
            d[np.arange(b - a), np.arange(a, b)] = big                        # the self, by index
            d = np.where(d < big, d, big)                                     # NaN / inf never enter a slot
            d = np.concatenate([d, np.full((b - a, 3), big, np.float32)], 1)  # missing neighbours stay FLT_MAX
            s = np.sort(np.partition(d, 2, axis=1)[:, :3], axis=1)
            out[a:b] = ((s[:, 0] + s[:, 1]) + s[:, 2]) / np.float32(3.0)
    return out
