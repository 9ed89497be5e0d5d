"""Nearest neighbours on the GPU: simple_knn's ``distCUDA2`` (the mean squared distance of every point to its three nearest
neighbours) and pytorch3d's ``knn_points`` (the K nearest neighbours of every query, with their indices).

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

:func:`knn_points` is ``pytorch3d.ops.knn_points`` as SuGaR calls it (``sugar/sugar_scene/sugar_model.py:233``, ``:899``, ``:914``,
``:1213``), on the same tree and walk with K slots per query (C ABI ``gsr_knn_points``).  Its contract, pointwise:

* the same ``d(i, j)``, ``dx = fl(p2[j].x - p1[i].x)``; the candidates of query ``i`` are all ``j`` with ``d(i, j) < FLT_MAX`` -- the self
  is not excluded (``p1 is p2`` returns it first, at 0), NaN, inf and ``FLT_MAX`` never qualify;
* row ``i`` is the K smallest candidates in ascending ``(d, j)`` order: equal distances go by the lower index;
* ``dists`` float32, ``idx`` int64; a row with fewer than K candidates ends in ``(+inf, -1)`` (a deliberate deviation: pytorch3d's
  behaviour on non-finite input is unspecified).

:func:`knn_points_host` restates it in numpy; :func:`drop_in` is what ``autovfx_amd.install()`` puts in place of pytorch3d's.
"""
from __future__ import annotations

from typing import Callable, NamedTuple, Optional

import numpy as np
import torch

from . import _takes

FLT_MAX = float(np.finfo(np.float32).max)
MAX_POINTS = (1 << 30) - 1
MAX_K = 16


def _check(points) -> None:
    if not isinstance(points, torch.Tensor):
        raise TypeError(f"points must be a torch.Tensor, not {type(points).__name__}")
    # (the dtype is judged after the shape and with the reference's exception: here any dtype passes)
    _takes.refuse("mean_dist3", _takes.tensors((("points", points, points.dtype),), host="mean_dist3_host")
                  or _takes.shaped("points", points, "[P, 3]", points.dim() == 2 and points.shape[1] == 3))
    if points.dtype != torch.float32:
        raise RuntimeError(f"expected a float32 tensor of points, got {points.dtype}")
    if points.shape[0] > MAX_POINTS:
        _takes.refuse("mean_dist3", f"{points.shape[0]} points: at most 2^30 - 1")


def mean_dist3(points: torch.Tensor) -> torch.Tensor:
    """``points`` float32 ``[P, 3]`` on a GPU -> float32 ``[P]`` on the same device, queued on the current stream (no host
    synchronisation).  Refused before anything is launched: a CPU tensor, a shape other than ``[P, 3]`` (``ValueError``), a dtype other
    than float32 (``RuntimeError``, as the reference's ``data<float>()``).  No autograd."""
    from . import _lib

    _check(points)
    pts = _takes.c(points)
    P = int(pts.shape[0])
    out = torch.empty(P, dtype=torch.float32, device=pts.device)
    if P == 0:
        return out
    with torch.cuda.device(pts.device):
        scratch, nbytes = _lib.scratch("gsr_knn3_scratch_bytes", P, device=pts.device)
        _lib.call("gsr_knn3_mean_dist", P, pts.data_ptr(), out.data_ptr(), scratch.data_ptr(), nbytes, device=pts.device)
    return out


def _sq_dists(queries: np.ndarray, candidates: np.ndarray) -> np.ndarray:
    """``d(i, j)`` of the contract for float32 ``queries [C, 3]`` and ``candidates [P, 3]`` -> float32 ``[C, P]``: candidate minus
    query per axis, the squares summed left to right, every operation an fp32 elementwise one (no fused multiply-add).  Overflow and
    NaN pass through: the caller holds ``np.errstate``."""
    dx = candidates[None, :, 0] - queries[:, 0:1]
    d = dx * dx
    dy = candidates[None, :, 1] - queries[:, 1:2]
    d = d + dy * dy
    dz = candidates[None, :, 2] - queries[:, 2:3]
    d = d + dz * dz
    return d


def mean_dist3_host(points, chunk_elems: int = 1 << 23) -> np.ndarray:
    """The contract restated in numpy: every distance in fp32 elementwise operations (no fused multiply-add), the three smallest by
    partition, chunked over the queries.  ``points``: anything ``np.asarray`` takes, reshaped to ``[P, 3]`` float32."""
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.float32).reshape(-1, 3))
    P = pts.shape[0]
    out = np.empty(P, np.float32)
    big = np.float32(FLT_MAX)
    step = max(1, chunk_elems // max(P, 1))
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(0, P, step):
            b = min(P, a + step)
            d = _sq_dists(pts[a:b], pts)
            d[np.arange(b - a), np.arange(a, b)] = big                        # the self, by index
            d = np.where(d < big, d, big)                                     # NaN / inf never enter a slot
            d = np.concatenate([d, np.full((b - a, 3), big, np.float32)], 1)  # missing neighbours stay FLT_MAX
            s = np.sort(np.partition(d, 2, axis=1)[:, :3], axis=1)
            out[a:b] = ((s[:, 0] + s[:, 1]) + s[:, 2]) / np.float32(3.0)
    return out


class KNN(NamedTuple):
    """pytorch3d.ops.knn's ``_KNN``: the same field names in the same order."""
    dists: torch.Tensor
    idx: torch.Tensor
    knn: Optional[torch.Tensor]


def _why_not(p1, p2, lengths1, lengths2, norm, K) -> Optional[str]:
    """None when the kernels take the call, else the reason they do not."""
    why = (_takes.tensors((("p1", p1, torch.float32), ("p2", p2, torch.float32)), host="knn_points_host")
           or _takes.shaped("p1", p1, "[N, P1, 3]", p1.dim() == 3 and p1.shape[2] == 3)
           or _takes.shaped("p2", p2, "[N, P2, 3]", p2.dim() == 3 and p2.shape[2] == 3))
    if why is not None:
        return why
    if p1.shape[0] != p2.shape[0] or p1.shape[0] < 1:
        return f"p1 and p2 must have the same batch size N >= 1 (got {p1.shape[0]} and {p2.shape[0]})"
    if lengths1 is not None or lengths2 is not None:
        return "lengths1 / lengths2 are not supported"
    if norm != 2:
        return f"norm must be 2 (got {norm!r})"
    if type(K) is not int or not 1 <= K <= MAX_K:
        return f"K must be an int in 1..{MAX_K} (got {K!r})"
    if p2.shape[1] < K:
        return f"p2 has {p2.shape[1]} points, fewer than K = {K}"
    if p1.shape[1] > MAX_POINTS or p2.shape[1] > MAX_POINTS:
        return f"{p1.shape[1]} and {p2.shape[1]} points: at most 2^30 - 1 each"
    return _takes.capturing("the call allocates its scratch")


def knn_points_takes(p1, p2, lengths1=None, lengths2=None, norm=2, K=1, version=-1, return_nn=False, return_sorted=True) -> bool:
    """Whether :func:`knn_points` runs this call: CUDA float32 ``[N, P, 3]`` on one device, ``N >= 1``, no ``lengths``, ``norm == 2``,
    ``1 <= K <= 16``, ``P2 >= K``, ``P1, P2 < 2^30``, not under graph capture.  Inputs that require gradients are taken."""
    return _why_not(p1, p2, lengths1, lengths2, norm, K) is None


def _same_view(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a is b or (a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.stride() == b.stride())


def _search(p1: torch.Tensor, p2: torch.Tensor, K: int):
    """``[N, P1, 3]``, ``[N, P2, 3]`` (checked) -> ``dists [N, P1, K]`` float32, ``idx [N, P1, K]`` int64, on the current stream."""
    from . import _lib

    same = _same_view(p1, p2)
    c1 = _takes.c(p1)
    c2 = c1 if same else _takes.c(p2)
    N, P1, P2 = int(c1.shape[0]), int(c1.shape[1]), int(c2.shape[1])
    dists = torch.empty((N, P1, K), dtype=torch.float32, device=c1.device)
    idx = torch.empty((N, P1, K), dtype=torch.int64, device=c1.device)
    if P1 == 0:
        return dists, idx
    with torch.cuda.device(c1.device):
        scratch, nbytes = _lib.scratch("gsr_knn_points_scratch_bytes", P1, P2, int(same), device=c1.device)
        for n in range(N):   # (the batch elements share the scratch: they run one after the other on the stream)
            _lib.call("gsr_knn_points", P1, c1[n].data_ptr(), P2, c2[n].data_ptr(), K, dists[n].data_ptr(), idx[n].data_ptr(),
                      scratch.data_ptr(), nbytes, device=c1.device)
    return dists, idx


class _KnnPoints(torch.autograd.Function):
    """Forward: the kernels.  Backward: pytorch3d's rule for ``norm == 2`` in torch ops,
    ``g1[i] = sum_k 2 g[i,k] (p1[i] - p2[idx[i,k]])`` and the negated terms added into ``g2`` rows; ``idx == -1`` slots add nothing."""

    @staticmethod
    def forward(ctx, p1, p2, K):
        dists, idx = _search(p1, p2, K)
        ctx.save_for_backward(p1, p2, idx)
        ctx.mark_non_differentiable(idx)
        return dists, idx

    @staticmethod
    def backward(ctx, grad_dists, _grad_idx):
        p1, p2, idx = ctx.saved_tensors
        valid = idx >= 0
        safe = idx.clamp_min(0)
        N, P1, K = idx.shape
        near = torch.gather(p2, 1, safe.reshape(N, P1 * K, 1).expand(-1, -1, 3)).reshape(N, P1, K, 3)
        terms = (2.0 * grad_dists.to(torch.float32))[..., None] * (p1[:, :, None, :] - near)
        terms = torch.where(valid[..., None], terms, torch.zeros((), dtype=torch.float32, device=idx.device))   # (a NaN query's too)
        g1 = terms.sum(2) if ctx.needs_input_grad[0] else None
        g2 = None
        if ctx.needs_input_grad[1]:
            g2 = torch.zeros_like(p2)
            for n in range(N):
                g2[n].index_add_(0, safe[n].reshape(-1), -terms[n].reshape(-1, 3))
        return g1, g2, None


def _taken(p1, p2, K: int, return_nn: bool) -> KNN:
    """A call ``_why_not`` let through."""
    dists, idx = _KnnPoints.apply(p1, p2, K)
    near = None
    if return_nn:
        N, P1 = idx.shape[:2]
        near = torch.gather(p2, 1, idx.clamp_min(0).reshape(N, P1 * K, 1).expand(-1, -1, 3)).reshape(N, P1, K, 3)
    return KNN(dists, idx, near)


def knn_points(p1, p2, lengths1=None, lengths2=None, norm: int = 2, K: int = 1, version: int = -1, return_nn: bool = False,
               return_sorted: bool = True) -> KNN:
    """``pytorch3d.ops.knn_points``: for every point of ``p1 [N, P1, 3]`` its K nearest in ``p2 [N, P2, 3]`` -- squared distances
    ``dists [N, P1, K]`` (differentiable in both inputs), ``idx [N, P1, K]`` int64, and ``knn = p2`` gathered by ``idx``
    ``[N, P1, K, 3]`` with ``return_nn`` (else None; a missing slot, ``idx == -1``, holds ``p2[n, 0]`` there, a placeholder: mask
    by ``idx >= 0``).  Rows are always sorted (``return_sorted=False`` allows it);
    ``version`` is ignored.  Passing the same tensor twice is the self query, which needs no second sort.  A call
    :func:`knn_points_takes` rejects raises ``ValueError`` with the reason; queued on the current stream, no host synchronisation."""
    _takes.refuse("knn_points", _why_not(p1, p2, lengths1, lengths2, norm, K))
    return _taken(p1, p2, K, return_nn)


def drop_in(original: Callable) -> Callable:
    """A ``knn_points`` that runs the kernels for the calls :func:`knn_points_takes` accepts and ``original`` (pytorch3d's, same
    signature) for every other: CPU tensors, ``lengths``, other norms, K above 16, and 2-D points
    (``sugar_extractors/refined_mesh.py:147``).  ``autovfx_amd.install()`` builds it around ``pytorch3d.ops.knn.knn_points``."""
    def knn_points_drop_in(p1, p2, lengths1=None, lengths2=None, norm=2, K=1, version=-1, return_nn=False, return_sorted=True):
        if _why_not(p1, p2, lengths1, lengths2, norm, K) is not None:
            return original(p1, p2, lengths1=lengths1, lengths2=lengths2, norm=norm, K=K, version=version, return_nn=return_nn,
                            return_sorted=return_sorted)
        return _taken(p1, p2, K, return_nn)

    return _takes.dressed(knn_points_drop_in, "knn_points", original, "pytorch3d.ops.knn_points", "knn")


def knn_points_host(p1, p2, K: int, chunk_elems: int = 1 << 23):
    """The contract of :func:`knn_points` restated in numpy for one batch element: every distance in fp32 elementwise operations (no
    fused multiply-add), a lexsort on ``(d, j)``, chunked over the queries.  ``p1``, ``p2``: anything ``np.asarray`` takes,
    reshaped to ``[P, 3]`` float32.  Returns ``dists [P1, K]`` float32 and ``idx [P1, K]`` int64; ``P2 < K`` pads with ``(inf, -1)``."""
    a1 = np.ascontiguousarray(np.asarray(p1, dtype=np.float32).reshape(-1, 3))
    a2 = np.ascontiguousarray(np.asarray(p2, dtype=np.float32).reshape(-1, 3))
    P1, P2 = a1.shape[0], a2.shape[0]
    dists = np.full((P1, K), np.inf, np.float32)
    idx = np.full((P1, K), -1, np.int64)
    big = np.float32(FLT_MAX)
    step = max(1, chunk_elems // max(P2, 1))
    k = min(K, P2)
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(0, P1, step):
            b = min(P1, a + step)
            d = _sq_dists(a1[a:b], a2)
            d = np.where(d < big, d, np.float32(np.inf))      # NaN / inf / FLT_MAX are no candidates
            # only what is not above the k-th smallest distance of its row can be in the row: lexsort those by (row, d, j)
            rows, cols = np.nonzero(d <= np.partition(d, k - 1, axis=1)[:, k - 1:k])
            dd = d[rows, cols]
            order = np.lexsort((cols, dd, rows))
            first = np.searchsorted(rows[order], np.arange(b - a))[:, None] + np.arange(k)[None, :]
            dk, jk = dd[order][first], cols[order][first]
            found = dk < big
            dists[a:b, :k] = np.where(found, dk, np.float32(np.inf))
            idx[a:b, :k] = np.where(found, jk, -1)
    return dists, idx
