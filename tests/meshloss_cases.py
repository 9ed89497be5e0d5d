"""Meshes and the float64 truth shared by tests/test_meshloss.py and tests/test_meshloss_gpu.py.

The truth is pytorch3d's own route through ``mesh_normal_consistency`` restated in torch at any dtype: the hashed-edge ``unique`` with its
inverse, the sort of the ``3F`` face-edge incidences and their ``bincount``, the pair enumeration of ``find_verts`` on the host, three
cross products summed, ``1 - cosine_similarity(n0, -n1)`` and the weights ``1 / P``.  It shares nothing with the product's sort by
``(lo, hi)``."""
from __future__ import annotations

import numpy as np
import torch

from meshattrs_cases import F32, fan, random_mesh, torus  # noqa: F401  (the meshes of the face-normal tests serve here too)


# ---- meshes ---------------------------------------------------------------------------------------------------------------------------

def grid(nx: int, ny: int, step: float = 2.0 ** -3):
    """A flat, consistently oriented grid of ``nx * ny`` quads (two faces each) in the plane z = 1/4, coordinates multiples of ``step``."""
    i, j = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="ij")
    verts = np.stack((i * step, j * step, np.full(i.shape, 0.25)), -1).reshape(-1, 3)
    at = lambda a, b: (a * (ny + 1) + b).reshape(-1)
    a, b = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    faces = np.concatenate((np.stack((at(a, b), at(a + 1, b), at(a + 1, b + 1)), 1), np.stack((at(a, b), at(a + 1, b + 1), at(a, b + 1)), 1)))
    return verts.astype(F32), faces.astype(np.int64)


def cube():
    """The unit cube, twelve outward faces: twelve folds of 90 degrees and six flat diagonals among its 18 edges."""
    verts = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], F32)          # index 4 x + 2 y + z
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    faces = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    return verts, np.array(faces, np.int64)


def tetrahedron():
    """A regular tetrahedron: six edges, every fold the same angle, cos = 1/3 between the outward normals."""
    verts = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], F32)
    return verts, np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int64)


def book(c: int, seed: int):
    """``c`` faces around the one edge (0, 1): ``c (c - 1) / 2`` pairs on it, and 2 c edges with one face each.  Every other page is
    wound the other way."""
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(0, 2 * np.pi, c))
    pages = np.stack((np.cos(t), np.sin(t), rng.uniform(0.2, 0.8, c)), 1)
    verts = np.concatenate(([[0.0, 0.0, 0.0], [0.0, 0.0, 1.0]], pages)).astype(F32)
    k = np.arange(c)
    faces = np.stack((np.where(k % 2 == 0, 0, 1), np.where(k % 2 == 0, 1, 0), 2 + k), 1)
    return verts, faces.astype(np.int64)


def strip(n_faces: int, seed: int):
    """An open strip of ``n_faces`` triangles over ``n_faces + 2`` vertices: ``n_faces - 1`` interior edges, the rest on the border."""
    rng = np.random.default_rng(seed)
    k = np.arange(n_faces + 2)
    verts = np.stack((0.5 * k, (k % 2).astype(np.float64), 0.2 * rng.uniform(-1, 1, n_faces + 2)), 1).astype(F32)
    f = np.arange(n_faces)
    faces = np.where((f % 2 == 0)[:, None], np.stack((f, f + 1, f + 2), 1), np.stack((f + 1, f, f + 2), 1))
    return verts, faces.astype(np.int64)


# ---- pytorch3d's route ------------------------------------------------------------------------------------------------------------------

def find_verts(edge_num: np.ndarray) -> np.ndarray:
    """pytorch3d's ``_C.mesh_normal_consistency_find_verts``: for the edges in order, with ``c = edge_num[e]`` incidences starting at the
    running offset ``o``, the pairs ``(o + i, o + j)``, ``i < j``.  ``[P, 2]`` int64."""
    out, offset = [], 0
    for c in edge_num.tolist():
        for i in range(c):
            for j in range(i + 1, c):
                out.append((offset + i, offset + j))
        offset += c
    return np.array(out, np.int64).reshape(-1, 2)


def topology_torch(faces: torch.Tensor, V: int):
    """``(edges_packed [E, 2], edge_idx [3F] sorted, vert_idx [3F, 3], edge_num [E], pairs [P, 2])`` as pytorch3d builds them."""
    F = faces.shape[0]
    v0, v1, v2 = faces.unbind(1)
    edges = torch.cat((torch.stack((v1, v2), 1), torch.stack((v2, v0), 1), torch.stack((v0, v1), 1)), 0)
    edges, _ = edges.sort(dim=1)
    unique, inverse = torch.unique(V * edges[:, 0] + edges[:, 1], return_inverse=True)
    edges_packed = torch.stack((unique // V, unique % V), 1)
    face_to_edge = inverse.reshape(3, F).t()                                   # [F, 3]: the edge opposite each corner
    edge_idx = face_to_edge.reshape(-1)
    vert_idx = faces.view(-1, 1, 3).expand(-1, 3, -1).reshape(-1, 3)
    edge_idx, edge_sort_idx = edge_idx.sort()
    vert_idx = vert_idx[edge_sort_idx]
    edge_num = edge_idx.bincount(minlength=edges_packed.shape[0])
    pairs = torch.from_numpy(find_verts(edge_num.cpu().numpy())).to(faces.device)    # (the host round trip of the original)
    return edges_packed, edge_idx, vert_idx, edge_num, pairs


def normal_consistency_torch(verts: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
    """pytorch3d's ``mesh_normal_consistency`` for one mesh of ``F >= 1`` faces, at ``verts``' dtype and on its device; ``tensor([0.])``-like
    ``[1]`` zeros when no edge is shared."""
    edges_packed, edge_idx, vert_idx, _edge_num, pairs = topology_torch(faces, verts.shape[0])
    if pairs.shape[0] == 0:
        return torch.zeros((1,), dtype=verts.dtype, device=verts.device, requires_grad=verts.requires_grad)
    v0_idx, v1_idx = edges_packed.unbind(1)
    v0, v1 = verts[v0_idx[edge_idx]], verts[v1_idx[edge_idx]]
    n_temp0 = torch.cross(v1 - v0, verts[vert_idx[:, 0]] - v0, dim=1)
    n_temp1 = torch.cross(v1 - v0, verts[vert_idx[:, 1]] - v0, dim=1)
    n_temp2 = torch.cross(v1 - v0, verts[vert_idx[:, 2]] - v0, dim=1)
    n = n_temp0 + n_temp1 + n_temp2
    n0, n1 = n[pairs[:, 0]], -n[pairs[:, 1]]
    loss = 1 - torch.cosine_similarity(n0, n1, dim=1)
    weights = torch.full((pairs.shape[0],), 1.0 / pairs.shape[0], dtype=verts.dtype, device=verts.device)
    return (loss * weights).sum()


def gradients_torch(verts, faces, grad_loss: float, dtype):
    """``(loss, grad_verts)`` of pytorch3d's route at ``dtype`` by torch's CPU autograd, on the fp32 inputs."""
    v = torch.from_numpy(np.asarray(verts, F32)).to(dtype).requires_grad_(True)
    loss = normal_consistency_torch(v, torch.from_numpy(np.asarray(faces, np.int64))).sum()
    (loss * grad_loss).backward()
    return loss.detach().numpy(), v.grad.numpy()


def edge_counts(faces, V: int) -> np.ndarray:
    """The truth's ``bincount``: incidences per edge."""
    return topology_torch(torch.from_numpy(np.asarray(faces, np.int64)), V)[3].numpy()


# ---- float64 analysis of the pairs: the scale of the gradient, the error a term may carry ---------------------------------------------------

def _pair_geometry(verts, faces):
    """Per pair of the truth's table, in float64: ``lo, hi, opp_s, opp_t`` and ``e, w_s, w_t, n_s, n_t``."""
    v = np.asarray(verts, np.float64)
    faces_t = torch.from_numpy(np.asarray(faces, np.int64))
    edges_packed, edge_idx, vert_idx, _num, pairs = (t.numpy() for t in topology_torch(faces_t, v.shape[0]))
    lo, hi = edges_packed[edge_idx, 0], edges_packed[edge_idx, 1]
    # the corner of an incidence that is not on its edge (a face that repeats an index: any corner serves, its normal is zero)
    off = (vert_idx != lo[:, None]) & (vert_idx != hi[:, None])
    opp = vert_idx[np.arange(len(lo)), off.argmax(1)]
    s, t = pairs[:, 0], pairs[:, 1]
    e = v[hi[s]] - v[lo[s]]
    ws, wt = v[opp[s]] - v[lo[s]], v[opp[t]] - v[lo[s]]
    return lo[s], hi[s], opp[s], opp[t], e, ws, wt, np.cross(e, ws), np.cross(e, wt)


def _cross_abs(p, q):
    return np.abs(np.stack((p[:, 1] * q[:, 2], p[:, 2] * q[:, 0], p[:, 0] * q[:, 1]), 1)) + \
        np.abs(np.stack((p[:, 2] * q[:, 1], p[:, 0] * q[:, 2], p[:, 1] * q[:, 0]), 1))


def normal_consistency_gradient_scale(verts, faces, grad_loss: float) -> np.ndarray:
    """``[V, 3]`` float64: per element of ``grad_verts``, the sum over the pairs of the absolute products of the cross products that make up a
    pair's contribution to it (``|w_i g_j|`` for ``hi``, ``|g_i e_j|`` for the opposite vertices, all of them for ``lo``), with the pair's
    gradients ``g_s, g_t`` in float64.  No cancellation enters."""
    v = np.asarray(verts, np.float64)
    scale = np.zeros_like(v)
    lo, hi, os_, ot, e, ws, wt, ns, nt = _pair_geometry(verts, faces)
    if len(lo) == 0:
        return scale
    a, b = np.linalg.norm(ns, axis=1), np.linalg.norm(nt, axis=1)
    live = (a > 1e-8) & (b > 1e-8)                                             # (the scale is asked for on meshes without such faces)
    a, b = np.where(live, a, 1.0), np.where(live, b, 1.0)
    cos = (ns * nt).sum(1) / (a * b)
    c = grad_loss / len(lo)
    gs = c * (nt / (a * b)[:, None] - (cos / a ** 2)[:, None] * ns) * live[:, None]
    gt = c * (ns / (a * b)[:, None] - (cos / b ** 2)[:, None] * nt) * live[:, None]
    on_hi = _cross_abs(ws, gs) + _cross_abs(wt, gt)
    on_s, on_t = _cross_abs(gs, e), _cross_abs(gt, e)
    for rows, part in ((hi, on_hi), (os_, on_s), (ot, on_t), (lo, on_hi + on_s + on_t)):
        np.add.at(scale, rows, part)
    return scale


def term_error_bound(verts, faces) -> float:
    """The mean over the pairs of what fp32 may put on one term ``1 + d / (a b)``, from float64 geometry.  A normal ``n = e x w`` of fp32
    differences carries at most ``4 * 2^-24 (|e_i w_j| + |e_j w_i|)`` per component (one rounding in each of e and w, one per product, one
    for the difference), so at most ``8 * 2^-24 |e| |w|`` in length; a cosine moves by at most the relative change of each normal; the dot
    product, the two norms, the product ``a b``, the division and the addition of 1 round another 12 times on a value of at most 2."""
    _lo, _hi, _os, _ot, e, ws, wt, ns, nt = _pair_geometry(verts, faces)
    if len(e) == 0:
        return 0.0
    le = np.linalg.norm(e, axis=1)
    tilt = le * np.linalg.norm(ws, axis=1) / np.linalg.norm(ns, axis=1) + le * np.linalg.norm(wt, axis=1) / np.linalg.norm(nt, axis=1)
    return float((2.0 ** -24 * (8 * tilt + 24)).mean())


def relative_to(scale, got, truth) -> float:
    """The largest ``|got - truth| / scale`` over the elements with a positive scale; elements of scale 0 must be exactly 0."""
    got, truth = np.asarray(got, np.float64), np.asarray(truth, np.float64)
    assert np.all(got[scale == 0] == 0)
    live = scale > 0
    return float((np.abs(got - truth)[live] / scale[live]).max()) if live.any() else 0.0


# ---- a pytorch3d that is not there: Meshes, and a pytorch3d.loss package on disk ---------------------------------------------------------

class StubMeshes:
    """What the drop-in asks of pytorch3d's ``Meshes``: ``len``, ``verts_packed()``, ``faces_packed()``."""

    def __init__(self, verts, faces, count: int = 1):
        self._verts, self._faces, self._count = verts, faces, count

    def __len__(self):
        return self._count

    def verts_packed(self):
        return self._verts

    def faces_packed(self):
        return self._faces


STUB_PACKAGE = {
    "pytorch3d/__init__.py": "",
    "pytorch3d/loss/__init__.py": "from .mesh_normal_consistency import mesh_normal_consistency\n",
    "pytorch3d/loss/mesh_normal_consistency.py": (
        "calls = []\n\n\n"
        "def mesh_normal_consistency(meshes):\n"
        "    calls.append(meshes)\n"
        "    import meshloss_cases\n"
        "    return meshloss_cases.normal_consistency_torch(meshes.verts_packed(), meshes.faces_packed())\n"),
    "stub_trainer_refine.py": "from pytorch3d.loss import mesh_normal_consistency\n",
    "stub_trainer_coarse.py": "from pytorch3d.loss import mesh_normal_consistency as consistency\n",
    "stub_trainer_other.py": "import pytorch3d.loss\nfrom pytorch3d.loss import mesh_normal_consistency\n",
}
STUB_MODULES = ("pytorch3d", "pytorch3d.loss", "pytorch3d.loss.mesh_normal_consistency", "stub_trainer_refine", "stub_trainer_coarse",
                "stub_trainer_other")


def write_stub_package(root) -> None:
    """A ``pytorch3d.loss`` whose ``__init__`` does the ``from``-import, and three trainers that bind the function, under ``root``."""
    import os

    for name, text in STUB_PACKAGE.items():
        path = os.path.join(str(root), name)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as fh:
            fh.write(text)
