"""Meshes, fragments and float64 truths shared by tests/test_meshattrs.py and tests/test_meshattrs_gpu.py."""
from __future__ import annotations

import numpy as np
import torch

F32 = np.float32


def torus(nu: int, nv: int, seed: int, jitter: float = 0.2, grid: float = 0.0):
    """A closed mesh of ``nu * nv`` vertices and ``2 * nu * nv`` faces, every vertex in exactly six faces: a torus of radii 1 and 0.4 cut
    into quads and each quad into two triangles, the vertices moved by up to ``jitter`` of a cell.  ``grid > 0`` rounds the coordinates to
    multiples of it (a power of two: the edge vectors of a face are then exact in fp32)."""
    rng = np.random.default_rng(seed)
    u = (np.arange(nu)[:, None] + jitter * rng.uniform(-1, 1, (nu, nv))) * (2 * np.pi / nu)
    v = (np.arange(nv)[None, :] + jitter * rng.uniform(-1, 1, (nu, nv))) * (2 * np.pi / nv)
    ring = 1.0 + 0.4 * np.cos(v)
    verts = np.stack((ring * np.cos(u), ring * np.sin(u), 0.4 * np.sin(v)), axis=-1).reshape(-1, 3)
    if grid:
        verts = np.round(verts / grid) * grid
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    at = lambda a, b: ((a % nu) * nv + (b % nv)).reshape(-1)
    faces = np.concatenate((np.stack((at(i, j), at(i + 1, j), at(i + 1, j + 1)), 1), np.stack((at(i, j), at(i + 1, j + 1), at(i, j + 1)), 1)))
    return verts.astype(F32), faces[rng.permutation(len(faces))].astype(np.int64)


def random_mesh(V: int, n_faces: int, seed: int):
    """``n_faces`` triangles over ``V >= 3`` random vertices, three different vertices each."""
    rng = np.random.default_rng(seed)
    verts = rng.uniform(-1, 1, (V, 3)).astype(F32)
    faces = np.stack([rng.permutation(V)[:3] for _ in range(n_faces)]).astype(np.int64) if n_faces else np.zeros((0, 3), np.int64)
    return verts, faces


def fan(n_faces: int, seed: int):
    """Vertex 0 in every one of ``n_faces`` faces: a cone over a ring of ``n_faces`` vertices."""
    rng = np.random.default_rng(seed)
    t = np.arange(n_faces) * (2 * np.pi / n_faces)
    ring = np.stack((np.cos(t), np.sin(t), 0.1 * rng.uniform(-1, 1, n_faces)), 1)
    verts = np.concatenate(([[0.0, 0.0, 0.5]], ring)).astype(F32)
    k = np.arange(n_faces)
    return verts, np.stack((np.zeros(n_faces, np.int64), 1 + k, 1 + (k + 1) % n_faces), 1).astype(np.int64)


def fragments(shape, n_faces: int, D: int, seed: int, empty: float = 1 / 3, signed: bool = True):
    """``pix_to_face`` of ``shape`` with about ``empty`` of the slots -1, barycentrics that sum to one, attributes ``[n_faces, 3, D]`` and an
    upstream gradient.  ``signed=False``: attributes in [0, 1), like UVs and colours (no term of the interpolation cancels another)."""
    rng = np.random.default_rng(seed)
    pix = rng.integers(0, max(n_faces, 1), shape).astype(np.int64)
    pix[rng.uniform(size=shape) < empty] = -1
    if n_faces == 0:
        pix[...] = -1
    bary = rng.dirichlet((1.0, 1.0, 1.0), shape).astype(F32)
    attrs = (rng.uniform(-1, 1, (n_faces, 3, D)) if signed else rng.uniform(0, 1, (n_faces, 3, D))).astype(F32)
    grad = rng.uniform(-1, 1, tuple(shape) + (D,)).astype(F32)
    return pix, bary, attrs, grad


# ---- the forward formulas in torch, at any dtype: autograd of these in float64 is the truth -------------------------------------------

def faces_forward_torch(verts: torch.Tensor, faces: torch.Tensor):
    v0, v1, v2 = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    a, b = v1 - v0, v2 - v0
    c = torch.stack((a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]), 1)
    n = torch.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
    return n / 2, c / torch.clamp(n, min=1e-6)[:, None]


def interp_forward_torch(pix: torch.Tensor, bary: torch.Tensor, attrs: torch.Tensor):
    held = pix >= 0
    a = attrs[pix.clamp(min=0)]                                                      # [..., 3, D]
    out = (bary[..., 0, None] * a[..., 0, :] + bary[..., 1, None] * a[..., 1, :]) + bary[..., 2, None] * a[..., 2, :]
    return out * held[..., None]


def faces_gradients_torch(verts, faces, grad_areas, grad_normals, dtype):
    """``(areas, normals, grad_verts)`` of the forward formulas at ``dtype`` by torch's CPU autograd, on the fp32 inputs."""
    v = torch.from_numpy(np.asarray(verts, F32)).to(dtype).requires_grad_(True)
    areas, normals = faces_forward_torch(v, torch.from_numpy(faces))
    loss = (areas * torch.from_numpy(grad_areas).to(dtype)).sum() + (normals * torch.from_numpy(grad_normals).to(dtype)).sum()
    loss.backward()
    return areas.detach().numpy(), normals.detach().numpy(), v.grad.numpy()


def interp_gradients_torch(pix, bary, attrs, grad, dtype):
    """``(out, grad_bary, grad_attrs)`` of the forward formula at ``dtype`` by torch's CPU autograd, on the fp32 inputs."""
    w = torch.from_numpy(bary).to(dtype).requires_grad_(True)
    a = torch.from_numpy(attrs).to(dtype).requires_grad_(True)
    out = interp_forward_torch(torch.from_numpy(pix), w, a)
    (out * torch.from_numpy(grad).to(dtype)).sum().backward()
    return out.detach().numpy(), w.grad.numpy(), a.grad.numpy()


# ---- the scales of the backward comparisons: the absolute values of the products the float64 computation adds up ----------------------

def faces_gradient_scale(verts, faces, grad_areas, grad_normals):
    """``[V, 3]`` float64: per element of ``grad_verts``, the sum over its faces of ``|b_i g_c_j|`` and ``|g_c_i a_j|``, the products of the two
    cross products that make up the face's contribution (both cross products for v0), with ``g_c`` in float64.  No cancellation enters."""
    v = np.asarray(verts, np.float64)
    v0, v1, v2 = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    a, b = v1 - v0, v2 - v0
    c = np.cross(a, b)
    n = np.linalg.norm(c, axis=1)[:, None]
    m = c / n
    g = np.asarray(grad_normals, np.float64)
    gc = np.asarray(grad_areas, np.float64)[:, None] * c / (2 * n) + (g - m * (m * g).sum(1, keepdims=True)) / n
    cross_abs = lambda p, q: np.abs(np.stack((p[:, 1] * q[:, 2], p[:, 2] * q[:, 0], p[:, 0] * q[:, 1]), 1)) + \
        np.abs(np.stack((p[:, 2] * q[:, 1], p[:, 0] * q[:, 2], p[:, 1] * q[:, 0]), 1))
    ga, gb = cross_abs(b, gc), cross_abs(gc, a)
    scale = np.zeros_like(v)
    for i, part in enumerate((ga + gb, ga, gb)):
        np.add.at(scale, faces[:, i], part)
    return scale


def interp_gradient_scales(pix, bary, attrs, grad):
    """``(scale of grad_bary, scale of grad_attrs)`` in float64: the sums of ``|grad[p, d] attrs[f, k, d]|`` over d, and of ``|bary[p, k] grad[p, d]|``
    over the slots that hold the face."""
    flat = pix.reshape(-1)
    held = flat >= 0
    w, g, a = bary.reshape(-1, 3).astype(np.float64), grad.reshape(flat.shape[0], -1).astype(np.float64), attrs.astype(np.float64)
    scale_bary = np.zeros(w.shape)
    scale_bary[held] = np.abs(g[held][:, None, :] * a[flat[held]]).sum(-1)
    scale_attrs = np.zeros(a.shape)
    np.add.at(scale_attrs, flat[held], np.abs(w[held][:, :, None] * g[held][:, None, :]))
    return scale_bary.reshape(bary.shape), scale_attrs


def relative_to(scale, got, truth):
    """The largest ``|got - truth| / scale`` over the elements with a positive scale; elements of scale 0 must be exactly 0."""
    got, truth = np.asarray(got, np.float64), np.asarray(truth, np.float64)
    assert np.all(got[scale == 0] == 0)
    live = scale > 0
    return float((np.abs(got - truth)[live] / scale[live]).max()) if live.any() else 0.0


# ---- the bound on an atomically summed element -------------------------------------------------------------------------------------

def atomic_sum_check(got, terms, index, size, what: str):
    """``got [size, ...]`` against the fp32 ``terms [T, ...]`` added to rows ``index [T]`` in any order: per element
    ``|got - S| <= (n + 2) 2^-24 sum|t_i| + n 2^-149`` with S the float64 sum and n the number of terms; n = 1 must be the term's bits and
    n = 0 exactly 0.  Returns the largest error over the bound (elements with n >= 2)."""
    got = np.asarray(got, F32).reshape(size, -1)
    terms = np.asarray(terms, F32).reshape(len(index), got.shape[1])
    total, total_abs = np.zeros(got.shape), np.zeros(got.shape)
    count = np.zeros(size, np.int64)
    np.add.at(total, index, terms.astype(np.float64))
    np.add.at(total_abs, index, np.abs(terms.astype(np.float64)))
    np.add.at(count, index, 1)
    assert np.isfinite(got).all(), what
    assert np.all(got[count == 0] == 0), f"{what}: an element nothing is added to is not 0"
    once = count == 1
    if once.any():
        single = np.zeros(got.shape, F32)
        rows = np.nonzero(once[index])[0]
        single[index[rows]] = terms[rows]
        assert np.array_equal(got[once] + F32(0.0), single[once] + F32(0.0)), f"{what}: an element with one term is not that term"   # (+0: -0 == 0)
    n = count[:, None].astype(np.float64)
    bound = (n + 2) * 2.0 ** -24 * total_abs + n * 2.0 ** -149
    err = np.abs(got.astype(np.float64) - total)
    assert np.all(err <= bound), f"{what}: {int((err > bound).sum())} elements outside the bound, worst {float((err / np.maximum(bound, 1e-300)).max()):.3g} x"
    many = count >= 2
    return float((err[many] / bound[many]).max()) if many.any() else 0.0
