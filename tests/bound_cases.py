"""Meshes, the float64 truth and the bars shared by tests/test_bound.py, tests/test_bound_gpu.py, tests/golden/make_bound_fixtures.py and
scripts/bench_bound.py.

**The truth** is :func:`face_forward`, a torch restatement of the contract of ``autovfx_amd/bound.py`` at any dtype, run in float64 with
autograd.  **The stub model** (:class:`StubSuGaR`) has the three properties in the shape of the reference's chain of torch operations -- the
comparator of the drop-ins and of the benchmark -- and :func:`matrix_to_quaternion` restates pytorch3d 0.7.4's.

**The bars** come from the fixtures ``tests/golden/bound/ref_*.npz`` -- the reference's own three getters, fp32 on the CPU -- and from
nothing else: per tensor, the largest ratio over all fixtures of the reference's error against the truth to ``2^-24 x`` a per-element
scale, times 4 (another summation order in the three-term sums, a 2-ulp ``expf``).  The scales:

* ``points``: ``|v0 b0| + |v1 b1| + |v2 b2|`` per coordinate; ``scaling``: the element's own magnitude;
* ``quaternions``: 1 for every component -- the last step divides the row by its length, which mixes the four components' errors, so
  a component's error is relative to the unit length of the row, not to its own size;
* the gradients: ``sum |J| |g|`` over the outputs of the face (``grad_verts``: summed over the vertex's faces), with ``J`` the float64
  Jacobian of the face's outputs and ``g`` the upstream gradient: the absolute terms of the chain-rule sum that forms the element.
  ``grad_verts`` adds the absolute products of the two cross products through which ``c = a x b`` reaches the vertices, ``|b_i g_c_j|`` and
  ``|g_c_i a_j|`` with ``g_c`` in float64, as ``meshattrs_cases.faces_gradient_scale`` does (7j): they cancel for every displacement of a vertex
  that leaves the normal alone, and without them torch's own fp32 autograd of the truth's formulas is 19 x ``2^-24 x scale`` off.
  ``grad_complex`` takes the same sum through ``z = complex / |complex|``: that normalisation's backward is the difference
  ``gz_b / |c| - z_b (gz . z) / |c|``, which cancels along the radius, so the scale is ``sum_a (delta_ab + |z_a| |z_b|) / |c| x sum_o |dq_o / dz_a| |g_o|``,
  the absolute terms of that difference.

Measured on the eight fixtures (the reference's ratio / the bar, in units of ``2^-24 x scale``; ``RECORDED`` below)::

    points 2.222 / 8.89        scaling 1.004 / 4.02         quaternions 2.472 / 9.89
    grad_verts 3.379 / 13.5    grad_complex 5.753 / 23.0    grad_log_scales 1.712 / 6.85

(:func:`bars` computes them from the files; tests/test_bound.py asserts that they are the numbers above.)

**Near-tie rows.**  A row whose two largest ``q_abs`` of the truth are within 1e-3 of each other may take another candidate in fp32.
Those rows are compared through ``quaternion_to_matrix``, which does not see the sign -- each entry of the matrix is ``1 - 2 (qa^2 + qb^2)``
or ``2 (qa qb +- qc qd)`` of a unit quaternion, so an error ``e`` per component moves it by at most ``2 (|qa| + |qb| + |qc| + |qd|) e <= 4 e``: the
bar there is 4 x that of the quaternions, in units of ``2^-24`` (the reference reaches 3.05) -- and are left out of the gradient
comparisons, together with the vertices of their faces.  At most 1 % of a
case's rows may be near ties: :func:`near_ties` asserts it.
"""
from __future__ import annotations

import glob
import os

import numpy as np
import torch

from meshattrs_cases import faces_forward_torch, torus

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = os.path.join(HERE, "golden", "bound")
TIE = 1e-3
OUTPUTS = ("points", "scaling", "quaternions")
GRADS = ("grad_verts", "grad_complex", "grad_log_scales")

# the barycentric coordinates SuGaR gives 1, 3, 4 and 6 Gaussians per triangle (values, sugar_model.py:170-210)
BARY = {1: [[1 / 3, 1 / 3, 1 / 3]],
        3: [[1 / 2, 1 / 4, 1 / 4], [1 / 4, 1 / 2, 1 / 4], [1 / 4, 1 / 4, 1 / 2]],
        4: [[1 / 3, 1 / 3, 1 / 3], [2 / 3, 1 / 6, 1 / 6], [1 / 6, 2 / 3, 1 / 6], [1 / 6, 1 / 6, 2 / 3]],
        6: [[2 / 3, 1 / 6, 1 / 6], [1 / 6, 2 / 3, 1 / 6], [1 / 6, 1 / 6, 2 / 3], [1 / 6, 5 / 12, 5 / 12], [5 / 12, 1 / 6, 5 / 12], [5 / 12, 5 / 12, 1 / 6]]}


def bary_of(G: int) -> np.ndarray:
    if G in BARY:
        return np.asarray(BARY[G], F32)
    return np.random.default_rng(G).dirichlet((2.0, 2.0, 2.0), G).astype(F32)


# ---- cases ------------------------------------------------------------------------------------------------------------------------------

def _parameters(n_faces: int, G: int, rng):
    N = n_faces * G
    return dict(bary=bary_of(G), complex=rng.normal(0, 1, (N, 2)).astype(F32), log_scales=rng.uniform(-6, -2, (N, 2)).astype(F32),
                thickness=np.asarray(F32(3.7e-6)), grad_points=rng.uniform(-1, 1, (N, 3)).astype(F32),
                grad_scaling=rng.uniform(-1, 1, (N, 3)).astype(F32), grad_quaternions=rng.uniform(-1, 1, (N, 4)).astype(F32))


def torus_case(nu: int, nv: int, G: int, seed: int) -> dict:
    """``2 nu nv`` faces of a jittered torus, ``G`` Gaussians each."""
    verts, faces = torus(nu, nv, seed)
    return dict(verts=verts, faces=faces, **_parameters(len(faces), G, np.random.default_rng(1000 + seed)))


def sized_case(n_faces: int, G: int, seed: int, V: int = 0, spread: bool = False) -> dict:
    """Exactly ``n_faces`` faces: the first of a torus large enough.  ``V`` > the torus' vertices appends unused ones; ``spread`` moves the
    used ones to indices spread up to ``V - 1``."""
    nv = 5
    nu = max(3, -(-n_faces // (2 * nv)))
    verts, faces = torus(nu, nv, seed)
    faces = faces[:n_faces]
    if V > len(verts):
        rng = np.random.default_rng(seed)
        where = np.concatenate((np.sort(rng.choice(V - 1, len(verts) - 1, replace=False)), [V - 1])) if spread else np.arange(len(verts))
        all_verts = rng.uniform(-1, 1, (V, 3)).astype(F32)
        all_verts[where] = verts
        verts, faces = all_verts, where[faces].astype(np.int64)
    return dict(verts=verts, faces=faces, **_parameters(n_faces, G, np.random.default_rng(2000 + seed)))


def shared_case(n_faces: int, G: int, seed: int) -> dict:
    """``n_faces`` faces over the same three vertices (in rotating order): every vertex gets ``n_faces`` atomic terms."""
    rng = np.random.default_rng(seed)
    verts = rng.uniform(-1, 1, (3, 3)).astype(F32)
    faces = np.stack([np.roll(np.arange(3), i % 3) for i in range(n_faces)]).astype(np.int64)
    return dict(verts=verts, faces=faces, **_parameters(n_faces, G, rng))


def _rotation_about(axis: np.ndarray, angle: float) -> np.ndarray:
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def branch_case(candidate: int, n_faces: int, G: int, seed: int) -> dict:
    """Faces whose frame ``[R_0 | R_1 | R_2]`` is a turn by 0..0.5 rad (candidate 0) or a near-half-turn (2.6..3.1 rad, either sense) about an
    axis within 0.15 rad of x, y or z (candidates 1, 2, 3): that candidate of ``matrix_to_quaternion`` wins on every row.  Every face has
    its own three vertices."""
    rng = np.random.default_rng(3000 + 10 * candidate + seed)
    verts, comp = [], []
    for _ in range(n_faces):
        axis = np.eye(3)[max(candidate - 1, 0)] + 0.15 * rng.uniform(-1, 1, 3) / np.sqrt(3)
        angle = rng.uniform(0.0, 0.5) if candidate == 0 else rng.choice((-1, 1)) * rng.uniform(2.6, 3.1)
        T = _rotation_about(axis, angle)
        r0, t1, t2 = T[:, 0], T[:, 1], T[:, 2]
        phi = rng.uniform(-np.pi, np.pi)
        b1 = np.cos(phi) * t1 - np.sin(phi) * t2
        b2 = np.cross(r0, b1)
        v0 = rng.uniform(-1, 1, 3)
        v1 = v0 - rng.uniform(0.05, 0.2) * b1
        v2 = v0 + rng.uniform(-0.1, 0.1) * b1 - rng.uniform(0.05, 0.2) * b2
        verts += [v0, v1, v2]
        for g in range(G):
            psi = phi + rng.uniform(-0.02, 0.02)
            comp.append(rng.uniform(0.5, 2.0) * np.array([np.cos(psi), np.sin(psi)]))
    verts = np.asarray(verts, F32)
    faces = np.arange(3 * n_faces, dtype=np.int64).reshape(-1, 3)
    case = dict(verts=verts, faces=faces, **_parameters(n_faces, G, rng))
    case["complex"] = np.asarray(comp, F32)
    return case


def tie_case() -> dict:
    """One face whose frame is exactly a quarter turn about x, every operation exact in fp32: ``q_abs[0] == q_abs[1] == sqrt(2)``."""
    case = dict(verts=np.array([[0, 0, 1], [0, 0, 0], [0, 1, 1]], F32), faces=np.array([[0, 1, 2]], np.int64),
                **_parameters(1, 1, np.random.default_rng(5)))
    case["complex"] = np.array([[1.0, 0.0]], F32)
    return case


# ---- pytorch3d's names, restated ---------------------------------------------------------------------------------------------------------

def matrix_to_quaternion_074(R: torch.Tensor) -> torch.Tensor:
    """``autovfx_amd.dynamic_scene.matrix_to_quaternion`` (the algorithm of pytorch3d 0.7.4) for ``[..., 3, 3]`` torch tensors, with autograd:
    the four ``pre``, a square root that is 0 with a zero gradient where ``pre <= 0``, the four candidate rows over ``2 max(q_abs, 0.1)``,
    and the row of the first largest ``q_abs`` picked with a boolean mask -- a ``nonzero``, as in pytorch3d, so that the host
    synchronisation of the reference's chain stays visible to the tests and the benchmark."""
    lead = R.shape[:-2]
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = (R.reshape(lead + (9,))[..., i] for i in range(9))
    pre = torch.stack((1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22, 1.0 - m00 - m11 + m22), -1)
    live = pre > 0
    q_abs = torch.where(live, torch.sqrt(torch.where(live, pre, torch.ones_like(pre))), torch.zeros_like(pre))
    sq = q_abs * q_abs
    cand = torch.stack((torch.stack((sq[..., 0], m21 - m12, m02 - m20, m10 - m01), -1),
                        torch.stack((m21 - m12, sq[..., 1], m10 + m01, m02 + m20), -1),
                        torch.stack((m02 - m20, m10 + m01, sq[..., 2], m12 + m21), -1),
                        torch.stack((m10 - m01, m20 + m02, m21 + m12, sq[..., 3]), -1)), -2)
    cand = cand / (2.0 * q_abs.clamp_min(0.1))[..., None]
    taken = torch.arange(4, device=R.device) == q_abs.argmax(-1, keepdim=True)
    return cand[taken].reshape(lead + (4,))


matrix_to_quaternion = matrix_to_quaternion_074      # the name StubSuGaR.quaternions looks up, as the reference's module does: tests replace it


def matrix_to_quaternion_standardized(matrix: torch.Tensor) -> torch.Tensor:
    """What later pytorch3d releases return: the same, with a non-negative real part."""
    q = matrix_to_quaternion_074(matrix)
    return torch.where(q[..., 0:1] < 0, -q, q)


def quaternion_to_matrix(q: np.ndarray) -> np.ndarray:
    q = np.asarray(q, np.float64)
    r, i, j, k = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    two_s = 2.0 / (q * q).sum(-1)
    return np.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                     two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                     two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)), axis=-1)


class StubMeshes:
    """``Meshes`` as far as ``SuGaR.quaternions`` uses it: ``faces_normals_list()`` by the forward of DESIGN.md 7j in torch."""

    def __init__(self, verts, faces, textures=None):
        self._verts, self._faces = verts[0], faces[0]

    def faces_normals_list(self):
        return [faces_forward_torch(self._verts, self._faces)[1]]


class StubSuGaR:
    """A model bound to a surface mesh with the three properties as chains of torch operations in the reference's shape (its own
    ``points``, ``scaling`` and ``quaternions``, ``sugar_model.py:376-391``, ``:408-423``, ``:425-452``, restated), and the attributes the
    drop-ins read."""

    def __init__(self, case: dict, device="cpu", requires_grad: bool = False):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self.device = torch.device(device)
        self.binded_to_surface_mesh, self.editable, self.scale_activation = True, False, torch.exp
        self._points = t(case["verts"]).requires_grad_(requires_grad)
        self._surface_mesh_faces = t(case["faces"])
        self.surface_triangle_bary_coords = t(case["bary"])[..., None]
        self.n_gaussians_per_surface_triangle = int(case["bary"].shape[0])
        self._quaternions = t(case["complex"]).requires_grad_(requires_grad)
        self._scales = t(case["log_scales"]).requires_grad_(requires_grad)
        self.surface_mesh_thickness = t(np.asarray(case["thickness"], F32).reshape(()))
        self._n_points = len(case["complex"])

    @property
    def surface_mesh(self):
        return StubMeshes(verts=[self._points], faces=[self._surface_mesh_faces])

    def get_covariance(self, **kwargs):
        raise NotImplementedError

    @property
    def points(self):
        if not self.binded_to_surface_mesh:
            return self._points
        corners = self._points[self._surface_mesh_faces]
        return (corners[:, None] * self.surface_triangle_bary_coords[None]).sum(dim=-2).reshape(self._n_points, 3)

    @property
    def scaling(self):
        if not self.binded_to_surface_mesh:
            return self.scale_activation(self._scales)
        if self.editable:
            raise NotImplementedError("the editable scale factor is the reference's alone")
        return torch.cat([self.surface_mesh_thickness * torch.ones(len(self._scales), 1, device=self.device), self.scale_activation(self._scales)], dim=-1)

    @property
    def quaternions(self):
        if not self.binded_to_surface_mesh:
            return torch.nn.functional.normalize(self._quaternions, dim=-1)
        unit = torch.nn.functional.normalize
        F, G = len(self._surface_mesh_faces), self.n_gaussians_per_surface_triangle
        corners = self._points[self._surface_mesh_faces]
        normal = unit(self.surface_mesh.faces_normals_list()[0], dim=-1)                      # the first axis: the face normal
        edge = unit(corners[:, 0] - corners[:, 1], dim=-1)                                    # the frame's second axis before the turn
        third = unit(torch.cross(normal, edge, dim=-1))
        turn = unit(self._quaternions, dim=-1).view(F, G, 2)                                  # the learned turn about the normal
        cos, sin = turn[..., 0:1], turn[..., 1:2]
        columns = (normal[:, None].expand(F, G, 3), cos * edge[:, None] + sin * third[:, None], -sin * edge[:, None] + cos * third[:, None])
        R = torch.stack(columns, dim=-1).reshape(F * G, 3, 3)
        return unit(matrix_to_quaternion(R), dim=-1)


# ---- the truth: the contract in torch, at any dtype ---------------------------------------------------------------------------------------

def face_forward(corners, bary, complex, log_scales, thickness, standardize: bool = False, complex_is_unit: bool = False, c=None):
    """``corners [..., 3, 3]`` (vertex, coordinate), ``bary [G, 3]``, ``complex [..., G, 2]``, ``log_scales [..., G, 2]`` ->
    ``(points [..., G, 3], scaling [..., G, 3], quaternions [..., G, 4], q_abs [..., G, 4])`` by the contract of autovfx_amd/bound.py."""
    unit = lambda w: w / torch.clamp(torch.sqrt((w * w).sum(-1, keepdim=True)), min=1e-12)
    cross = lambda u, w: torch.stack((u[..., 1] * w[..., 2] - u[..., 2] * w[..., 1], u[..., 2] * w[..., 0] - u[..., 0] * w[..., 2],
                                      u[..., 0] * w[..., 1] - u[..., 1] * w[..., 0]), -1)
    v0, v1, v2 = corners[..., 0, :], corners[..., 1, :], corners[..., 2, :]
    c = cross(v1 - v0, v2 - v0) if c is None else c                 # (given: the scales differentiate with respect to it)
    normal = c / torch.clamp(torch.sqrt((c * c).sum(-1, keepdim=True)), min=1e-6)
    r0 = unit(normal)
    b1 = unit(v0 - v1)
    b2 = unit(cross(r0, b1))
    z = complex if complex_is_unit else unit(complex)
    r0, b1, b2 = r0[..., None, :], b1[..., None, :], b2[..., None, :]
    r1 = z[..., 0:1] * b1 + z[..., 1:2] * b2
    r2 = -z[..., 1:2] * b1 + z[..., 0:1] * b2
    r0 = r0.expand(r1.shape)
    m = lambda i, j: (r0, r1, r2)[j][..., i]
    pre = torch.stack((1 + m(0, 0) + m(1, 1) + m(2, 2), 1 + m(0, 0) - m(1, 1) - m(2, 2), 1 - m(0, 0) + m(1, 1) - m(2, 2),
                       1 - m(0, 0) - m(1, 1) + m(2, 2)), -1)
    positive = pre > 0
    q_abs = torch.where(positive, torch.sqrt(torch.where(positive, pre, torch.ones_like(pre))), torch.zeros_like(pre))
    rows = torch.stack((
        torch.stack((q_abs[..., 0] ** 2, m(2, 1) - m(1, 2), m(0, 2) - m(2, 0), m(1, 0) - m(0, 1)), -1),
        torch.stack((m(2, 1) - m(1, 2), q_abs[..., 1] ** 2, m(1, 0) + m(0, 1), m(0, 2) + m(2, 0)), -1),
        torch.stack((m(0, 2) - m(2, 0), m(1, 0) + m(0, 1), q_abs[..., 2] ** 2, m(1, 2) + m(2, 1)), -1),
        torch.stack((m(1, 0) - m(0, 1), m(2, 0) + m(0, 2), m(2, 1) + m(1, 2), q_abs[..., 3] ** 2), -1)), -2)
    rows = rows / (2 * torch.clamp(q_abs, min=0.1))[..., None]
    k = q_abs.detach().argmax(-1)
    u = torch.gather(rows, -2, k[..., None, None].expand(k.shape + (1, 4)))[..., 0, :]
    if standardize:
        u = torch.where(u[..., 0:1] < 0, -u, u)
    quaternions = unit(u)
    points = (v0[..., None, :] * bary[:, 0:1] + v1[..., None, :] * bary[:, 1:2]) + v2[..., None, :] * bary[:, 2:3]
    scaling = torch.cat((thickness * torch.ones_like(log_scales[..., 0:1]), torch.exp(log_scales)), -1)
    return points, scaling, quaternions, q_abs


def _tensors(case: dict, dtype):
    t = lambda k: torch.from_numpy(np.asarray(case[k], F32)).to(dtype)
    faces = torch.from_numpy(case["faces"])
    G = case["bary"].shape[0]
    return t("verts"), faces, t("bary"), t("complex").reshape(len(faces), G, 2), t("log_scales").reshape(len(faces), G, 2), t("thickness"), G


def truth(case: dict, standardize: bool = False, dtype=torch.float64, grads: bool = True) -> dict:
    """The three outputs, ``q_abs``, and (``grads``) the gradients for the case's upstream gradients, by torch's CPU autograd at ``dtype``, as
    numpy arrays of that dtype.  Only faces with every index in range."""
    verts, faces, bary, z, s, thickness, G = _tensors(case, dtype)
    N = len(faces) * G
    verts.requires_grad_(grads), z.requires_grad_(grads), s.requires_grad_(grads)
    points, scaling, quats, q_abs = face_forward(verts[faces], bary, z, s, thickness, standardize)
    out = dict(points=points.reshape(N, 3), scaling=scaling.reshape(N, 3), quaternions=quats.reshape(N, 4), q_abs=q_abs.reshape(N, 4))
    if grads:
        loss = sum((out[name] * torch.from_numpy(case["grad_" + name]).to(dtype)).sum() for name in OUTPUTS)
        loss.backward()
        out.update(grad_verts=verts.grad, grad_complex=z.grad.reshape(N, 2), grad_log_scales=s.grad.reshape(N, 2))
    return {k: v.detach().numpy() for k, v in out.items()}


def near_ties(q_abs: np.ndarray, what: str = "") -> np.ndarray:
    """``[N]`` bool: the rows whose two largest ``q_abs`` are within ``TIE``; asserts that they are at most 1 % of the rows."""
    top = np.sort(np.asarray(q_abs, np.float64), axis=1)
    tie = top[:, 3] - top[:, 2] < TIE
    assert tie.sum() <= 0.01 * len(tie), f"{what}: {int(tie.sum())} of {len(tie)} rows are near ties: move the seed"
    return tie


# ---- the scales ---------------------------------------------------------------------------------------------------------------------------

def output_scales(case: dict) -> dict:
    v = np.asarray(case["verts"], np.float64)[case["faces"]]                       # [F, 3, 3]
    b = np.asarray(case["bary"], np.float64)                                       # [G, 3]
    points = (np.abs(v[:, None, :, :] * b[None, :, :, None])).sum(2).reshape(-1, 3)
    scaling = np.concatenate((np.full((len(case["complex"]), 1), abs(float(case["thickness"]))), np.exp(np.asarray(case["log_scales"], np.float64))), 1)
    return dict(points=points, scaling=scaling, quaternions=np.ones((len(case["complex"]), 4)))


def gradient_scales(case: dict, standardize: bool = False) -> dict:
    """``sum |J| |g|`` per element of the three gradients, in float64 (the module docstring)."""
    verts, faces, bary, z, s, thickness, G = _tensors(case, torch.float64)
    F = len(faces)
    g = torch.cat([torch.from_numpy(case["grad_" + name]).to(torch.float64).reshape(F, G, -1) for name in OUTPUTS], -1).abs()   # [F, G, 10]

    def outputs(corners, zz, ss):
        return torch.cat(face_forward(corners, bary, zz, ss, thickness, standardize, complex_is_unit=True)[:3], -1)             # [G, 10], of the unit z

    length = torch.sqrt((z * z).sum(-1, keepdim=True))
    zu = z / length
    J = torch.func.vmap(torch.func.jacrev(outputs, argnums=(0, 1, 2)))(verts[faces], zu, s)
    per_corner = (J[0].abs() * g[..., None, None]).sum((1, 2))                                                                 # [F, 3, 3]
    # the vertices: c = a x b enters through two cross products, b x g_c and g_c x a, whose products cancel for every displacement of a
    # vertex that leaves the normal alone; their absolute products are terms of the element (as in meshattrs_cases.faces_gradient_scale)
    corners = verts[faces]
    a, b = corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0]
    c = torch.linalg.cross(a, b).requires_grad_(True)
    signed = torch.cat([torch.from_numpy(case["grad_" + name]).to(torch.float64).reshape(F, G, -1) for name in OUTPUTS], -1)
    through_c = torch.cat(face_forward(corners, bary, z, s, thickness, standardize, c=c)[:3], -1)
    g_c, = torch.autograd.grad((through_c * signed).sum(), c)
    cross_abs = lambda p, q: (torch.stack((p[:, 1] * q[:, 2], p[:, 2] * q[:, 0], p[:, 0] * q[:, 1]), 1).abs()
                              + torch.stack((p[:, 2] * q[:, 1], p[:, 0] * q[:, 2], p[:, 1] * q[:, 0]), 1).abs())
    g_a, g_b = cross_abs(b, g_c), cross_abs(g_c, a)
    per_corner = per_corner + torch.stack((g_a + g_b, g_a, g_b), 1)
    grad_verts = np.zeros((len(verts), 3))
    np.add.at(grad_verts, faces.numpy().reshape(-1), per_corner.numpy().reshape(-1, 3))
    # the complex numbers: the absolute chain through z = complex / |complex|, whose backward is gz_b / |c| - z_b (gz . z) / |c|: two terms
    # that cancel along the radius, so the element's scale is sum_a (delta_ab + |z_a| |z_b|) / |c| x sum_o |dq_o / dz_a| |g_o|
    through_z = (J[1].abs() * g[..., None, None]).sum((1, 2))                                                                  # [F, G, 2]
    dz = (torch.eye(2, dtype=torch.float64) + (zu[..., :, None] * zu[..., None, :]).abs()) / length[..., None]                 # [F, G, a, b]
    return dict(grad_verts=grad_verts, grad_complex=(dz * through_z[..., :, None]).sum(-2).numpy().reshape(-1, 2),
                grad_log_scales=(J[2].abs() * g[..., None, None]).sum((1, 2)).numpy().reshape(-1, 2))


def ratio(got, want, scale, keep=None) -> float:
    """The largest ``|got - want| / (2^-24 scale)`` over the kept elements; an element of scale 0 must be exact."""
    got, want, scale = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(scale, np.float64)
    keep = np.ones(got.shape, bool) if keep is None else np.broadcast_to(keep, got.shape)
    err = np.abs(got - want)
    assert np.all(err[keep & (scale == 0)] == 0)
    live = keep & (scale > 0)
    return float((err[live] / (2.0 ** -24 * scale[live])).max()) if live.any() else 0.0


def ratios(case: dict, got: dict, standardize: bool = False, want: dict = None, what: str = "") -> dict:
    """Every tensor of ``got`` (outputs and gradients by name) against the truth, as ratios to ``2^-24 x scale``; the near-tie rows of the
    quaternions go through ``quaternion_to_matrix`` (key ``"matrices"``, in units of ``2^-24``) and are left out of the gradients, as
    are the vertices of their faces."""
    want = truth(case, standardize) if want is None else want
    tie = near_ties(want["q_abs"], what)
    G = case["bary"].shape[0]
    out_scale, out = output_scales(case), {}
    for name in OUTPUTS:
        if name in got:
            keep = ~tie[:, None] if name == "quaternions" else None
            out[name] = ratio(got[name], want[name], out_scale[name], keep)
    if "quaternions" in got and tie.any():
        out["matrices"] = ratio(quaternion_to_matrix(got["quaternions"][tie]), quaternion_to_matrix(want["quaternions"][tie]), np.ones((int(tie.sum()), 9)))
    if any(name in got for name in GRADS):
        scale = gradient_scales(case, standardize)
        tie_faces = tie.reshape(-1, G).any(1)
        tie_verts = np.zeros(len(case["verts"]), bool)
        tie_verts[case["faces"][tie_faces].reshape(-1)] = True
        keeps = dict(grad_verts=~tie_verts[:, None], grad_complex=~tie[:, None], grad_log_scales=None)
        for name in GRADS:
            if name in got:
                out[name] = ratio(got[name], want[name], scale[name], keeps[name])
    return out


# ---- the fixtures and the bars --------------------------------------------------------------------------------------------------------

def fixtures() -> dict:
    """name -> the arrays of ``tests/golden/bound/ref_<name>.npz``."""
    out = {}
    for path in sorted(glob.glob(os.path.join(FIXTURES, "ref_*.npz"))):
        with np.load(path) as z:
            out[os.path.basename(path)[4:-4]] = {k: z[k] for k in z.files}
    return out


def fixture_case(fx: dict) -> dict:
    return {k: fx[k] for k in ("verts", "faces", "bary", "complex", "log_scales", "thickness", "grad_points", "grad_scaling", "grad_quaternions")}


RECORDED = dict(points=2.222, scaling=1.004, quaternions=2.472, grad_verts=3.379, grad_complex=5.753, grad_log_scales=1.712)   # the docstring's
_bars = {}


def reference_ratios() -> dict:
    """Per tensor, the largest ratio the reference's own fp32 result reaches on the fixtures."""
    worst = {}
    for name, fx in fixtures().items():
        got = {k[4:]: fx[k] for k in fx if k.startswith("ref.")}
        for k, v in ratios(fixture_case(fx), got, what=name).items():
            worst[k] = max(worst.get(k, 0.0), v)
    return worst


def bars() -> dict:
    """Per tensor, 4 x :func:`reference_ratios`; ``"matrices"``: 4 x the quaternions' bar (the module docstring)."""
    if not _bars:
        worst = reference_ratios()
        _bars.update({k: 4.0 * worst[k] for k in OUTPUTS + GRADS})
        _bars["matrices"] = 4.0 * _bars["quaternions"]
    return _bars


def check(case: dict, got: dict, standardize: bool = False, what: str = "", want: dict = None) -> dict:
    """Asserts every tensor of ``got`` within the bars; returns the ratios."""
    found = ratios(case, got, standardize, want, what)
    for k, v in found.items():
        assert v <= bars()[k], f"{what}: {k} at {v:.3g} x 2^-24 x scale, the bar is {bars()[k]:.3g}"
    return found
