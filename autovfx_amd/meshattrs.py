"""Face areas and normals, and face-attribute interpolation, on the GPU: pytorch3d's ``_C.face_areas_normals_forward`` / ``_backward`` and
``_C.interpolate_face_attributes_forward`` / ``_backward``.

The first pair sits under ``Meshes.faces_normals_packed()``: ``SuGaR.quaternions`` (``sugar/sugar_scene/sugar_model.py:425-452``) calls it
several times per iteration of the refinement stage and differentiates it into the vertices, ``SuGaR.get_normals`` (``:835``) and
``sugar_extractors/refined_mesh.py:134`` call it too.  The second pair sits under every pytorch3d shader and texture sampler: the texture
extraction (``refined_mesh.py:194-197``, ``sugar_model.py:2595-2596``) and ``metrics.py:274-290`` run it on the fragments
``autovfx_amd.meshraster`` returns.  A pytorch3d built against torch-ROCm has neither on the GPU.  The four functions below run the HIP
kernels of ``gsr_meshattrs.hip`` (C ABI ``gsr_face_areas_normals``, ``gsr_face_areas_normals_backward``, ``gsr_interp_face_attrs``,
``gsr_interp_face_attrs_backward``) behind pytorch3d's argument lists; the ``drop_in_*`` are what ``autovfx_amd.install()`` puts in place of
pytorch3d's operators; the ``*_host`` functions restate the contract in numpy.  pytorch3d's Python autograd classes stay pytorch3d's: they
look the operators up on ``_C`` at call time.

The contract is pytorch3d's published kernels as recalled, pinned here; the tests hold the code to this text.  Every
operation is an fp32 one in the order written, nothing contracted into a fused multiply-add; division and ``sqrt`` are the correctly rounded
ones; ``max`` is C's ``fmaxf`` (a NaN operand loses).

**Face areas and normals, forward.**  ``verts [V, 3]`` float32, ``faces [F, 3]`` int64 -> ``areas [F]``, ``normals [F, 3]``.  Per face with
vertices ``v0, v1, v2``::

    a = v1 - v0                      b = v2 - v0
    c = (a.y * b.z - a.z * b.y,  a.z * b.x - a.x * b.z,  a.x * b.y - a.y * b.x)
    n = sqrt((c.x * c.x + c.y * c.y) + c.z * c.z)
    area = n / 2                     normal = c / max(n, 1e-6)

A face with a vertex index outside ``[0, V)`` is outside pytorch3d's contract; here it gets area 0 and normal 0 and reads nothing
(difference 1).

**Face areas and normals, backward.**  ``grad_areas [F]``, ``grad_normals [F, 3]`` -> ``grad_verts [V, 3]``: the derivative of exactly that
forward.  Per face, with ``a, b, c, n`` as above, ``ga = grad_areas[f]``, ``g = grad_normals[f]``, componentwise over x, y, z::

    h = (ga * c) / (2 * n)           if n > 0, else 0                         (through the area)
    m = c / n;  dot = (m.x * g.x + m.y * g.y) + m.z * g.z
    q = (g - m * dot) / n            if n >= 1e-6                             (through the normal: the projection off m, over n)
    q = g / 1e-6                     otherwise: below the clamp the forward is c / 1e-6, linear in c
    g_c = h + q
    g_a = (b.y * g_c.z - b.z * g_c.y,  b.z * g_c.x - b.x * g_c.z,  b.x * g_c.y - b.y * g_c.x)          (b x g_c)
    g_b = (g_c.y * a.z - g_c.z * a.y,  g_c.z * a.x - g_c.x * a.z,  g_c.x * a.y - g_c.y * a.x)          (g_c x a)
    the face adds  -(g_a + g_b)  to v0,  g_a  to v1,  g_b  to v2

``grad_verts`` is zeroed and the faces' contributions are added with float atomics: each term is fixed by the text above, the order of a
vertex's sum is not, so a vertex in one face gets that face's bits, a vertex in no face exactly 0, and a vertex in several faces a sum that
may differ in its last bits between runs.  A NaN ``n`` takes the ``otherwise`` branches, as ``max(NaN, 1e-6) = 1e-6`` does in the forward.
Faces with an out-of-range index contribute nothing.  How pytorch3d's own backward treats ``n < 1e-6`` is not known here: it may differ
from the linear branch above (difference 2).

**Interpolation, forward.**  ``pix_to_face`` int64 of any shape S -- ``[P]``, as pytorch3d's ``interpolate_face_attributes`` flattens the
fragments before it calls the operator, or ``[N, H, W, K]`` --, ``barycentric_coords`` S + ``[3]``, ``face_attributes [F, 3, D]`` -> S + ``[D]``.
Per slot p with ``f = pix_to_face[p]``::

    out[p, d] = (bary[p, 0] * attrs[f, 0, d] + bary[p, 1] * attrs[f, 1, d]) + bary[p, 2] * attrs[f, 2, d]

and a row of zeros when ``f < 0``.  An index ``>= F`` is outside pytorch3d's contract; it is treated as empty (difference 3).

**Interpolation, backward.**  ``grad_pix_attrs`` S + ``[D]`` -> ``grad_barycentric_coords`` S + ``[3]``, ``grad_face_attributes [F, 3, D]``::

    grad_bary[p, k] = (((go[p, 0] * attrs[f, k, 0]) + go[p, 1] * attrs[f, k, 1]) + go[p, 2] * attrs[f, k, 2]) + ...     d ascending
    grad_attrs[f, k, d] += bary[p, k] * go[p, d]                                                   over the slots p that hold f

``grad_bary`` is zero for empty slots, uses no atomics and is fully specified.  ``grad_attrs`` is zeroed first and summed with float
atomics: the terms are fixed, the order is free, as for ``grad_verts``.

All four take at most 2^31 - 1 vertices, faces and slots, and ``1 <= D <= 65536``.
"""
from __future__ import annotations

from typing import Callable, Optional, Tuple

import numpy as np
import torch

from . import _mesh_host, _takes

MAX_COUNT = (1 << 31) - 1
MAX_D = 65536
_F = np.float32


# ---- which calls the kernels take -----------------------------------------------------------------------------------------------------

ALLOCATES = "the call allocates its outputs; such a call is left to the original"
_f32, _i64 = torch.float32, torch.int64


def _why_not_faces(verts, faces, grad_areas=None, grad_normals=None, backward: bool = False) -> Optional[str]:
    """None when the kernels take the call, else the reason they do not."""
    why = _takes.mesh(verts, faces)
    if why is None and backward:
        F = faces.shape[0]
        why = (_takes.tensors((("grad_areas", grad_areas, _f32), ("grad_normals", grad_normals, _f32)), like=verts)
               or _takes.shaped("grad_areas", grad_areas, "[F]", tuple(grad_areas.shape) == (F,))
               or _takes.shaped("grad_normals", grad_normals, "[F, 3]", tuple(grad_normals.shape) == (F, 3)))
    if why is None and (verts.shape[0] > MAX_COUNT or faces.shape[0] > MAX_COUNT):
        why = f"{verts.shape[0]} vertices, {faces.shape[0]} faces: at most 2^31 - 1 of each"
    return why or _takes.capturing(ALLOCATES)


def _why_not_interp(pix_to_face, bary, attrs, grad_out=None, backward: bool = False) -> Optional[str]:
    """None when the kernels take the call, else the reason they do not."""
    why = _takes.tensors((("face_attributes", attrs, _f32), ("pix_to_face", pix_to_face, _i64), ("barycentric_coords", bary, _f32))
                         + ((("grad_pix_attrs", grad_out, _f32),) if backward else ()))
    if why is None:
        why = _takes.shaped("face_attributes", attrs, "[F, 3, D] with D >= 1", attrs.dim() == 3 and attrs.shape[1] == 3 and attrs.shape[2] >= 1)
    if why is None and attrs.shape[2] > MAX_D:
        why = f"D = {attrs.shape[2]}: at most {MAX_D}"
    if why is None:
        S = tuple(pix_to_face.shape)
        why = (_takes.shaped("pix_to_face", pix_to_face, "[P] or [N, H, W, K]", len(S) >= 1)
               or _takes.shaped("barycentric_coords", bary, "pix_to_face's shape + [3]", tuple(bary.shape) == S + (3,))
               or (_takes.shaped("grad_pix_attrs", grad_out, "pix_to_face's shape + [D]", tuple(grad_out.shape) == S + (attrs.shape[2],))
                   if backward else None))
    if why is None and (pix_to_face.numel() > MAX_COUNT or attrs.shape[0] > MAX_COUNT):
        why = f"{pix_to_face.numel()} slots, {attrs.shape[0]} faces: at most 2^31 - 1 of each"
    return why or _takes.capturing(ALLOCATES)


def face_areas_normals_takes(verts, faces) -> bool:
    """Whether :func:`face_areas_normals_forward` runs this call: a CUDA float32 ``[V, 3]`` and an int64 ``[F, 3]`` on the same device, not
    under graph capture."""
    return _why_not_faces(verts, faces) is None


def face_areas_normals_backward_takes(grad_areas, grad_normals, verts, faces) -> bool:
    """As :func:`face_areas_normals_takes`, with CUDA float32 ``grad_areas [F]`` and ``grad_normals [F, 3]`` on the same device."""
    return _why_not_faces(verts, faces, grad_areas, grad_normals, backward=True) is None


def interpolate_face_attributes_takes(pix_to_face, barycentric_coords, face_attributes) -> bool:
    """Whether :func:`interpolate_face_attributes_forward` runs this call: an int64 ``pix_to_face`` of shape S (``[P]`` or ``[N, H, W, K]``),
    CUDA float32 barycentrics S + ``[3]`` and attributes ``[F, 3, D]`` with ``1 <= D <= 65536`` on one device, not under graph capture."""
    return _why_not_interp(pix_to_face, barycentric_coords, face_attributes) is None


def interpolate_face_attributes_backward_takes(pix_to_face, barycentric_coords, face_attributes, grad_pix_attrs) -> bool:
    """As :func:`interpolate_face_attributes_takes`, with a CUDA float32 ``grad_pix_attrs`` S + ``[D]`` on the same device."""
    return _why_not_interp(pix_to_face, barycentric_coords, face_attributes, grad_pix_attrs, backward=True) is None


# ---- the calls ------------------------------------------------------------------------------------------------------------------------

def _faces_forward(verts, faces):
    from . import _lib

    v, f = _takes.cs(verts, faces)
    V, F = int(v.shape[0]), int(f.shape[0])
    areas = torch.empty((F,), dtype=torch.float32, device=v.device)
    normals = torch.empty((F, 3), dtype=torch.float32, device=v.device)
    with torch.cuda.device(v.device):
        _lib.call("gsr_face_areas_normals", V, F, _lib.ptr(v), _lib.ptr(f), _lib.ptr(areas), _lib.ptr(normals), device=v.device)
    return areas, normals


def _faces_backward(grad_areas, grad_normals, verts, faces):
    from . import _lib

    v, f, ga, gn = _takes.cs(verts, faces, grad_areas, grad_normals)
    V, F = int(v.shape[0]), int(f.shape[0])
    grad_verts = torch.empty((V, 3), dtype=torch.float32, device=v.device)
    with torch.cuda.device(v.device):
        _lib.call("gsr_face_areas_normals_backward", V, F, _lib.ptr(v), _lib.ptr(f), _lib.ptr(ga), _lib.ptr(gn), _lib.ptr(grad_verts),
                  device=v.device)
    return grad_verts


def _interp_forward(pix_to_face, bary, attrs):
    from . import _lib

    p, w, a = _takes.cs(pix_to_face, bary, attrs)
    P, F, D = int(p.numel()), int(a.shape[0]), int(a.shape[2])
    out = torch.empty(tuple(p.shape) + (D,), dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        _lib.call("gsr_interp_face_attrs", P, F, D, _lib.ptr(p), _lib.ptr(w), _lib.ptr(a), _lib.ptr(out), device=a.device)
    return out


def _interp_backward(pix_to_face, bary, attrs, grad_out):
    from . import _lib

    p, w, a, g = _takes.cs(pix_to_face, bary, attrs, grad_out)
    P, F, D = int(p.numel()), int(a.shape[0]), int(a.shape[2])
    grad_bary = torch.empty(tuple(p.shape) + (3,), dtype=torch.float32, device=a.device)
    grad_attrs = torch.empty((F, 3, D), dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        _lib.call("gsr_interp_face_attrs_backward", P, F, D, _lib.ptr(p), _lib.ptr(w), _lib.ptr(a), _lib.ptr(g), _lib.ptr(grad_bary),
                  _lib.ptr(grad_attrs), device=a.device)
    return grad_bary, grad_attrs


def face_areas_normals_forward(verts, faces) -> Tuple[torch.Tensor, torch.Tensor]:
    """``pytorch3d._C.face_areas_normals_forward`` -> ``(areas [F], normals [F, 3])`` by the module's contract, queued on the current stream.
    Non-contiguous inputs are copied.  A call :func:`face_areas_normals_takes` rejects raises ``ValueError`` with the reason."""
    _takes.refuse("face_areas_normals_forward", _why_not_faces(verts, faces))
    return _faces_forward(verts, faces)


def face_areas_normals_backward(grad_areas, grad_normals, verts, faces) -> torch.Tensor:
    """``pytorch3d._C.face_areas_normals_backward`` -> ``grad_verts [V, 3]`` by the module's contract (float atomics: the order of a vertex's
    sum is free).  A call :func:`face_areas_normals_backward_takes` rejects raises ``ValueError`` with the reason."""
    _takes.refuse("face_areas_normals_backward", _why_not_faces(verts, faces, grad_areas, grad_normals, backward=True))
    return _faces_backward(grad_areas, grad_normals, verts, faces)


def interpolate_face_attributes_forward(pix_to_face, barycentric_coords, face_attributes) -> torch.Tensor:
    """``pytorch3d._C.interpolate_face_attributes_forward`` -> ``pix_attrs``, ``pix_to_face``'s shape + ``[D]``, by the module's contract.  A call
    :func:`interpolate_face_attributes_takes` rejects raises ``ValueError`` with the reason."""
    _takes.refuse("interpolate_face_attributes_forward", _why_not_interp(pix_to_face, barycentric_coords, face_attributes))
    return _interp_forward(pix_to_face, barycentric_coords, face_attributes)


def interpolate_face_attributes_backward(pix_to_face, barycentric_coords, face_attributes, grad_pix_attrs) -> Tuple[torch.Tensor, torch.Tensor]:
    """``pytorch3d._C.interpolate_face_attributes_backward`` -> ``(grad_barycentric_coords, grad_face_attributes [F, 3, D])``
    by the module's contract (float atomics into the second).  A call :func:`interpolate_face_attributes_backward_takes` rejects raises
    ``ValueError`` with the reason."""
    _takes.refuse("interpolate_face_attributes_backward", _why_not_interp(pix_to_face, barycentric_coords, face_attributes, grad_pix_attrs, backward=True))
    return _interp_backward(pix_to_face, barycentric_coords, face_attributes, grad_pix_attrs)


def _drop_in(name: str, original: Callable, why_not: Callable, taken: Callable) -> Callable:
    """An operator named ``name`` that runs ``taken`` for the calls ``why_not`` lets through and ``original`` with the caller's arguments for
    every other."""
    def operator(*args, **kwargs):
        if not kwargs and why_not(*args) is None:     # (pytorch3d's Python calls positionally; a call by keyword is the original's)
            return taken(*args)
        return original(*args, **kwargs)

    return _takes.dressed(operator, name, original, f"pytorch3d._C.{name}", "meshattrs")


def _guarded(why_not: Callable, count: int, **fixed) -> Callable:
    """``why_not`` for exactly ``count`` positional arguments; any other call shape is the original's."""
    def check(*args):
        return why_not(*args, **fixed) if len(args) == count else "another argument list"

    return check


def drop_in_face_areas_normals_forward(original: Callable) -> Callable:
    """A ``face_areas_normals_forward`` that runs the kernel for the calls :func:`face_areas_normals_takes` accepts and ``original``
    (pytorch3d's operator) for every other: CPU tensors, other dtypes, ranks or devices, graph capture."""
    return _drop_in("face_areas_normals_forward", original, _guarded(_why_not_faces, 2), _faces_forward)


def drop_in_face_areas_normals_backward(original: Callable) -> Callable:
    """As :func:`drop_in_face_areas_normals_forward`, for ``face_areas_normals_backward(grad_areas, grad_normals, verts, faces)``."""
    return _drop_in("face_areas_normals_backward", original,
                    _guarded(lambda ga, gn, v, f: _why_not_faces(v, f, ga, gn, backward=True), 4), _faces_backward)


def drop_in_interpolate_face_attributes_forward(original: Callable) -> Callable:
    """An ``interpolate_face_attributes_forward`` that runs the kernel for the calls :func:`interpolate_face_attributes_takes` accepts and
    ``original`` for every other."""
    return _drop_in("interpolate_face_attributes_forward", original, _guarded(_why_not_interp, 3), _interp_forward)


def drop_in_interpolate_face_attributes_backward(original: Callable) -> Callable:
    """As :func:`drop_in_interpolate_face_attributes_forward`, for the backward's four arguments."""
    return _drop_in("interpolate_face_attributes_backward", original, _guarded(_why_not_interp, 4, backward=True), _interp_backward)


# ---- the contract in numpy ------------------------------------------------------------------------------------------------------------

def face_areas_normals_host(verts, faces):
    """The forward of the module's contract in numpy, every operation an fp32 elementwise one in the contract's order.  Returns
    ``(areas [F], normals [F, 3])``."""
    verts, faces = _mesh_host.verts_faces(verts, faces)
    valid, v0, v1, v2 = _mesh_host.face_corners(verts, faces)
    with np.errstate(all="ignore"):
        _a, _b, c, n = _mesh_host.face_cross(v0, v1, v2)
        areas = n / _F(2.0)
        normals = c / np.fmax(n, _mesh_host.FACE_NORMAL_EPS)[:, None]
    return np.where(valid, areas, _F(0.0)).astype(_F), np.where(valid[:, None], normals, _F(0.0)).astype(_F)


def face_areas_normals_backward_host(grad_areas, grad_normals, verts, faces):
    """The backward of the module's contract in numpy.  Returns ``(grad_verts [V, 3], contributions [F, 3, 3])``: ``contributions[f, i]`` is
    what face f adds to its vertex i (zeros for a face with an out-of-range index), each an fp32 value fixed by the contract;
    ``grad_verts`` is their fp32 sum in face order, one of the orders the kernel's atomics may take."""
    verts, faces = _mesh_host.verts_faces(verts, faces)
    F = faces.shape[0]
    ga = np.asarray(grad_areas, dtype=_F).reshape(F)
    g = np.asarray(grad_normals, dtype=_F).reshape(F, 3)
    valid, v0, v1, v2 = _mesh_host.face_corners(verts, faces)
    with np.errstate(all="ignore"):
        a, b, c, n = _mesh_host.face_cross(v0, v1, v2)
        h = np.where((n > _F(0.0))[:, None], (ga[:, None] * c) / (_F(2.0) * n)[:, None], _F(0.0))
        gc = (h + _mesh_host.normal_backward(c, n, g)).astype(_F)
        g_a, g_b = _mesh_host.cross(b, gc), _mesh_host.cross(gc, a)
        contributions = np.stack((-(g_a + g_b), g_a, g_b), axis=1).astype(_F)
    contributions[~valid] = _F(0.0)
    grad_verts = np.zeros((verts.shape[0], 3), _F)
    keep = np.nonzero(valid)[0]
    with np.errstate(all="ignore"):
        np.add.at(grad_verts, faces[keep].reshape(-1), contributions[keep].reshape(-1, 3))
    return grad_verts, contributions


def _slots(pix_to_face, bary, attrs):
    attrs = np.ascontiguousarray(np.asarray(attrs, dtype=_F))
    pix = np.asarray(pix_to_face, dtype=np.int64)
    w = np.asarray(bary, dtype=_F).reshape(-1, 3)
    flat = pix.reshape(-1)
    held = (flat >= 0) & (flat < attrs.shape[0])
    return pix.shape, flat, held, w, attrs


def interp_face_attrs_host(pix_to_face, bary, attrs):
    """The interpolation of the module's contract in numpy: ``pix_to_face`` of any shape S, ``bary`` S + [3], ``attrs [F, 3, D]`` ->
    S + [D]."""
    shape, flat, held, w, attrs = _slots(pix_to_face, bary, attrs)
    D = attrs.shape[2]
    out = np.zeros((flat.shape[0], D), _F)
    if held.any():
        a = attrs[flat[held]]
        wk = w[held]
        with np.errstate(all="ignore"):
            out[held] = (wk[:, 0:1] * a[:, 0] + wk[:, 1:2] * a[:, 1]) + wk[:, 2:3] * a[:, 2]
    return out.reshape(shape + (D,))


def interp_face_attrs_backward_host(pix_to_face, bary, attrs, grad_out):
    """The interpolation's backward in numpy.  Returns ``(grad_bary S + [3], grad_attrs [F, 3, D])``; ``grad_attrs`` is the fp32 sum of the
    terms ``bary[p, k] * grad_out[p, d]`` in slot order, one of the orders the kernel's atomics may take."""
    shape, flat, held, w, attrs = _slots(pix_to_face, bary, attrs)
    D = attrs.shape[2]
    go = np.asarray(grad_out, dtype=_F).reshape(-1, D)
    grad_bary = np.zeros((flat.shape[0], 3), _F)
    grad_attrs = np.zeros(attrs.shape, _F)
    if held.any():
        a, g, wk = attrs[flat[held]], go[held], w[held]
        with np.errstate(all="ignore"):
            acc = g[:, None, 0] * a[:, :, 0]
            for d in range(1, D):
                acc = acc + g[:, None, d] * a[:, :, d]
            grad_bary[held] = acc
            np.add.at(grad_attrs, flat[held], wk[:, :, None] * g[:, None, :])
    return grad_bary.reshape(shape + (3,)), grad_attrs
