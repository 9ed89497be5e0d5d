"""The Gaussians SuGaR binds to a surface mesh, on the GPU: ``SuGaR.points``, ``SuGaR.scaling`` and ``SuGaR.quaternions`` with
``binded_to_surface_mesh`` set (``sugar/sugar_scene/sugar_model.py:376-391``, ``:408-423``, ``:425-452``).

The refinement (``sugar_trainers/refine.py:564-576``, ``:823-830``) reads each of the three once per ``render_image_gaussian_rasterizer``
call (``sugar_model.py:2006``, ``:2082``, ``:2085``) and differentiates them into the vertices, ``_scales`` and ``_quaternions``.  The
reference computes them with a chain of small torch kernels -- face normals, three ``F.normalize`` and a cross product, a 2-D rotation, a
``cat`` into ``[N, 3, 3]``, pytorch3d's ``matrix_to_quaternion`` (two ``stack``s, a masked ``sqrt``, an ``argmax`` and a boolean-mask index,
which is a ``nonzero`` and so a host synchronisation), a last ``normalize`` -- although everything is local to one face.
:func:`bound_gaussians` is one autograd node over the two kernels of ``gsr_bound.hip`` (C ABI ``gsr_bound_gaussians``,
``gsr_bound_gaussians_backward``): one lane per face, the face's frame computed once for its ``G`` Gaussians, nothing of size ``[N, .]``
kept between forward and backward, no host synchronisation.  ``drop_in_points``, ``drop_in_scaling`` and ``drop_in_quaternions`` are what
``autovfx_amd.install()`` puts in place of the three property getters; ``bound_gaussians_host`` and ``bound_gaussians_backward_host``
restate the contract in numpy.

The contract; the tests hold the code to this text.  Every operation is an fp32 one in the order written, nothing
contracted into a fused multiply-add; division and ``sqrt`` are the correctly rounded ones; ``max`` is C's ``fmaxf`` (a NaN operand loses);
``exp`` is the device library's ``expf`` on the GPU and numpy's on the host, the one operation whose bits may differ between the two
(as in 7g and 7h).  ``|w|`` of a 3-vector is ``sqrt((w.x w.x + w.y w.y) + w.z w.z)``, ``u x w`` is
``(u.y w.z - u.z w.y, u.z w.x - u.x w.z, u.x w.y - u.y w.x)``, ``u . w`` is ``(u.x w.x + u.y w.y) + u.z w.z``, and ``unit(w) = w / max(|w|, 1e-12)``
(``F.normalize``).

**Forward.**  ``verts [V, 3]`` float32, ``faces [F, 3]`` int64, ``bary [G, 3]``, ``complex [F G, 2]`` (the raw ``_quaternions``),
``log_scales [F G, 2]`` (the raw ``_scales``), ``thickness`` (one float on the device) -> ``points [F G, 3]``, ``scaling [F G, 3]``,
``quaternions [F G, 4]`` (w, x, y, z); Gaussian ``g`` of face ``f`` is row ``f G + g``.  Per face with vertices ``v0, v1, v2``::

    a = v1 - v0        b = v2 - v0        c = a x b        n = |c|        normal = c / max(n, 1e-6)                      (exactly 7j)
    R_0 = unit(normal)          base_R_1 = unit(v0 - v1)          base_R_2 = unit(R_0 x base_R_1)

and per Gaussian of it, with ``(p, q) = complex[f G + g]``, ``(b0, b1, b2) = bary[g]``, ``(s0, s1) = log_scales[f G + g]``::

    z = (p, q) / max(sqrt(p p + q q), 1e-12)
    R_1 = z.re base_R_1 + z.im base_R_2                R_2 = (-z.im) base_R_1 + z.re base_R_2               (componentwise)
    m = [R_0 | R_1 | R_2]                              (m_ij: component i of column j)
    pre = (((1 + m00) + m11) + m22,  ((1 + m00) - m11) - m22,  ((1 - m00) + m11) - m22,  ((1 - m00) - m11) + m22)
    q_abs[j] = sqrt(pre[j]) if pre[j] > 0 else 0       (the zero-subgradient square root)
    k = the lowest index among the largest q_abs       (argmax, ties to the lowest index; a scan upwards with ``>``)
    row 0 = (q_abs[0]^2, m21 - m12, m02 - m20, m10 - m01)        row 1 = (m21 - m12, q_abs[1]^2, m10 + m01, m02 + m20)
    row 2 = (m02 - m20, m10 + m01, q_abs[2]^2, m12 + m21)        row 3 = (m10 - m01, m20 + m02, m21 + m12, q_abs[3]^2)
    u = row k / (2 max(q_abs[k], 0.1))                 (matrix_to_quaternion of pytorch3d 0.7.4; q^2 is q q)
    u = -u if standardize and u[0] < 0                 (standardize_quaternion of later releases)
    quaternion = u / max(sqrt(((u0 u0 + u1 u1) + u2 u2) + u3 u3), 1e-12)
    point = (v0 b0 + v1 b1) + v2 b2                    scaling = (thickness, exp(s0), exp(s1))

The four ``pre`` add up to 4, so for finite inputs the candidate taken has ``q_abs >= 1``: the floor decides nothing for it.

**Backward.**  ``grad_points``, ``grad_scaling``, ``grad_quaternions`` (any may be absent) -> ``grad_verts [V, 3]``, ``grad_complex [F G, 2]``,
``grad_log_scales [F G, 2]``: the derivative of exactly that text, the forward recomputed.  Every clamp takes the branch autograd takes; with
``unit_backward(x, g)`` for ``y = x / max(|x|, 1e-12)``, sums from the left::

    D = max(|x|, 1e-12)        gx = g / D        and, if |x| >= 1e-12:        gx = gx + x ((-((g . x) / (D D))) / |x|)

the steps are, per Gaussian with ``gq = grad_quaternions[i]`` (``u`` the row before the flip, ``s`` after it)::

    gs = unit_backward(s, gq)          gu = -gs if flipped else gs          gc = gu / d        with d = 2 max(q_abs[k], 0.1)
    gd = -((((gu0 u0 + gu1 u1) + gu2 u2) + gu3 u3) / d)
    gqk = (2 q_abs[k]) gc[k]           and, if q_abs[k] > 0.1:        gqk = gqk + 2 gd
    gpre = gqk / (2 q_abs[k]) if pre[k] > 0 else 0
    g_m00, g_m11, g_m22 = +-gpre with the signs of row k's pre;  every other m_ij occurs once in row k, in the entry e that holds its
    sum or difference:  g_mij = gc[e], negated where m_ij is subtracted.  The rows not taken get nothing.
    g_R0, g_R1, g_R2 = the columns of g_m
    gz = (g_R1 . base_R_1 + g_R2 . base_R_2,  g_R1 . base_R_2 - g_R2 . base_R_1)        grad_complex[i] = unit_backward((p, q), gz)
    G0 += g_R0         G1 += z.re g_R1 + (-z.im) g_R2         G2 += z.im g_R1 + z.re g_R2          (from +0, g ascending)

then once per face::

    gx = unit_backward(R_0 x base_R_1, G2)        G0 = G0 + base_R_1 x gx        G1 = G1 + gx x R_0
    ge = unit_backward(v0 - v1, G1)               gn = unit_backward(normal, G0)
    g_c = (gn - m (m . gn)) / n  with m = c / n   if n >= 1e-6,  else  gn / 1e-6                                          (7j)
    g_a = b x g_c              g_b = g_c x a
    the face adds  (P0 + ge) + (-(g_a + g_b))  to v0,   (P1 + (-ge)) + g_a  to v1,   P2 + g_b  to v2

with ``P_i`` the sum, from +0 and over g ascending, of ``bary[g][i] grad_points[f G + g]`` (``P_i`` alone when ``grad_quaternions`` is absent, +0
when ``grad_points`` is).  ``grad_log_scales[i] = (grad_scaling[i][1] exp(s0), grad_scaling[i][2] exp(s1))``; the thickness gets no gradient
(the reference's parameter does not require one).  ``grad_complex`` and ``grad_log_scales`` use no atomics and are fully specified.
``grad_verts`` is zeroed and each face's nine terms are added with float atomics: the terms are fixed by the text above, the order of a
vertex's sum is not, as for ``gsr_face_areas_normals_backward`` (7j).

A face with a vertex index outside ``[0, V)`` reads nothing, gets ``points = 0`` and ``quaternions = 0`` and no gradient; ``scaling`` does not
depend on the face.  The reference would raise or read out of bounds there (the stated difference).  At most 2^31 - 1 vertices and
Gaussians, ``1 <= G <= 8``.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence

import numpy as np
import torch

from . import _mesh_host, _takes
from ._mesh_host import cross as _cross, dot as _dot, norm as _norm

MAX_COUNT = (1 << 31) - 1
MAX_G = 8
OUTPUTS = ("points", "scaling", "quaternions")
_F = np.float32
UNIT_EPS = _F(1e-12)
QUAT_FLOOR = _F(0.1)


# ---- which calls the kernels take -----------------------------------------------------------------------------------------------------

def _why_not(verts, faces, bary, complex, log_scales, thickness, want) -> Optional[str]:
    """None when the kernels take the call, else the reason they do not."""
    if not want or any(w not in OUTPUTS for w in want) or len(set(want)) != len(want):
        return f"want must name some of {OUTPUTS}, each once (got {tuple(want)!r})"
    why = (_takes.mesh(verts, faces, "bound_gaussians_host")
           or _takes.tensors(tuple((name, t, torch.float32) for name, t in (("bary", bary), ("complex", complex), ("log_scales", log_scales),
                                                                            ("thickness", thickness))), verts, "bound_gaussians_host")
           or _takes.shaped("bary", bary, "[G, 3] with G >= 1", bary.dim() == 2 and bary.shape[1] == 3 and bary.shape[0] >= 1))
    if why is not None:
        return why
    G, F = int(bary.shape[0]), int(faces.shape[0])
    if G > MAX_G:
        return f"G = {G} Gaussians per face: at most {MAX_G}"
    why = (_takes.shaped("complex", complex, f"[F G, 2] = [{F * G}, 2]", tuple(complex.shape) == (F * G, 2))
           or _takes.shaped("log_scales", log_scales, f"[F G, 2] = [{F * G}, 2]", tuple(log_scales.shape) == (F * G, 2)))
    if why is not None:
        return why
    if thickness.numel() != 1:
        return f"thickness must hold one element (got {list(thickness.shape)})"
    if verts.shape[0] > MAX_COUNT or F * G > MAX_COUNT:
        return f"{verts.shape[0]} vertices, {F * G} Gaussians: at most 2^31 - 1 of each"
    return _takes.capturing("the call allocates its outputs")


class _BoundGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, faces, bary, complex, log_scales, thickness, want, standardize):
        from . import _lib

        v, f, b, z, s, th = _takes.cs(verts, faces, bary, complex, log_scales, thickness)
        th = th.reshape(1)
        V, F, G = int(v.shape[0]), int(f.shape[0]), int(b.shape[0])
        out = {name: torch.empty((F * G, width), dtype=torch.float32, device=v.device) if name in want else None
               for name, width in zip(OUTPUTS, (3, 3, 4))}
        with torch.cuda.device(v.device):
            _lib.call("gsr_bound_gaussians", V, F, G, _lib.ptr(v), _lib.ptr(f), _lib.ptr(b), _lib.ptr(z), _lib.ptr(s), _lib.ptr(th),
                      int(standardize), *(_lib.ptr(out[name]) for name in OUTPUTS), device=v.device)
        ctx.save_for_backward(v, f, b, z, s)
        ctx.standardize = int(standardize)
        ctx.set_materialize_grads(False)
        return tuple(out[name] for name in OUTPUTS)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_points, grad_scaling, grad_quaternions):
        from . import _lib

        v, f, b, z, s = ctx.saved_tensors
        V, F, G = int(v.shape[0]), int(f.shape[0]), int(b.shape[0])
        grads = [None if g is None else _takes.c(g) for g in (grad_points, grad_scaling, grad_quaternions)]
        grad_verts = torch.empty((V, 3), dtype=torch.float32, device=v.device)
        grad_complex = torch.empty((F * G, 2), dtype=torch.float32, device=v.device)
        grad_log_scales = torch.empty((F * G, 2), dtype=torch.float32, device=v.device)
        with torch.cuda.device(v.device):
            _lib.call("gsr_bound_gaussians_backward", V, F, G, _lib.ptr(v), _lib.ptr(f), _lib.ptr(b), _lib.ptr(z), _lib.ptr(s), ctx.standardize,
                      *(_lib.ptr(g) for g in grads), _lib.ptr(grad_verts), _lib.ptr(grad_complex), _lib.ptr(grad_log_scales), device=v.device)
        need = ctx.needs_input_grad
        return (grad_verts if need[0] else None, None, None, grad_complex if need[3] else None, grad_log_scales if need[4] else None,
                None, None, None)


def bound_gaussians(verts, faces, bary, complex, log_scales, thickness, *, want: Sequence[str] = OUTPUTS, standardize: bool = False):
    """The wanted ones of ``points [F G, 3]``, ``scaling [F G, 3]`` and ``quaternions [F G, 4]`` by the module's contract, as a tuple in
    ``want``'s order: one launch on the current stream, one autograd node, differentiable once in ``verts``, ``complex`` and
    ``log_scales`` (one more launch; float atomics into the vertices' gradient: the order of a vertex's sum is free).  ``thickness`` is a
    tensor of one element on the device, read by the kernel.  ``standardize``: negate a quaternion whose real part is negative, as
    ``matrix_to_quaternion`` does from pytorch3d 0.7.5 on.  No host synchronisation.  CPU tensors, other dtypes or shapes, mixed devices,
    ``G > 8`` and graph capture raise ``ValueError`` with the reason."""
    want = tuple(want)
    _takes.refuse("bound_gaussians", _why_not(verts, faces, bary, complex, log_scales, thickness, want))
    out = dict(zip(OUTPUTS, _BoundGaussians.apply(verts, faces, bary, complex, log_scales, thickness, want, bool(standardize))))
    return tuple(out[name] for name in want)


# ---- the three property getters -------------------------------------------------------------------------------------------------------

_PROBE = ((1.0, 0.0, 0.0), (0.0, -0.9899924966004454, 0.1411200080598672), (0.0, -0.1411200080598672, -0.9899924966004454))
"""A turn by -3 rad about x: pytorch3d 0.7.4 answers with candidate 1 and a real part of -0.0707; a standardising release with +0.0707."""


def standardizes(matrix_to_quaternion: Callable) -> bool:
    """Whether this ``matrix_to_quaternion`` ends with ``standardize_quaternion``: one call on one host matrix."""
    q = matrix_to_quaternion(torch.tensor(_PROBE, dtype=torch.float32)[None])
    return bool(float(q.reshape(-1)[0]) > 0.0)


def _why_original(self) -> Optional[str]:
    """Why the reference's getter runs for this model (None: the kernels do), from its flags and its tensors' descriptions alone."""
    if not getattr(self, "binded_to_surface_mesh", False):
        return "the model is not bound to a surface mesh"
    if getattr(self, "editable", False):
        return "editable=True: the scale factor stays the reference's"
    if getattr(self, "scale_activation", None) is not torch.exp:
        return "scale_activation is not torch.exp"
    try:
        bary = self.surface_triangle_bary_coords
        if not (isinstance(bary, torch.Tensor) and bary.dim() == 3 and bary.shape[-1] == 1):
            return "surface_triangle_bary_coords is not [G, 3, 1]"
        return _why_not(self._points, self._surface_mesh_faces, bary[..., 0], self._quaternions, self._scales, self.surface_mesh_thickness, OUTPUTS)
    except AttributeError as e:
        return f"the model lacks {e}"


def _drop_in(name: str, original_fget: Callable) -> Callable:
    probed = []

    def fget(self):
        if _why_original(self) is not None:
            return original_fget(self)
        standardize = False
        if name == "quaternions":
            if not probed:
                fn = getattr(original_fget, "__globals__", {}).get("matrix_to_quaternion")
                probed.append(None if fn is None else standardizes(fn))
            if probed[0] is None:        # (a getter that does not reach matrix_to_quaternion through its module is not the reference's)
                return original_fget(self)
            standardize = probed[0]
        return bound_gaussians(self._points, self._surface_mesh_faces, self.surface_triangle_bary_coords[..., 0], self._quaternions, self._scales,
                               self.surface_mesh_thickness, want=(name,), standardize=standardize)[0]

    return _takes.dressed(fget, name, original_fget, f"SuGaR.{name}", "bound")


def drop_in_points(original_fget: Callable) -> Callable:
    """A getter for ``SuGaR.points`` that runs :func:`bound_gaussians` with only the points wanted on a bound CUDA float32 model, and
    ``original_fget`` for every other: an unbound model, ``editable=True``, a ``scale_activation`` that is not ``torch.exp``, a CPU model,
    other dtypes, graph capture -- decided before anything is read.  Nothing is cached between accesses."""
    return _drop_in("points", original_fget)


def drop_in_scaling(original_fget: Callable) -> Callable:
    """As :func:`drop_in_points`, for ``SuGaR.scaling``."""
    return _drop_in("scaling", original_fget)


def drop_in_quaternions(original_fget: Callable) -> Callable:
    """As :func:`drop_in_points`, for ``SuGaR.quaternions``.  Whether the quaternions are standardised follows the
    ``matrix_to_quaternion`` in ``original_fget``'s module, probed once on the host at the first access (:func:`standardizes`)."""
    return _drop_in("quaternions", original_fget)


# ---- the contract in numpy ------------------------------------------------------------------------------------------------------------

def _unit(w: np.ndarray, m: np.ndarray) -> np.ndarray:
    return w / np.fmax(m, UNIT_EPS)[..., None]


def _unit_backward(x: np.ndarray, m: np.ndarray, g: np.ndarray) -> np.ndarray:
    D = np.fmax(m, UNIT_EPS)
    gx = g / D[..., None]
    w = (-(_dot(g, x) / (D * D))) / m
    return np.where((m >= UNIT_EPS)[..., None], gx + x * w[..., None], gx)


def _inputs(verts, faces, bary, complex, log_scales):
    verts, faces = _mesh_host.verts_faces(verts, faces)
    bary = np.asarray(bary, dtype=_F).reshape(-1, 3)
    G, N = bary.shape[0], faces.shape[0] * bary.shape[0]
    return verts, faces, bary, np.asarray(complex, dtype=_F).reshape(N, 2), np.asarray(log_scales, dtype=_F).reshape(N, 2), G


def _frame(verts: np.ndarray, faces: np.ndarray) -> dict:
    """Per face: ``valid`` and the contract's a, b, c, n, normal, m0, r0, e, me, b1, x, mx, b2 (zeros for the faces that are not valid)."""
    t = {}
    t["valid"], t["v0"], t["v1"], t["v2"] = _mesh_host.face_corners(verts, faces)
    t["a"], t["b"], t["c"], t["n"] = _mesh_host.face_cross(t["v0"], t["v1"], t["v2"])
    t["normal"] = t["c"] / np.fmax(t["n"], _mesh_host.FACE_NORMAL_EPS)[:, None]
    t["m0"] = _norm(t["normal"])
    t["r0"] = _unit(t["normal"], t["m0"])
    t["e"] = t["v0"] - t["v1"]
    t["me"] = _norm(t["e"])
    t["b1"] = _unit(t["e"], t["me"])
    t["x"] = _cross(t["r0"], t["b1"])
    t["mx"] = _norm(t["x"])
    t["b2"] = _unit(t["x"], t["mx"])
    return t


_ROWS = (   # row k of the candidates: per entry ("q",) or (i, j, sign, i', j'): m_ij + sign m_i'j'
    (("q",), (2, 1, -1, 1, 2), (0, 2, -1, 2, 0), (1, 0, -1, 0, 1)),
    ((2, 1, -1, 1, 2), ("q",), (1, 0, 1, 0, 1), (0, 2, 1, 2, 0)),
    ((0, 2, -1, 2, 0), (1, 0, 1, 0, 1), ("q",), (1, 2, 1, 2, 1)),
    ((1, 0, -1, 0, 1), (2, 0, 1, 0, 2), (2, 1, 1, 1, 2), ("q",)),
)
_PRE_SIGNS = ((1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1))


def _rotation(t: dict, complex: np.ndarray, G: int, standardize: bool) -> dict:
    """Per Gaussian: the contract's z, R_1, R_2, k, pre[k], q_abs[k], d, u, flipped, |row| and the quaternion."""
    rep = lambda a: np.repeat(a, G, axis=0)
    r0, b1, b2 = rep(t["r0"]), rep(t["b1"]), rep(t["b2"])
    r = {"r0": r0, "b1": b1, "b2": b2}
    r["mz"] = np.sqrt(complex[:, 0] * complex[:, 0] + complex[:, 1] * complex[:, 1])
    z = complex / np.fmax(r["mz"], UNIT_EPS)[:, None]
    zr, zi = z[:, 0:1], z[:, 1:2]
    r["zr"], r["zi"] = zr, zi
    r1 = zr * b1 + zi * b2
    r2 = (-zi) * b1 + zr * b2
    m = np.stack((r0, r1, r2), axis=-1)                                            # m[:, i, j]: component i of column j
    r["m"] = m
    one = _F(1.0)
    pre = np.stack((((one + m[:, 0, 0]) + m[:, 1, 1]) + m[:, 2, 2], ((one + m[:, 0, 0]) - m[:, 1, 1]) - m[:, 2, 2],
                    ((one - m[:, 0, 0]) + m[:, 1, 1]) - m[:, 2, 2], ((one - m[:, 0, 0]) - m[:, 1, 1]) + m[:, 2, 2]), axis=1)
    q_abs = np.where(pre > 0, np.sqrt(np.where(pre > 0, pre, one)), _F(0.0)).astype(_F)
    r["pre_all"], r["q_abs"] = pre, q_abs
    k = np.zeros(len(complex), np.int64)
    best = q_abs[:, 0].copy()
    for j in range(1, 4):
        better = q_abs[:, j] > best
        k, best = np.where(better, j, k), np.where(better, q_abs[:, j], best)
    r["k"], r["qk"] = k, best
    r["pre"] = np.take_along_axis(pre, k[:, None], axis=1)[:, 0]
    sq = best * best
    cand = np.zeros((len(complex), 4), _F)
    for row, entries in enumerate(_ROWS):
        for e, entry in enumerate(entries):
            if entry == ("q",):
                value = sq
            else:
                i, j, sign, i2, j2 = entry
                value = m[:, i, j] + m[:, i2, j2] if sign > 0 else m[:, i, j] - m[:, i2, j2]
            cand[:, e] = np.where(k == row, value, cand[:, e])
    r["d"] = _F(2.0) * np.fmax(best, QUAT_FLOOR)
    r["u"] = cand / r["d"][:, None]
    r["flipped"] = (r["u"][:, 0] < 0) if standardize else np.zeros(len(complex), bool)
    r["s"] = np.where(r["flipped"][:, None], -r["u"], r["u"])
    r["mq"] = _norm(r["s"])
    r["out"] = _unit(r["s"], r["mq"])
    return r


def bound_gaussians_host(verts, faces, bary, complex, log_scales, thickness, standardize: bool = False):
    """The forward of the module's contract in numpy, every operation an fp32 elementwise one in the contract's order.  Returns
    ``(points [F G, 3], scaling [F G, 3], quaternions [F G, 4])``."""
    verts, faces, bary, complex, log_scales, G = _inputs(verts, faces, bary, complex, log_scales)
    with np.errstate(all="ignore"):
        t = _frame(verts, faces)
        r = _rotation(t, complex, G, standardize)
        valid = np.repeat(t["valid"], G)
        v0, v1, v2 = (np.repeat(t[k], G, axis=0) for k in ("v0", "v1", "v2"))
        w = np.tile(bary, (faces.shape[0], 1))
        points = (v0 * w[:, 0:1] + v1 * w[:, 1:2]) + v2 * w[:, 2:3]
        scaling = np.concatenate((np.full((len(complex), 1), np.asarray(thickness, _F).reshape(-1)[0], _F), np.exp(log_scales)), axis=1)
    return (np.where(valid[:, None], points, _F(0.0)).astype(_F), scaling.astype(_F), np.where(valid[:, None], r["out"], _F(0.0)).astype(_F))


def bound_gaussians_backward_host(verts, faces, bary, complex, log_scales, grad_points=None, grad_scaling=None, grad_quaternions=None,
                                  standardize: bool = False):
    """The backward of the module's contract in numpy.  Returns ``(grad_verts [V, 3], grad_complex [F G, 2], grad_log_scales [F G, 2],
    added [T, 3], rows [T])``: ``added[i]`` is what a face adds to vertex ``rows[i]`` (three entries per face with all indices in range, in
    face order), each an fp32 value fixed by the contract; ``grad_verts`` is their fp32 sum in that order, one of the orders the kernel's
    atomics may take."""
    verts, faces, bary, complex, log_scales, G = _inputs(verts, faces, bary, complex, log_scales)
    F, N = faces.shape[0], len(complex)
    zero3 = np.zeros((F, 3), _F)
    with np.errstate(all="ignore"):
        t = _frame(verts, faces)
        grad_log_scales = np.zeros((N, 2), _F)
        if grad_scaling is not None:
            grad_log_scales = (np.asarray(grad_scaling, _F).reshape(N, 3)[:, 1:3] * np.exp(log_scales)).astype(_F)
        P = [zero3.copy(), zero3.copy(), zero3.copy()]
        if grad_points is not None:
            gp = np.asarray(grad_points, _F).reshape(F, G, 3)
            for g in range(G):
                for i in range(3):
                    P[i] = P[i] + bary[g, i] * gp[:, g]
        grad_complex = np.zeros((N, 2), _F)
        terms = P
        if grad_quaternions is not None:
            r = _rotation(t, complex, G, standardize)
            gq = np.asarray(grad_quaternions, _F).reshape(N, 4)
            gs = _unit_backward(r["s"], r["mq"], gq)
            gu = np.where(r["flipped"][:, None], -gs, gs)
            gc = gu / r["d"][:, None]
            gd = -(_dot(gu, r["u"]) / r["d"])
            k, qk = r["k"], r["qk"]
            gqk = (_F(2.0) * qk) * np.take_along_axis(gc, k[:, None], axis=1)[:, 0]
            gqk = np.where(qk > QUAT_FLOOR, gqk + _F(2.0) * gd, gqk)
            gpre = np.where(r["pre"] > 0, gqk / (_F(2.0) * qk), _F(0.0)).astype(_F)
            gm = np.zeros((N, 3, 3), _F)
            for row, entries in enumerate(_ROWS):
                here = k == row
                for i in range(3):
                    gm[:, i, i] = np.where(here, _F(_PRE_SIGNS[row][i]) * gpre, gm[:, i, i])
                for e, entry in enumerate(entries):
                    if entry == ("q",):
                        continue
                    i, j, sign, i2, j2 = entry
                    gm[:, i, j] = np.where(here, gc[:, e], gm[:, i, j])
                    gm[:, i2, j2] = np.where(here, gc[:, e] if sign > 0 else -gc[:, e], gm[:, i2, j2])
            g0, g1, g2 = gm[:, :, 0], gm[:, :, 1], gm[:, :, 2]
            b1, b2, zr, zi = r["b1"], r["b2"], r["zr"], r["zi"]
            gz = np.stack((_dot(g1, b1) + _dot(g2, b2), _dot(g1, b2) - _dot(g2, b1)), axis=1)
            grad_complex = np.where(np.repeat(t["valid"], G)[:, None], _unit_backward(complex, r["mz"], gz), _F(0.0)).astype(_F)
            per = lambda a: a.reshape(F, G, 3)
            c0, c1, c2 = per(g0), per(zr * g1 + (-zi) * g2), per(zi * g1 + zr * g2)
            G0, G1, G2 = zero3.copy(), zero3.copy(), zero3.copy()
            for g in range(G):
                G0, G1, G2 = G0 + c0[:, g], G1 + c1[:, g], G2 + c2[:, g]
            gx = _unit_backward(t["x"], t["mx"], G2)
            G0, G1 = G0 + _cross(t["b1"], gx), G1 + _cross(gx, t["r0"])
            ge = _unit_backward(t["e"], t["me"], G1)
            gn = _unit_backward(t["normal"], t["m0"], G0)
            g_c = _mesh_host.normal_backward(t["c"], t["n"], gn)
            g_a, g_b = _cross(t["b"], g_c), _cross(g_c, t["a"])
            terms = [(P[0] + ge) + (-(g_a + g_b)), (P[1] + (-ge)) + g_a, P[2] + g_b]
    keep = np.nonzero(t["valid"])[0]
    added = np.stack(terms, axis=1).astype(_F)[keep].reshape(-1, 3)
    rows = faces[keep].reshape(-1)
    grad_verts = np.zeros((verts.shape[0], 3), _F)
    with np.errstate(all="ignore"):
        np.add.at(grad_verts, rows, added)
    return grad_verts, grad_complex, grad_log_scales, added, rows
