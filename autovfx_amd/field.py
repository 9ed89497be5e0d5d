"""SuGaR's density field over a neighbour list, fused: ``SuGaR.get_field_values`` (``sugar/sugar_scene/sugar_model.py:1118-1187``, once per
regularised iteration of all three trainers, 1 M samples x 16 neighbours) and ``SuGaR.compute_density`` (``:1216-1239``, the mesh extraction).

The reference gathers ``[N, K, 3]`` centres, ``[N, K, 3, 3]`` inverse scaled rotations and ``[N, K]`` strengths, runs a batched 3x3
product, a square-sum, a clamp, an ``exp`` and a sum over K, and its backward scatters all of that back with index-accumulate
atomics.  :func:`field_values` is one autograd Function over the HIP kernels of ``gsr_field.hip`` (C ABI ``gsr_field_forward`` /
``gsr_field_backward``): one lane per sample, one 64-byte record per (sample, neighbour), nothing of size ``[N, K]`` kept for the backward
except the outputs asked for.  The contract, per sample ``i`` and slot ``k`` with ``j = idx[i, k]``, plain fp32,
left to right, nothing contracted:

* ``s = x_i - c_j``; ``w_a = (M_j[0][a] s_0 + M_j[1][a] s_1) + M_j[2][a] s_2`` (``M^T s``, ``:1146``);
* ``q = clamp((w_0 w_0 + w_1 w_1) + w_2 w_2, 0, 1e8)``; ``o[i, k] = (density_factor sigma_j) exp(-0.5 q)``;
* ``density[i] = sum_k o[i, k]`` and ``beta[i] = (sum_k m_j) / K`` (``get_beta``'s ``'average'`` mode, ``:1066``), k ascending from 0;
* a slot whose index is outside ``[0, P)`` is skipped: 0 to both sums, opacity 0, no gradient, nothing read (a deliberate deviation --
  ``knn_points`` here writes ``-1`` for a missing slot, PyTorch's gather would raise or fault).

Backward, with ``G = g_density[i] + g_opacities[i, k]``: ``dsigma_j += (G density_factor) e``; ``dq = (-0.5 G) o``, 0 where ``q`` lay
strictly outside ``[0, 1e8]`` before the clamp (torch's rule); ``dw_a = (2 w_a) dq``; ``ds_b = (M_j[b][0] dw_0 + M_j[b][1] dw_1) +
M_j[b][2] dw_2``; ``dx_i += ds``; ``dc_j -= ds``; ``dM_j[b][a] += s_b dw_a``; ``dm_j += g_beta[i] / K``.  The per-Gaussian sums meet
through float atomics: their last bits depend on the order of arrival.

:func:`field_values_host` / :func:`field_grads_host` restate both in numpy, the checker of the tests; :func:`drop_in_compute_density`
and :func:`drop_in_get_field_values` are what ``autovfx_amd.install()`` puts on ``SuGaR``.
"""
from __future__ import annotations

import math
from typing import Callable, Optional

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _takes

MAX_K = 64
MAX_COUNT = (1 << 30) - 1
Q_MAX = 1e8


def _why_not(x, idx, centers, inv_scaled_rotation, strengths, min_scaling=None, want_beta=False) -> Optional[str]:
    """None when the kernels take the call, else the reason they do not."""
    f32 = torch.float32
    named = (("x", x, f32), ("idx", idx, torch.int64), ("centers", centers, f32), ("inv_scaled_rotation", inv_scaled_rotation, f32),
             ("strengths", strengths, f32)) + ((("min_scaling", min_scaling, f32),) if min_scaling is not None else ())
    why = (_takes.tensors(named, host="field_values_host") or _takes.shaped("x", x, "[N, 3]", x.dim() == 2 and x.shape[1] == 3)
           or _takes.gaussians(x.shape[0], idx, centers, inv_scaled_rotation, strengths, MAX_K, "N"))
    if why is not None:
        return why
    P = centers.shape[0]
    if min_scaling is not None and tuple(min_scaling.shape) != (P,):
        return _takes.shaped("min_scaling", min_scaling, f"[P] with P = {P}", False)
    if want_beta and min_scaling is None:
        return "beta needs min_scaling"
    if x.shape[0] > MAX_COUNT or P > MAX_COUNT:
        return f"{x.shape[0]} samples and {P} Gaussians: at most 2^30 - 1 each"
    return _takes.capturing("the call allocates its scratch")


def field_takes(x, idx, centers, inv_scaled_rotation, strengths, min_scaling=None, density_factor=1.0, want_opacities=False,
                want_beta=False) -> bool:
    """Whether :func:`field_values` runs this call: CUDA float32 tensors on one device, ``x [N, 3]``, int64 ``idx [N, K]`` with
    ``1 <= K <= 64`` (any values: slots outside ``[0, P)``, pytorch3d-style ``-1`` among them, are skipped), ``centers [P, 3]``,
    ``inv_scaled_rotation [P, 3, 3]``, ``strengths [P]`` or ``[P, 1]``, ``min_scaling [P]`` when beta is wanted, a host number as
    ``density_factor``, not under graph capture.  Non-contiguous tensors and inputs that require gradients are taken."""
    if isinstance(density_factor, torch.Tensor) or not isinstance(density_factor, (int, float)):
        return False
    return _why_not(x, idx, centers, inv_scaled_rotation, strengths, min_scaling, want_beta) is None


class _Field(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, idx, centers, M, strengths, min_scaling, density_factor, want_opacities, want_beta):
        from . import _lib

        ctx.set_materialize_grads(False)      # an output nobody differentiates reaches the kernel as NULL, not as [N, K] zeros
        xs, ix, cs, Ms, ss = _takes.cs(x, idx, centers, M, strengths)
        ms = None if min_scaling is None else _takes.c(min_scaling)
        N, K, P = int(xs.shape[0]), int(ix.shape[1]), int(cs.shape[0])
        dev = xs.device
        density = torch.empty(N, dtype=torch.float32, device=dev)
        opacities = torch.empty((N, K), dtype=torch.float32, device=dev) if want_opacities else None
        beta = torch.empty(N, dtype=torch.float32, device=dev) if want_beta else None
        if P == 0:                      # every slot is out of range
            for out in (density, opacities, beta):
                if out is not None:
                    out.zero_()
        elif N > 0:
            with torch.cuda.device(dev):
                scratch, nbytes = _lib.scratch("gsr_field_scratch_bytes", P, device=dev)
                _lib.call("gsr_field_forward", N, K, P, xs.data_ptr(), ix.data_ptr(), cs.data_ptr(), Ms.data_ptr(), ss.data_ptr(),
                          _lib.ptr(ms), density_factor, density.data_ptr(), _lib.ptr(opacities), _lib.ptr(beta),
                          scratch.data_ptr(), nbytes, device=dev)
        ctx.save_for_backward(xs, ix, cs, Ms, ss, ms)     # the inputs: nothing of size [N, K] but the caller's own idx
        ctx.density_factor = density_factor
        ctx.strengths_shape = strengths.shape
        return density, opacities, beta

    @staticmethod
    @once_differentiable
    def backward(ctx, g_density, g_opacities, g_beta):
        from . import _lib

        xs, ix, cs, Ms, ss, ms = ctx.saved_tensors
        need = ctx.needs_input_grad
        N, K, P = int(xs.shape[0]), int(ix.shape[1]), int(cs.shape[0])
        dev = xs.device
        gd, go, gb = (None if g is None else g.detach().to(torch.float32).contiguous() for g in (g_density, g_opacities, g_beta))
        dx = torch.empty((N, 3), dtype=torch.float32, device=dev) if need[0] else None
        accum = torch.zeros((P, 16), dtype=torch.float32, device=dev)
        if N > 0 and P > 0:
            with torch.cuda.device(dev):
                scratch, nbytes = _lib.scratch("gsr_field_scratch_bytes", P, device=dev)
                _lib.call("gsr_field_backward", N, K, P, xs.data_ptr(), ix.data_ptr(), cs.data_ptr(), Ms.data_ptr(), ss.data_ptr(),
                          _lib.ptr(ms), ctx.density_factor, _lib.ptr(gd), _lib.ptr(go), _lib.ptr(gb), _lib.ptr(dx), accum.data_ptr(),
                          scratch.data_ptr(), nbytes, device=dev)
        elif dx is not None:
            dx.zero_()
        return (dx, None,
                accum[:, 0:3].contiguous() if need[2] else None,
                accum[:, 3:12].reshape(P, 3, 3) if need[3] else None,
                accum[:, 12].reshape(ctx.strengths_shape).contiguous() if need[4] else None,
                accum[:, 13].contiguous() if need[5] and ms is not None else None,
                None, None, None)


def field_values(x, idx, centers, inv_scaled_rotation, strengths, min_scaling=None, density_factor: float = 1.0,
                 want_opacities: bool = False, want_beta: bool = False):
    """``(density [N], opacities [N, K] or None, beta [N] or None)`` of the contract above, on the current stream, no host
    synchronisation.  Gradients flow into ``x``, ``centers``, ``inv_scaled_rotation``, ``strengths`` and ``min_scaling``, each only if it
    requires one.  A call :func:`field_takes` rejects raises ``ValueError`` with the reason."""
    if isinstance(density_factor, torch.Tensor) or not isinstance(density_factor, (int, float)):
        _takes.refuse("field_values", f"density_factor must be a host number (got {type(density_factor).__name__})")
    _takes.refuse("field_values", _why_not(x, idx, centers, inv_scaled_rotation, strengths, min_scaling, want_beta))
    return _Field.apply(x, idx, centers, inv_scaled_rotation, strengths, min_scaling if want_beta else None, float(density_factor),
                        bool(want_opacities), bool(want_beta))


# ---- the contract in numpy ----
def _host_inputs(x, idx, centers, M, strengths, min_scaling):
    x = np.asarray(x, np.float32).reshape(-1, 3)
    idx = np.asarray(idx, np.int64).reshape(x.shape[0], -1)
    c = np.asarray(centers, np.float32).reshape(-1, 3)
    M = np.asarray(M, np.float32).reshape(-1, 3, 3)
    sg = np.asarray(strengths, np.float32).reshape(-1)
    ms = None if min_scaling is None else np.asarray(min_scaling, np.float32).reshape(-1)
    valid = (idx >= 0) & (idx < c.shape[0])
    return x, idx, c, M, sg, ms, valid, np.where(valid, idx, 0)


def _host_pairs(x, c, M, j):
    """s [N,K,3], w [N,K,3], q before the clamp, e = exp(-0.5 clamp(q)), all fp32 elementwise in the contract's order."""
    s = x[:, None, :] - c[j]
    Mj = M[j]
    w = (Mj[..., 0, :] * s[..., 0:1] + Mj[..., 1, :] * s[..., 1:2]) + Mj[..., 2, :] * s[..., 2:3]
    q_raw = (w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1]) + w[..., 2] * w[..., 2]
    q = np.where(q_raw < 0, np.float32(0), np.where(q_raw > np.float32(Q_MAX), np.float32(Q_MAX), q_raw))
    return s, w, q_raw, np.exp(np.float32(-0.5) * q).astype(np.float32), Mj


def _sum_ascending(a):
    out = np.zeros(a.shape[0], np.float32)
    for k in range(a.shape[1]):
        out = out + a[:, k]
    return out


def field_values_host(x, idx, centers, inv_scaled_rotation, strengths, min_scaling=None, density_factor: float = 1.0):
    """The forward contract in numpy (fp32 elementwise, left to right): ``(density [N], opacities [N, K], beta [N] or None)``."""
    x, idx, c, M, sg, ms, valid, j = _host_inputs(x, idx, centers, inv_scaled_rotation, strengths, min_scaling)
    zero = np.float32(0)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if c.shape[0] == 0:
            o = np.zeros(idx.shape, np.float32)
        else:
            _, _, _, e, _ = _host_pairs(x, c, M, j)
            o = np.where(valid, (np.float32(density_factor) * sg[j]) * e, zero).astype(np.float32)
        beta = None
        if ms is not None:
            beta = _sum_ascending(np.where(valid, ms[j], zero) if c.shape[0] else np.zeros(idx.shape, np.float32)) / np.float32(idx.shape[1])
    return _sum_ascending(o), o, beta


def field_grads_host(x, idx, centers, inv_scaled_rotation, strengths, min_scaling=None, density_factor: float = 1.0, g_density=None,
                     g_opacities=None, g_beta=None) -> dict:
    """The backward contract in numpy: every term in fp32 in the contract's order; the per-Gaussian sums, which the kernel forms with
    atomics in arrival order, are taken here in (i, k) order.  Keys ``x``, ``centers``, ``inv_scaled_rotation``, ``strengths``
    (``[P]``), ``min_scaling``."""
    x, idx, c, M, sg, ms, valid, j = _host_inputs(x, idx, centers, inv_scaled_rotation, strengths, min_scaling)
    N, K = idx.shape
    P = c.shape[0]
    f = np.float32
    gd = np.zeros(N, f) if g_density is None else np.asarray(g_density, f).reshape(N)
    out = {"x": np.zeros((N, 3), f), "centers": np.zeros((P, 3), f), "inv_scaled_rotation": np.zeros((P, 3, 3), f), "strengths": np.zeros(P, f),
           "min_scaling": np.zeros(P, f)}
    if P == 0:
        return out
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        s, w, q_raw, e, Mj = _host_pairs(x, c, M, j)
        G = np.broadcast_to(gd[:, None], (N, K)) if g_opacities is None else gd[:, None] + np.asarray(g_opacities, f).reshape(N, K)
        o = (f(density_factor) * sg[j]) * e
        dsig = np.where(valid, (G * f(density_factor)) * e, f(0))
        dq = np.where(valid & ~((q_raw < 0) | (q_raw > f(Q_MAX))), (f(-0.5) * G) * o, f(0))
        dw = (f(2) * w) * dq[..., None]
        ds = (Mj[..., :, 0] * dw[..., 0:1] + Mj[..., :, 1] * dw[..., 1:2]) + Mj[..., :, 2] * dw[..., 2:3]
        dM = s[..., :, None] * dw[..., None, :]
        for k in range(K):
            out["x"] = out["x"] + ds[:, k]
    flat = j.reshape(-1)
    np.add.at(out["centers"], flat, -ds.reshape(-1, 3))
    np.add.at(out["inv_scaled_rotation"], flat, dM.reshape(-1, 3, 3))
    np.add.at(out["strengths"], flat, dsig.reshape(-1))
    if ms is not None and g_beta is not None:
        gm = np.asarray(g_beta, f).reshape(N) / f(K)
        np.add.at(out["min_scaling"], flat, np.where(valid, gm[:, None], f(0)).reshape(-1))
    return out


# ---- what install() puts on SuGaR ----
def _quick_no(x) -> bool:
    """Calls that go to the reference before any input is built: not a CUDA float32 [N, 3] sample tensor, or under graph capture."""
    return (not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != 3
            or _takes.capturing("") is not None)


def drop_in_compute_density(original: Callable) -> Callable:
    """``SuGaR.compute_density`` (``sugar_model.py:1216-1239``): the inputs are built as the reference builds them, the gather, product,
    ``exp`` and sum are :func:`field_values`.  A call the kernels do not take (CPU tensors, another dtype, ...) runs ``original``."""
    def compute_density(self, x, closest_gaussians_idx=None, density_factor=1., return_closest_gaussian_opacities=False):
        if _quick_no(x):
            return original(self, x, closest_gaussians_idx=closest_gaussians_idx, density_factor=density_factor,
                            return_closest_gaussian_opacities=return_closest_gaussian_opacities)
        if closest_gaussians_idx is None:
            closest_gaussians_idx = self.get_gaussians_closest_to_samples(x)
        centers = self.points
        inv_scaled_rotation = self.get_covariance(return_full_matrix=True, return_sqrt=True, inverse_scales=True)
        strengths = self.strengths
        if not field_takes(x, closest_gaussians_idx, centers, inv_scaled_rotation, strengths, None, density_factor):
            return original(self, x, closest_gaussians_idx=closest_gaussians_idx, density_factor=density_factor,
                            return_closest_gaussian_opacities=return_closest_gaussian_opacities)
        densities, neighbor_opacities, _ = field_values(x, closest_gaussians_idx, centers, inv_scaled_rotation, strengths, None, density_factor,
                                                        want_opacities=return_closest_gaussian_opacities)
        return (densities, neighbor_opacities) if return_closest_gaussian_opacities else densities

    return _takes.dressed(compute_density, "compute_density", original, "SuGaR.compute_density", "field")


def drop_in_get_field_values(original: Callable) -> Callable:
    """``SuGaR.get_field_values`` (``sugar_model.py:1118-1187``): defaults and keyword overrides as the reference resolves them, the
    gather / product / ``exp`` / sum (and ``get_beta``'s ``'average'`` mode) in :func:`field_values`, then the reference's own statements:
    the ``density`` clone, the ``>= 1`` renormalisation, ``get_beta`` for the other modes, the clamped densities, the ``sdf`` value.
    ``return_sdf_grad=True`` (no trainer passes it) and every call the kernels do not take run ``original``."""
    def get_field_values(self, x, gaussian_idx=None, closest_gaussians_idx=None, gaussian_strengths=None, gaussian_centers=None,
                         gaussian_inv_scaled_rotation=None, return_sdf=True, density_threshold=1., density_factor=1.,
                         return_sdf_grad=False, sdf_grad_max_value=10., opacity_min_clamp=1e-16,
                         return_closest_gaussian_opacities=False, return_beta=False):
        def reference():
            return original(self, x, gaussian_idx=gaussian_idx, closest_gaussians_idx=closest_gaussians_idx,
                            gaussian_strengths=gaussian_strengths, gaussian_centers=gaussian_centers,
                            gaussian_inv_scaled_rotation=gaussian_inv_scaled_rotation, return_sdf=return_sdf,
                            density_threshold=density_threshold, density_factor=density_factor, return_sdf_grad=return_sdf_grad,
                            sdf_grad_max_value=sdf_grad_max_value, opacity_min_clamp=opacity_min_clamp,
                            return_closest_gaussian_opacities=return_closest_gaussian_opacities, return_beta=return_beta)

        if return_sdf_grad or _quick_no(x):
            return reference()
        if gaussian_strengths is None:
            gaussian_strengths = self.strengths
        if gaussian_centers is None:
            gaussian_centers = self.points
        if gaussian_inv_scaled_rotation is None:
            gaussian_inv_scaled_rotation = self.get_covariance(return_full_matrix=True, return_sqrt=True, inverse_scales=True)
        if closest_gaussians_idx is None:
            closest_gaussians_idx = self.knn_idx[gaussian_idx]

        needs_beta = return_sdf or return_beta
        fused_beta = needs_beta and self.beta_mode == 'average'
        wants_opacities = return_closest_gaussian_opacities or (needs_beta and self.beta_mode == 'weighted_average')
        min_scaling = self.scaling.min(dim=-1)[0] if fused_beta else None
        if not field_takes(x, closest_gaussians_idx, gaussian_centers, gaussian_inv_scaled_rotation, gaussian_strengths, min_scaling,
                           density_factor, wants_opacities, fused_beta):
            gaussian_idx = None       # (resolved above; the reference then takes closest_gaussians_idx as it is)
            return reference()
        densities, neighbor_opacities, beta = field_values(x, closest_gaussians_idx, gaussian_centers, gaussian_inv_scaled_rotation,
                                                           gaussian_strengths, min_scaling, density_factor, wants_opacities, fused_beta)

        # what the reference does with the sum (:1150-1178), in the same arithmetic
        fields = {"density": densities.clone()}
        saturated = densities >= 1.0
        densities = torch.where(saturated, densities / (densities.detach() + 1e-12), densities)     # (:1151-1152: >= 1 becomes 1, gradient kept)
        if return_closest_gaussian_opacities:
            fields["closest_gaussian_opacities"] = neighbor_opacities
        if needs_beta:
            if not fused_beta:        # 'weighted_average' and 'learnable' stay get_beta's
                beta = self.get_beta(x, closest_gaussians_idx=closest_gaussians_idx, closest_gaussians_opacities=neighbor_opacities,
                                     densities=densities, opacity_min_clamp=opacity_min_clamp)
            if return_beta:
                fields["beta"] = beta
        if return_sdf:
            level = math.sqrt(-2.0 * math.log(min(density_threshold, 1.0)))
            fields["sdf"] = beta * (torch.sqrt(-2.0 * torch.log(densities.clamp(min=opacity_min_clamp))) - level)
        return fields

    return _takes.dressed(get_field_values, "get_field_values", original, "SuGaR.get_field_values", "field")
