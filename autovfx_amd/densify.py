"""The densification of the reference's training loops (``scene/gaussian_model.py:339-417``) without its boolean-mask round trips.

Drop-ins for two methods of the reference's ``GaussianModel`` (installed by ``autovfx_amd.install()``):

* :func:`add_densification_stats` (``:415-417``, every iteration): one ``gsr_densify_stats`` launch, no host synchronisation, instead
  of two boolean-mask read-modify-writes and a masked gather (each boolean index is a ``nonzero`` with a host round trip);
* :func:`densify_and_prune` (``:399-413``, every 100 iterations): the reference rewrites the model and both Adam moments four times
  (clone ``cat``, split ``cat``, two boolean prunes).  Here ``gsr_densify_plan`` classifies all rows and places the survivors by
  prefix sums, the host reads three counts once, the children's ``xyz`` / ``scaling`` (2|S| rows) are computed with the reference's
  own torch expressions -- the same ``torch.normal`` call, so the generator ends where the reference leaves it -- and ONE
  ``gsr_densify_apply`` launch writes the six new parameters and twelve new moments.  Two host synchronisations (the counts; the
  children that survive the last prune) against more than twenty.

The results are the reference's bit for bit: values, order (kept originals, clones, children copy 1, copy 2), fresh ``nn.Parameter``
objects in ``group["params"][0]`` and on the model, the optimizer's state dictionaries re-keyed with ``step`` untouched, zeroed
``xyz_gradient_accum`` / ``denom`` / ``max_radii2D``.  A call :func:`kernel_takes` (or :func:`stats_kernel_takes`) does not accept
runs the reference's own method (``GaussianModel.reference_<name>``): torch's result or torch's exception.

:func:`plan_host` restates the plan in plain torch ops on any device, and :func:`densify_and_prune_host` runs the whole method on it:
what the CPU tests hold to the reference and the GPU tests hold the kernels to.
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, Optional

import torch
from torch import nn

from . import _lib
from .optim import _dense_fp32, _f32, _plain_number

__all__ = ["add_densification_stats", "densify_and_prune", "densify_and_prune_host", "kernel_takes", "stats_kernel_takes", "plan_host",
           "accumulate_stats"]

# the optimizer's group names and the model attributes they hold (gaussian_model.py:164-171), with the floats of a row
GROUPS = (("xyz", "_xyz"), ("f_dc", "_features_dc"), ("f_rest", "_features_rest"), ("opacity", "_opacity"), ("scaling", "_scaling"),
          ("rotation", "_rotation"))
_TAIL = {"xyz": (3,), "f_dc": (1, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,)}   # f_rest: (k, 3), any k >= 0
MAX_ROWS = 1 << 29       # 3 N rows and 2 N indices stay below 2^31


def _finite32(x) -> bool:
    return _plain_number(x) and math.isfinite(x) and math.isfinite(_f32(x))


def _bounds(model, max_grad, min_opacity, extent, max_screen_size) -> Optional[dict]:
    """The reference's Python scalars (gaussian_model.py:366,388,406,409), or None when one of them is no finite plain number."""
    try:
        dense, ws = model.percent_dense * extent, 0.1 * extent
    except Exception:
        return None
    if not all(map(_finite32, (max_grad, min_opacity, dense, ws))):
        return None
    if max_screen_size is not None and not (_plain_number(max_screen_size) and max_screen_size >= 0):
        return None                                   # a negative size prunes every row through `max_radii2D > size`
    return {"max_grad": max_grad, "dense_bound": dense, "min_opacity": min_opacity, "ws_bound": ws if max_screen_size else None}


def kernel_takes(model, max_grad, min_opacity, extent, max_screen_size, capturing: bool = False, device_type: str = "cuda") -> bool:
    """Whether the kernels compute this ``densify_and_prune`` call exactly as the reference's method would.  Host only (reads
    attributes, launches nothing).  ``device_type``: where the kernels run; tests pass "meta" / "cpu" to walk the rules."""
    if capturing:
        return False
    b = _bounds(model, max_grad, min_opacity, extent, max_screen_size)
    if b is None or not max_grad > 0:                  # max_grad <= 0: clones could be split again (the padded gradient is 0)
        return False
    xyz = getattr(model, "_xyz", None)
    if not _dense_fp32(xyz, device_type) or xyz.dim() != 2:
        return False
    n, device = xyz.shape[0], xyz.device
    if not 2 <= n < MAX_ROWS:                          # n == 1: the reference's squeeze() makes a 0-d mask (its own shapes)
        return False
    opt = getattr(model, "optimizer", None)
    groups = getattr(opt, "param_groups", None)
    if not isinstance(groups, list) or len(groups) != 6 or sorted(g.get("name", "") for g in groups) != sorted(k for k, _ in GROUPS):
        return False
    by_name = {g["name"]: g for g in groups}
    for name, attr in GROUPS:
        p, group = getattr(model, attr, None), by_name[name]
        if len(group["params"]) != 1 or group["params"][0] is not p or type(p) is not nn.Parameter:
            return False
        tail = tuple(p.shape[1:])
        if not _dense_fp32(p, device_type, device) or p.dim() < 2 or p.shape[0] != n:
            return False
        if tail != _TAIL.get(name, tail) or (name == "f_rest" and (p.dim() != 3 or tail[1] != 3)):
            return False
        st = opt.state.get(p) if hasattr(opt.state, "get") else None
        if st is not None:
            m, v = st.get("exp_avg"), st.get("exp_avg_sq")
            if not (_dense_fp32(m, device_type, device) and _dense_fp32(v, device_type, device) and m.shape == p.shape and v.shape == p.shape):
                return False
    for stat in (getattr(model, "xyz_gradient_accum", None), getattr(model, "denom", None)):
        if not _dense_fp32(stat, device_type, device) or tuple(stat.shape) != (n, 1):
            return False
    return True


def stats_kernel_takes(model, viewspace_point_tensor, update_filter, capturing: bool = False, device_type: str = "cuda") -> bool:
    """Whether one ``gsr_densify_stats`` launch is this ``add_densification_stats`` call.  Host only."""
    if capturing:
        return False
    grad = getattr(viewspace_point_tensor, "grad", None)
    accum, denom = getattr(model, "xyz_gradient_accum", None), getattr(model, "denom", None)
    if not _dense_fp32(grad, device_type) or grad.dim() != 2 or grad.shape[1] < 2:
        return False
    n = grad.shape[0]
    if not 0 < n < MAX_ROWS:
        return False
    f = update_filter
    if not (isinstance(f, torch.Tensor) and f.dtype == torch.bool and f.device == grad.device and tuple(f.shape) == (n,) and f.is_contiguous()):
        return False
    return all(_dense_fp32(t, device_type, grad.device) and tuple(t.shape) == (n, 1) for t in (accum, denom)) and accum is not denom


def _reference(model, name: str):
    fn = getattr(type(model), "reference_" + name, None)
    if fn is None:
        raise RuntimeError(f"autovfx_amd.densify.{name}: the kernels do not take this call and {type(model).__name__} has no "
                           f"reference_{name} to run instead (autovfx_amd.install() keeps it)")
    return fn


# ---------------------------------------------------------------------------------------------------------------- stats
def accumulate_stats(grad: torch.Tensor, update_filter: torch.Tensor, accum: torch.Tensor, denom: torch.Tensor,
                     radii: Optional[torch.Tensor] = None, max_radii: Optional[torch.Tensor] = None) -> None:
    """``gsr_densify_stats`` on tensors: ``accum[f] += norm(grad[f, :2])``, ``denom[f] += 1`` and, with ``radii`` (int32) and
    ``max_radii`` given, ``max_radii[f] = max(max_radii[f], radii[f])`` -- the line the reference's loops spell inline.  One launch,
    no host synchronisation.  The caller vouches for the layout (dense fp32 / bool / int32 on one GPU)."""
    n = grad.shape[0]
    with torch.cuda.device(grad.device):
        _lib.call("gsr_densify_stats", n, grad.data_ptr(), grad.shape[1], update_filter.data_ptr(), accum.data_ptr(), denom.data_ptr(),
                  _lib.ptr(radii), _lib.ptr(max_radii), device=grad.device)
    torch.autograd.graph.increment_version([accum, denom] + ([max_radii] if max_radii is not None else []))


def add_densification_stats(self, viewspace_point_tensor, update_filter):
    """``GaussianModel.add_densification_stats`` (gaussian_model.py:415-417)."""
    if not stats_kernel_takes(self, viewspace_point_tensor, update_filter, _lib.capturing()):
        return _reference(self, "add_densification_stats")(self, viewspace_point_tensor, update_filter)
    accumulate_stats(viewspace_point_tensor.grad, update_filter, self.xyz_gradient_accum, self.denom)


# ----------------------------------------------------------------------------------------------------------------- plan
def plan_host(accum, denom, scaling, opacity, max_grad, dense_bound, min_opacity, ws_bound=None) -> Dict[str, torch.Tensor]:
    """The plan of ``densify_and_prune`` (gaussian_model.py:399-411, ``max_grad > 0``) in torch ops on the tensors' device, the
    scalars compared as the reference compares them (Python numbers against fp32 tensors).  ``ws_bound``: ``0.1 * extent`` when
    ``max_screen_size`` is set, else None.  Returns ``src_of`` (the kept originals, then the surviving clones: source rows, int32),
    ``split_idx`` (the split parents, int32), ``counts`` = [kept, clones, split, 0] and the three boolean classes."""
    g = accum / denom
    g[g.isnan()] = 0.0
    big = torch.max(torch.exp(scaling), dim=1).values
    clone = torch.logical_and(torch.norm(g, dim=-1) >= max_grad, big <= dense_bound)
    split = torch.logical_and(g.squeeze(-1) >= max_grad, big > dense_bound)   # the gradient padded with 0 for the clones: none of them
    pruned = (torch.sigmoid(opacity) < min_opacity).reshape(-1)
    if ws_bound is not None:
        pruned = torch.logical_or(pruned, big > ws_bound)   # max_radii2D was zeroed by densification_postfix: never above a size >= 0
    keep, clone_kept = ~split & ~pruned, clone & ~pruned
    rows = lambda mask: torch.nonzero(mask).reshape(-1).to(torch.int32)
    k, c, s = rows(keep), rows(clone_kept), rows(split)
    return {"src_of": torch.cat((k, c)), "split_idx": s, "keep": keep, "clone": clone_kept, "split": split,
            "counts": torch.tensor([k.numel(), c.numel(), s.numel(), 0], dtype=torch.int32)}


def _build_rotation(r: torch.Tensor) -> torch.Tensor:
    """utils/general_utils.py:78-99 (rotation matrices of unnormalised quaternions w, x, y, z), the same operations entry by entry."""
    norm = torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])
    q = r / norm[:, None]
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    rows = (1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
            2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
            2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y))
    return torch.stack(rows, dim=-1).reshape(-1, 3, 3)


def _children(model, sidx: torch.Tensor, b: dict):
    """The 2|S| children of the split parents ``sidx`` (int64 rows) as densify_and_split computes them (:368-373) on the gathered
    subset -- ONE torch.normal call of the reference's shapes, also for |S| == 0 -- and which of them the last prune keeps
    (:406-410; a child has its parent's opacity).  Returns (new_xyz, new_scaling, kept child rows as int64)."""
    scales = torch.exp(model._scaling.index_select(0, sidx))
    stds = scales.repeat(2, 1)
    means = torch.zeros((stds.size(0), 3), device=stds.device)
    samples = torch.normal(mean=means, std=stds)
    rots = _build_rotation(model._rotation.index_select(0, sidx)).repeat(2, 1, 1)
    new_xyz = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + model._xyz.index_select(0, sidx).repeat(2, 1)
    new_scaling = torch.log(scales.repeat(2, 1) / (0.8 * 2))
    if sidx.numel() == 0:
        return new_xyz, new_scaling, sidx
    pruned = (torch.sigmoid(model._opacity.index_select(0, sidx).repeat(2, 1)) < b["min_opacity"]).reshape(-1)
    if b["ws_bound"] is not None:
        pruned = torch.logical_or(pruned, torch.exp(new_scaling).max(dim=1).values > b["ws_bound"])
    return new_xyz, new_scaling, torch.nonzero(~pruned).reshape(-1)   # the second (and last) host synchronisation


def _install_results(model, new: Dict[str, tuple]) -> None:
    """Point 6: fresh Parameters in the groups and on the model, the state dictionaries re-keyed (``step`` untouched), zero stats."""
    opt = model.optimizer
    for group in opt.param_groups:
        p, m, v = new[group["name"]]
        old = group["params"][0]
        st = opt.state.get(old, None)
        param = nn.Parameter(p.requires_grad_(True))
        if st is not None:
            st["exp_avg"], st["exp_avg_sq"] = m, v
            del opt.state[old]
            group["params"][0] = param
            opt.state[param] = st
        else:
            group["params"][0] = param
        setattr(model, dict(GROUPS)[group["name"]], param)
    n, device = model._xyz.shape[0], model._xyz.device
    model.xyz_gradient_accum = torch.zeros((n, 1), device=device)
    model.denom = torch.zeros((n, 1), device=device)
    model.max_radii2D = torch.zeros((n), device=device)


def _sources(model):
    """name -> (parameter, exp_avg or None, exp_avg_sq or None)"""
    out = {}
    for name, attr in GROUPS:
        p = getattr(model, attr)
        st = model.optimizer.state.get(p, None)
        out[name] = (p, st["exp_avg"], st["exp_avg_sq"]) if st is not None else (p, None, None)
    return out


@torch.no_grad()
def densify_and_prune_host(self, max_grad, min_opacity, extent, max_screen_size):
    """The method on :func:`plan_host` and torch ops alone, on whatever device the model is: the restatement the tests compare
    with the reference's own method (CPU) and the kernels with (GPU).  The caller checked ``kernel_takes(..., device_type=...)``."""
    b = _bounds(self, max_grad, min_opacity, extent, max_screen_size)
    plan = plan_host(self.xyz_gradient_accum, self.denom, self._scaling, self._opacity, **b)
    n_keep = int(plan["counts"][0])
    src_of, sidx = plan["src_of"].to(torch.int64), plan["split_idx"].to(torch.int64)
    new_xyz, new_scaling, child_rows = _children(self, sidx, b)
    parents = sidx.repeat(2).index_select(0, child_rows)
    side = {"xyz": new_xyz, "scaling": new_scaling}
    new = {}
    for name, (p, m, v) in _sources(self).items():
        front = p.index_select(0, src_of)
        kids = side[name].index_select(0, child_rows) if name in side else p.index_select(0, parents)
        moments = []
        for t in (m, v):
            if t is None:
                moments.append(None)
                continue
            out = torch.zeros_like(torch.cat((front, kids)))
            out[:n_keep] = t.index_select(0, src_of[:n_keep])
            moments.append(out)
        new[name] = (torch.cat((front, kids)), *moments)
    _install_results(self, new)
    torch.cuda.empty_cache()


@torch.no_grad()
def _densify_and_prune_kernels(self, b: dict, empty_cache: bool = True) -> None:
    n, device = self._xyz.shape[0], self._xyz.device
    with torch.cuda.device(device):
        scratch, scratch_bytes = _lib.scratch("gsr_densify_plan_scratch_bytes", n, device=device)
        src_of = torch.empty(2 * n, dtype=torch.int32, device=device)
        split_idx = torch.empty(n, dtype=torch.int32, device=device)
        counts = torch.empty(4, dtype=torch.int32, device=device)
        ws = b["ws_bound"]
        _lib.call("gsr_densify_plan", n, self.xyz_gradient_accum.data_ptr(), self.denom.data_ptr(), self._scaling.data_ptr(),
                  self._opacity.data_ptr(), _f32(b["max_grad"]), _f32(b["dense_bound"]), _f32(b["min_opacity"]),
                  0 if ws is None else 1, 0.0 if ws is None else _f32(ws), src_of.data_ptr(), split_idx.data_ptr(),
                  counts.data_ptr(), scratch.data_ptr(), scratch_bytes, device=device)
        n_keep, n_clone, n_split, _ = counts.tolist()               # the first host synchronisation: the sizes of everything below
        new_xyz, new_scaling, child_rows = _children(self, split_idx[:n_split].to(torch.int64), b)
        child_rows = child_rows.to(torch.int32)
        n_front = n_keep + n_clone
        n_out = n_front + child_rows.numel()
        side = {"xyz": new_xyz.contiguous(), "scaling": new_scaling.contiguous()}
        descs, new = [], {}
        for name, (p, m, v) in _sources(self).items():
            row = p[0].numel()
            outs = []
            for k, t in enumerate((p, m, v)):
                if t is None:
                    outs.append(None)
                    continue
                out = torch.empty((n_out,) + tuple(p.shape[1:]), dtype=torch.float32, device=device)
                outs.append(out)
                if row and n_out:
                    s = side.get(name) if k == 0 else None
                    descs.append(_lib.DensifyTensor(t.data_ptr(), out.data_ptr(), s.data_ptr() if s is not None and s.numel() else None, row,
                                                    0 if k == 0 else 1))
            new[name] = tuple(outs)
        if descs:
            plan = _lib.DensifyPlan(n, n_keep, n_front, n_out, n_split, src_of.data_ptr(), child_rows.data_ptr() if child_rows.numel() else None,
                                    split_idx.data_ptr())
            _lib.call("gsr_densify_apply", (_lib.DensifyTensor * len(descs))(*descs), len(descs), ctypes.byref(plan), device=device)
    _install_results(self, new)
    if empty_cache:
        torch.cuda.empty_cache()


def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size):
    """``GaussianModel.densify_and_prune`` (gaussian_model.py:399-413)."""
    if not kernel_takes(self, max_grad, min_opacity, extent, max_screen_size, _lib.capturing()):
        return _reference(self, "densify_and_prune")(self, max_grad, min_opacity, extent, max_screen_size)
    _densify_and_prune_kernels(self, _bounds(self, max_grad, min_opacity, extent, max_screen_size))
