"""The optimizer of the reference's Gaussian training loops, ``torch.optim.Adam`` (``scene/gaussian_model.py:159-177``), in one launch.

:class:`Adam` is ``torch.optim.Adam``: the same constructor, ``param_groups``, ``state`` layout, ``state_dict()`` and
``load_state_dict()``, so checkpoints load in both directions.  Its ``step()`` computes torch's default GPU update (the foreach path,
``_multi_tensor_adam``) bit for bit, but as ONE kernel over every parameter of every group (``gsr_adam.hip``, C ABI
``gsr_adam_step``) instead of about seven foreach kernels per group.  Nothing is cached between steps: the reference
swaps parameters and edits ``exp_avg`` / ``exp_avg_sq`` in place during densification, so every step reads ``param_groups`` and
``state`` afresh.  The kernel writes through raw pointers, so the version counters of the tensors it wrote are bumped afterwards,
as an in-place op would bump them (the rasterizer binding's geometry reuse and the raw-parameter memo key on them).

The kernel takes a step when :func:`kernel_takes` says so: amsgrad, maximize, capturable, differentiable and fused off, no weight
decay, ``foreach`` not ``False``, numeric ``lr`` / betas / eps, beta1 > 0.5, dense contiguous fp32 parameters, gradients and moments on one GPU,
no graph capture.  Every other step is torch's own ``Adam.step``: torch's result or torch's exception.
"""
from __future__ import annotations

import ctypes
from typing import Iterable, List

import torch
from torch.optim.optimizer import _get_value

from . import _lib

__all__ = ["Adam", "kernel_takes", "from_torch_adam"]

_PARAM_TYPES = (torch.Tensor, torch.nn.Parameter)   # torch's foreach default applies to exactly these (_foreach_supported_types)
_OFF = ("amsgrad", "maximize", "capturable", "differentiable", "fused")


def _f32(x: float) -> float:
    return ctypes.c_float(x).value


def _plain_number(x) -> bool:
    return isinstance(x, (int, float)) and not isinstance(x, bool)   # numpy's float64 (the lr schedule's) is a float


def _dense_fp32(t, device_type: str, device=None) -> bool:
    """A dense, contiguous fp32 tensor on a device of ``device_type`` (on ``device`` if given)."""
    return (isinstance(t, torch.Tensor) and t.layout == torch.strided and t.dtype == torch.float32 and t.device.type == device_type
            and (device is None or t.device == device) and t.is_contiguous() and not t.is_neg() and not t.is_conj())


def kernel_takes(param_groups: Iterable[dict], state, capturing: bool = False, device_type: str = "cuda") -> bool:
    """Whether one ``gsr_adam_step`` launch computes this step exactly as ``torch.optim.Adam.step`` would.  Host only (reads
    attributes, launches nothing).  ``state``: the optimizer's ``state`` mapping; moments that exist must match their parameter.
    ``device_type``: where the kernel runs ("cuda", a HIP device); tests pass "meta" to walk the rules without a GPU."""
    if capturing:
        return False
    device = None
    for group in param_groups:
        if any(group.get(k, False) for k in _OFF) or group.get("foreach") is False:
            return False
        if not _plain_number(group.get("weight_decay")) or group["weight_decay"] != 0:
            return False
        betas = group.get("betas")
        if not (isinstance(betas, (tuple, list)) and len(betas) == 2 and all(map(_plain_number, betas))):
            return False
        if not 0.0 <= _f32(1 - betas[0]) < 0.5:   # gsr_adam_step's range: beta1 <= 0.5 is ATen's other lerp branch, beta1 > 1 no Adam
            return False
        if not (_plain_number(group.get("lr")) and _plain_number(group.get("eps"))):
            return False
        for p in group["params"]:
            g = p.grad
            if g is None:
                continue
            if type(p) not in _PARAM_TYPES or not _dense_fp32(p, device_type, device) or not _dense_fp32(g, device_type, p.device) or g.shape != p.shape:
                return False
            device = p.device
            st = state.get(p) if hasattr(state, "get") else None
            if st:
                step, m, v = st.get("step"), st.get("exp_avg"), st.get("exp_avg_sq")
                if not (isinstance(step, torch.Tensor) and step.device.type == "cpu" and step.dtype == torch.float32 and step.numel() == 1):
                    return False
                if not (_dense_fp32(m, device_type, device) and _dense_fp32(v, device_type, device) and m.shape == p.shape and v.shape == p.shape):
                    return False
    return device is not None


def _torch_step(opt: torch.optim.Adam):
    """torch's ``Adam.step`` without its profiling / hook wrapper (ours already ran it)."""
    fn = torch.optim.Adam.step
    if getattr(fn, "hooked", False):
        fn = fn.__wrapped__
    return fn(opt)


class Adam(torch.optim.Adam):
    """``torch.optim.Adam`` with its default update fused into one HIP launch per step (see the module docstring)."""

    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if not kernel_takes(self.param_groups, self.state, _lib.capturing()):
            _torch_step(self)
            return loss
        with torch.no_grad():
            self._kernel_step()
        return loss

    def _kernel_step(self) -> None:
        batches = {}                 # (w, b2, c, eps) -> descriptors sharing those scalars
        written: List[torch.Tensor] = []
        all_steps: List[torch.Tensor] = []
        device = None
        for group in self.param_groups:
            params, grads, exp_avgs, exp_avg_sqs, max_exp_avg_sqs, steps = [], [], [], [], [], []
            self._init_group(group, params, grads, exp_avgs, exp_avg_sqs, max_exp_avg_sqs, steps)   # torch's own lazy state
            if not params:
                continue
            device = params[0].device
            all_steps += steps
            beta1, beta2 = group["betas"]
            lr = group["lr"]
            key = (_f32(1 - beta1), _f32(beta2), _f32(1 - beta2), _f32(group["eps"]))
            out = batches.setdefault(key, [])
            for p, g, m, v, step in zip(params, grads, exp_avgs, exp_avg_sqs, steps):
                # the count torch's fp32 `step += 1` gives (the exact double sum rounded once to fp32), read from a CPU tensor without
                # advancing it yet: the counters move only once every launch went out
                t = _f32(_get_value(step) + 1.0)
                step_size = (lr / (1 - beta1 ** t)) * -1   # torch's doubles, in torch's order
                bias2_sqrt = (1 - beta2 ** t) ** 0.5
                out.append(_lib.AdamTensor(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), step_size, bias2_sqrt))
                written += (p, m, v)
        if device is None:
            return
        with torch.cuda.device(device):
            for (w, b2, c, eps), descs in batches.items():
                for i in range(0, len(descs), _lib.ADAM_MAX_TENSORS):
                    part = descs[i:i + _lib.ADAM_MAX_TENSORS]
                    _lib.call("gsr_adam_step", (_lib.AdamTensor * len(part))(*part), len(part), w, b2, c, eps, device=device)
        torch._foreach_add_(all_steps, torch.tensor(1.0, device="cpu"), alpha=1.0)   # as torch increments CPU steps
        torch.autograd.graph.increment_version(written)


def from_torch_adam(opt: torch.optim.Optimizer) -> torch.optim.Optimizer:
    """``opt`` as this package's :class:`Adam` -- the same ``param_groups`` (the same dictionaries), defaults and state -- when it is
    exactly a ``torch.optim.Adam``; anything else is returned as it is."""
    if type(opt) is not torch.optim.Adam:
        return opt
    ours = Adam(opt.param_groups, **opt.defaults)
    ours.state.update(opt.state)
    return ours

