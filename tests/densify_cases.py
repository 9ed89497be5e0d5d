"""Shared by tests/test_densify.py and tests/test_densify_gpu.py: a model shaped like the reference's ``GaussianModel`` whose
densification is RESTATED here with the reference's sequence of torch operations (clone ``cat``, split ``cat``, two boolean prunes;
``scene/gaussian_model.py:283-417``) on whatever device its tensors are -- the truth the kernels are held to on the GPU -- and the
builders of its states."""
from __future__ import annotations

import copy

import torch
from torch import nn

from autovfx_amd import densify as D

ATTRS = dict(D.GROUPS)
LRS = {"xyz": 1.6e-4, "f_dc": 2.5e-3, "f_rest": 2.5e-3 / 20.0, "opacity": 0.05, "scaling": 5e-3, "rotation": 1e-3}


class Model:
    """The attributes ``autovfx_amd.densify`` reads and writes, and the reference-shaped methods as ``reference_<name>``."""
    percent_dense = 0.01

    def __init__(self, tensors: dict, opt_cls=torch.optim.Adam):
        for name, attr in D.GROUPS:
            setattr(self, attr, nn.Parameter(tensors[name].clone()))
        n, dev = self._xyz.shape[0], self._xyz.device
        self.xyz_gradient_accum = torch.zeros((n, 1), device=dev)
        self.denom = torch.zeros((n, 1), device=dev)
        self.max_radii2D = torch.zeros(n, device=dev)
        self.optimizer = opt_cls([{"params": [getattr(self, ATTRS[k])], "lr": LRS[k], "name": k} for k in ATTRS], lr=0.0, eps=1e-15)

    # --- the reference's surgery, restated ---
    def _set(self, fn_param, fn_moment):
        for group in self.optimizer.param_groups:
            old = group["params"][0]
            st = self.optimizer.state.get(old, None)
            new = nn.Parameter(fn_param(group["name"], old).requires_grad_(True))
            if st is not None:
                st["exp_avg"], st["exp_avg_sq"] = fn_moment(group["name"], st["exp_avg"]), fn_moment(group["name"], st["exp_avg_sq"])
                del self.optimizer.state[old]
                self.optimizer.state[new] = st
            group["params"][0] = new
            setattr(self, ATTRS[group["name"]], new)

    def _append(self, rows: dict):
        self._set(lambda k, p: torch.cat((p, rows[k]), dim=0), lambda k, m: torch.cat((m, torch.zeros_like(rows[k])), dim=0))
        n, dev = self._xyz.shape[0], self._xyz.device
        self.xyz_gradient_accum, self.denom, self.max_radii2D = torch.zeros((n, 1), device=dev), torch.zeros((n, 1), device=dev), torch.zeros(n, device=dev)

    def _prune(self, mask):
        valid = ~mask
        self._set(lambda k, p: p[valid], lambda k, m: m[valid])
        self.xyz_gradient_accum, self.denom, self.max_radii2D = self.xyz_gradient_accum[valid], self.denom[valid], self.max_radii2D[valid]

    @torch.no_grad()
    def reference_densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size):
        grads = self.xyz_gradient_accum / self.denom
        grads[grads.isnan()] = 0.0
        sel = torch.logical_and(torch.norm(grads, dim=-1) >= max_grad, torch.max(torch.exp(self._scaling), dim=1).values <= self.percent_dense * extent)
        self._append({k: getattr(self, a)[sel] for k, a in ATTRS.items()})
        n = self._xyz.shape[0]
        padded = torch.zeros(n, device=self._xyz.device)
        padded[:grads.shape[0]] = grads.squeeze()
        sel = torch.logical_and(padded >= max_grad, torch.max(torch.exp(self._scaling), dim=1).values > self.percent_dense * extent)
        stds = torch.exp(self._scaling)[sel].repeat(2, 1)
        samples = torch.normal(mean=torch.zeros((stds.size(0), 3), device=stds.device), std=stds)
        rots = D._build_rotation(self._rotation[sel]).repeat(2, 1, 1)
        rows = {k: getattr(self, a)[sel].repeat(2, *([1] * (getattr(self, a).dim() - 1))) for k, a in ATTRS.items()}
        rows["xyz"] = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + self._xyz[sel].repeat(2, 1)
        rows["scaling"] = torch.log(torch.exp(self._scaling)[sel].repeat(2, 1) / (0.8 * 2))
        self._append(rows)
        self._prune(torch.cat((sel, torch.zeros(2 * int(sel.sum()), device=sel.device, dtype=torch.bool))))
        mask = (torch.sigmoid(self._opacity) < min_opacity).squeeze()
        if max_screen_size:
            mask = torch.logical_or(torch.logical_or(mask, self.max_radii2D > max_screen_size),
                                    torch.exp(self._scaling).max(dim=1).values > 0.1 * extent)
        self._prune(mask)
        torch.cuda.empty_cache()

    def reference_add_densification_stats(self, viewspace_point_tensor, update_filter):
        self.xyz_gradient_accum[update_filter] += torch.norm(viewspace_point_tensor.grad[update_filter, :2], dim=-1, keepdim=True)
        self.denom[update_filter] += 1


def random_tensors(n: int, degree: int = 3, seed: int = 0, device="cpu") -> dict:
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    k = (degree + 1) ** 2 - 1
    t = {"xyz": r(n, 3), "f_dc": r(n, 1, 3), "f_rest": r(n, k, 3) * 0.1, "opacity": r(n, 1) * 2.5, "scaling": r(n, 3) * 0.9 - 3.0, "rotation": r(n, 4)}
    return {key: v.to(device) for key, v in t.items()}


def fill_stats(m, seed: int = 1, zero_share: float = 0.4, thr: float = 0.0002) -> None:
    """Two rounds' worth of statistics: ``zero_share`` of the rows never seen (denom 0), gradients spread around ``thr``."""
    n, dev = m._xyz.shape[0], m._xyz.device
    g = torch.Generator().manual_seed(seed)
    seen = (torch.rand(n, 1, generator=g) >= zero_share).float()
    m.denom = (seen * torch.randint(1, 3, (n, 1), generator=g).float()).to(dev)
    m.xyz_gradient_accum = (seen * torch.rand(n, 1, generator=g) * 4 * thr * 2).to(dev)
    m.max_radii2D = (torch.rand(n, generator=g) * 50).to(dev)


def train_steps(m, steps: int) -> None:
    for _ in range(steps):
        loss = sum((getattr(m, a) * getattr(m, a)).sum() for a in ATTRS.values())
        loss.backward()
        m.optimizer.step()
        m.optimizer.zero_grad(set_to_none=True)


def twin(m):
    """A deep copy with its own parameters and optimizer (same class, same state values)."""
    return copy.deepcopy(m)


def snapshot(m) -> dict:
    out = {"accum": m.xyz_gradient_accum, "denom": m.denom, "max_radii2D": m.max_radii2D}
    for group in m.optimizer.param_groups:
        p = group["params"][0]
        assert p is getattr(m, ATTRS[group["name"]]) and type(p) is nn.Parameter and p.requires_grad and p.grad is None and p.is_leaf
        out[group["name"]] = p.detach()
        st = m.optimizer.state.get(p, None)
        if st is not None:
            for key in ("step", "exp_avg", "exp_avg_sq"):
                out[group["name"] + "." + key] = st[key]
    assert len(m.optimizer.state) in (0, 6)
    return out


def assert_same(want: dict, got: dict) -> None:
    assert want.keys() == got.keys()
    for key in want:
        a, b = want[key], got[key]
        assert a.shape == b.shape and a.dtype == b.dtype and a.device == b.device, key
        assert torch.equal(a, b) or (a.float().isnan() == b.float().isnan()).all() and torch.equal(a.nan_to_num(), b.nan_to_num()), key
