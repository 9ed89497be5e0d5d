"""Shared by tests/test_densify.py and tests/test_densify_gpu.py: a model shaped like the reference's ``GaussianModel`` whose
densification is RESTATED here with the reference's sequence of torch operations (clone ``cat``, split ``cat``, two boolean prunes;
``scene/gaussian_model.py:283-417``) on whatever device its tensors are -- the truth the kernels are held to on the GPU -- and the
builders of its states."""
from __future__ import annotations

import copy
import math

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


_INT_OF_SIZE = {2: torch.int16, 4: torch.int32, 8: torch.int64}


def assert_same_tensor(a: torch.Tensor, b: torch.Tensor, key="") -> None:
    """Equal bit patterns outside the NaN positions (so -0.0 is not 0.0 and an infinity is not FLT_MAX), NaN positions the same."""
    assert a.shape == b.shape and a.dtype == b.dtype and a.device == b.device, key
    if not a.dtype.is_floating_point:
        assert torch.equal(a, b), key
        return
    nan = a.isnan()
    assert torch.equal(nan, b.isnan()), key
    bits = lambda t: t.detach().contiguous().view(_INT_OF_SIZE[t.element_size()]).masked_fill(nan, 0)
    assert torch.equal(bits(a), bits(b)), key


def assert_same(want: dict, got: dict) -> None:
    assert want.keys() == got.keys()
    for key in want:
        assert_same_tensor(want[key], got[key], key)


# --- rows the random builders never make: non-finite statistics and parameters, and rows of a chosen class ---

THR, MIN_OP, EXTENT = 0.0002, 0.005, 5.0
_NON_FINITE = {"nan": float("nan"), "+inf": float("inf"), "-inf": -float("inf")}
# (kind, whether the row's gradient is set above the threshold; None: the kind sets the statistics itself)
INJECTIONS = ([(k, None) for k in ("accum.nan", "accum.+inf", "accum.-inf", "accum.negative", "denom.0.accum+", "denom.0.accum0", "denom.nan",
                                   "denom.+inf.accum+inf")]
              + [(f"scaling.{v}.{c}", hot) for v in _NON_FINITE for c in range(3) for hot in (True, False)]
              + [(k, hot) for k in ("scaling.nan0.+inf2", "scaling.exp0", "opacity.nan", "opacity.+inf", "opacity.-inf") for hot in (True, False)])
PINNED = ((0, "accum.nan", None), (63, "denom.0.accum+", None), (64, "scaling.nan.0", True), (1023, "opacity.nan", False), (1024, "scaling.+inf.2", True))


def inject_non_finite(model, thr: float = THR) -> dict:
    """Writes every kind of INJECTIONS into ``model`` in place, one kind per row, on rows a short stride apart (19, less on a small
    model: several land in each wave) and cycling through the kinds as often as the model has room; rows 0, 63, 64, 1023 and 1024 (wave
    and workgroup edges) carry one kind of each of the four tensors.  The scaling and opacity kinds come with a gradient of 3 thr and
    of thr / 4 in turn (denom 1), so that a non-finite scale meets both outcomes of the gradient tests; the accum and denom kinds land
    on the model's own scales (seven in eight above the clone bound of 0.05) and on small ones in turn.  ``scaling.exp0`` is finite: the
    largest scale is exp(0) = 1 on every exp there is, which is ON the clone bound when ``percent_dense * extent`` is 1.
    Returns kind -> rows (int64, on the CPU)."""
    n = model._xyz.shape[0]
    pinned = [p for p in PINNED if p[0] < n]
    taken = {p[0] for p in pinned}
    stride = max(1, min(19, (n - len(taken)) // len(INJECTIONS)))
    assert stride * len(INJECTIONS) <= n, "the model has no room for one row of every kind"
    free = [i for i in range(stride // 2, n, stride) if i not in taken]
    plan = [p + (0,) for p in pinned] + [(i,) + INJECTIONS[j % len(INJECTIONS)] + (j // len(INJECTIONS),) for j, i in enumerate(free)]
    accum, denom = model.xyz_gradient_accum, model.denom
    rows = {}
    with torch.no_grad():
        for i, kind, hot, cycle in plan:
            rows.setdefault(kind, []).append(i)
            if hot is None and cycle % 2:
                model._scaling[i].clamp_(max=-4.0)                       # every other time on a small row (exp(-4) = 0.018)
            if hot is not None:
                accum[i], denom[i] = (3.0 if hot else 0.25) * thr, 1.0
            part = kind.split(".")
            if kind == "accum.negative":
                accum[i], denom[i] = -3.0 * thr, 1.0
            elif part[0] == "accum":
                accum[i], denom[i] = _NON_FINITE[part[1]], 1.0
            elif kind == "denom.0.accum+":
                accum[i], denom[i] = 3.0 * thr, 0.0                      # x / 0 = inf
            elif kind == "denom.0.accum0":
                accum[i], denom[i] = 0.0, 0.0                            # 0 / 0 = NaN: g = 0
            elif kind == "denom.nan":
                accum[i], denom[i] = 3.0 * thr, float("nan")             # g = 0
            elif kind == "denom.+inf.accum+inf":
                accum[i], denom[i] = float("inf"), float("inf")          # inf / inf = NaN: g = 0
            elif kind == "scaling.nan0.+inf2":
                model._scaling[i, 0], model._scaling[i, 2] = float("nan"), float("inf")
            elif kind == "scaling.exp0":
                model._scaling[i] = torch.tensor([-6.0, 0.0, -6.0])
            elif part[0] == "scaling":
                model._scaling[i, int(part[2])] = _NON_FINITE[part[1]]
            else:
                model._opacity[i, 0] = _NON_FINITE[part[1]]
    assert set(rows) == {k for k, _ in INJECTIONS}
    return {k: torch.tensor(v, dtype=torch.int64) for k, v in rows.items()}


def non_finite_model(n: int, degree: int = 3, steps: int = 1, seed: int = 6, device="cpu", opt_cls=torch.optim.Adam):
    """A random model with moments and statistics, and every injection on top.  Returns (model, kind -> rows)."""
    m = Model(random_tensors(n, degree, seed, device), opt_cls)
    train_steps(m, steps)
    fill_stats(m, seed + 1)
    return m, inject_non_finite(m)


KEEP, CLONE, SPLIT, PRUNED, CLONE_PRUNED, SPLIT_PRUNED, WORLD_PRUNED = range(7)


def rows_of_classes(cls, degree: int = 0, seed: int = 0, device="cpu", steps: int = 0, opt_cls=torch.optim.Adam):
    """A model whose row i has the class ``cls[i]`` (KEEP .. WORLD_PRUNED) at THR, MIN_OP, EXTENT, every value well clear of every
    bound: denom 1, a gradient of 3 THR (hot) or THR / 4, scales of 0.002 with one of 0.2 on a split parent (its children: 0.125) and
    one of 0.8 on a row only the world-size bound (0.5) prunes, opacities of 2 (sigmoid 0.88) or -9 (0.00012).  ``plan_host`` is asked
    whether it sees these classes, with and without the world-size bound."""
    cls = torch.as_tensor(cls, dtype=torch.int64).cpu()
    n = cls.numel()
    m = Model(random_tensors(n, degree, seed, device), opt_cls)
    train_steps(m, steps)
    is_ = lambda *which: torch.isin(cls, torch.tensor(which))
    hot, split, dim, wide = is_(CLONE, SPLIT, CLONE_PRUNED, SPLIT_PRUNED), is_(SPLIT, SPLIT_PRUNED), is_(PRUNED, CLONE_PRUNED, SPLIT_PRUNED), is_(WORLD_PRUNED)
    scaling = torch.full((n, 3), math.log(0.002))
    at = torch.arange(n)
    scaling[at[split], at[split] % 3] = math.log(0.2)
    scaling[at[wide], at[wide] % 3] = math.log(0.8)
    with torch.no_grad():
        m._scaling.copy_(scaling)
        m._opacity.copy_(torch.where(dim, -9.0, 2.0).reshape(n, 1))
    m.denom = torch.ones((n, 1), device=device)
    m.xyz_gradient_accum = (torch.where(hot, 3.0, 0.25) * THR).reshape(n, 1).to(device)
    m.max_radii2D = (torch.rand(n, generator=torch.Generator().manual_seed(seed)) * 50).to(device)
    for ws in (None, 0.1 * EXTENT):
        plan = D.plan_host(m.xyz_gradient_accum, m.denom, m._scaling.detach(), m._opacity.detach(), THR, Model.percent_dense * EXTENT, MIN_OP, ws)
        keep = is_(KEEP, CLONE) if ws else is_(KEEP, CLONE, WORLD_PRUNED)
        assert torch.equal(plan["keep"].cpu(), keep) and torch.equal(plan["clone"].cpu(), is_(CLONE)) and torch.equal(plan["split"].cpu(), split)
    return m


def rows_left(cls, mss) -> int:
    """The size of the result: kept originals, a clone beside each cloned row, two children for each surviving split parent."""
    count = torch.bincount(torch.as_tensor(cls, dtype=torch.int64), minlength=7).tolist()
    return count[KEEP] + 2 * count[CLONE] + 2 * count[SPLIT] + (0 if mss else count[WORLD_PRUNED])


def run_layouts(n: int) -> dict:
    """Class lists in which waves (64 rows), quarter workgroups (256) and workgroups (1024) hold one class only, or nothing at all."""
    i = torch.arange(n)
    out = {"mod7": i % 7, "waves": (i // 64) % 7, "quarters": (i // 256) % 7, "workgroups": (i // 1024) % 7}
    for c in range(7):
        out[f"all{c}"] = torch.full((n,), c)
    out["split_tail"] = torch.where(i >= n - 64, SPLIT, KEEP)
    out["clone_ends"] = torch.where((i == 0) | (i == n - 1), CLONE, KEEP)
    return out


def scan_layouts(n: int) -> dict:
    """For more than 256 workgroups (the scan kernel's step): A, clones and splits only in workgroups 255 and 256; B, nothing that
    is counted in the first 256 workgroups and a mix after; C, the mix first and nothing after."""
    i = torch.arange(n)
    seam = (i >= 255 * 1024) & (i < 257 * 1024)
    return {"A": torch.where(seam, 1 + i % 2, KEEP), "B": torch.where(i < 256 * 1024, PRUNED, i % 7), "C": torch.where(i < 256 * 1024, i % 7, PRUNED)}


def seam_layout(keep: int, seed: int = 0, clone: int = 300, split: int = 200, pruned: int = 50) -> torch.Tensor:
    """Shuffled; the result has keep + 2 clone + 2 split rows."""
    cls = torch.cat((torch.full((keep,), KEEP), torch.full((clone,), CLONE), torch.full((split,), SPLIT), torch.full((pruned,), PRUNED)))
    return cls[torch.randperm(cls.numel(), generator=torch.Generator().manual_seed(seed))]


