"""Shared by test_field.py and test_field_gpu.py: the fixtures of tests/golden/field (recorded runs of the reference's own
``SuGaR.get_field_values``), the float64 truth of autovfx_amd.field's contract, and the bars both tests hold results to.

Truth: a dense torch restatement in float64 (gather, batched product, clamp, exp, sum; slots outside ``[0, P)`` masked), gradients by
autograd.

Bars.  Forward, per output tensor: 4 x the largest error of the reference's own fp32 CPU result against the truth,
absolute (opacities reach 1e-268 in float64: a relative error per element means nothing).  On a fixture that is the fixture's own figure;
on any other case it is the largest figure of the fixtures relative to the tensor's largest magnitude, times the case's largest magnitude.
The factor 4 covers a 2-ulp device ``expf`` against glibc's and another order of the 3-term products and the K-term sum.
Gradients, per element: ``c (n_terms + 3) 2^-24 sum|terms|`` against float64 autograd, where the terms are the products that are summed
into the element (``M[b][a] dw_a`` for positions, ``s_b dw_a`` for the matrix, ``G f e`` for the strength, ``g_beta / K`` for the minimum
scale) and ``c`` is, per gradient tensor, 4 x the largest ratio the reference's own fp32 gradient reaches on the fixtures."""
from __future__ import annotations

import glob
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "field")
FIXTURES = sorted(os.path.basename(p)[len("ref_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "ref_*.npz")))
GRADS = ("x", "centers", "inv_scaled_rotation", "strengths", "min_scaling")
EPS = 2.0 ** -24
_cache: dict = {}


def fixture(name: str) -> dict:
    if name not in _cache:
        with np.load(os.path.join(GOLDEN, f"ref_{name}.npz")) as z:
            d = {k: z[k] for k in z.files}
        d["beta_mode"] = str(d["beta_mode"])
        d["density_factor"] = float(d["density_factor"])
        d["min_scaling"] = d["scaling"].min(axis=1)
        _cache[name] = d
    return _cache[name]


def scaling_grad_to_min(fx: dict, grad_scaling: np.ndarray) -> np.ndarray:
    """The reference's gradient of ``scaling [P,3]`` read at each row's minimum: the gradient of ``min_scaling``."""
    return grad_scaling[np.arange(len(grad_scaling)), fx["scaling"].argmin(axis=1)]


def truth(x, idx, centers, M, strengths, min_scaling=None, density_factor=1.0, g_density=None, g_opacities=None, g_beta=None) -> dict:
    """float64: outputs, autograd gradients, and per gradient element the number of terms and the sum of their magnitudes."""
    f = torch.float64
    x, c, M, sg = (torch.tensor(np.asarray(a, np.float64), dtype=f, requires_grad=True) for a in (x, centers, M, np.asarray(strengths).reshape(-1)))
    ms = None if min_scaling is None else torch.tensor(np.asarray(min_scaling, np.float64), requires_grad=True)
    idx = torch.tensor(np.asarray(idx, np.int64))
    N, K = idx.shape
    P = c.shape[0]
    valid = (idx >= 0) & (idx < P)
    j = idx.clamp(0, max(P - 1, 0))
    s = x[:, None, :] - c[j]
    w = (M[j].transpose(-1, -2) @ s[..., None])[..., 0]
    q_raw = (w * w).sum(-1)
    e = torch.exp(-0.5 * q_raw.clamp(0.0, 1e8))
    o = torch.where(valid, density_factor * sg[j] * e, torch.zeros((), dtype=f))
    out = {"density": o.sum(-1), "opacities": o, "beta": None if ms is None else torch.where(valid, ms[j], torch.zeros((), dtype=f)).sum(-1) / K}
    z = lambda a, shape: torch.zeros(shape, dtype=f) if a is None else torch.tensor(np.asarray(a, np.float64))
    gd, go, gb = z(g_density, (N,)), z(g_opacities, (N, K)), z(g_beta, (N,))
    loss = (gd * out["density"]).sum() + (go * o).sum() + (0 if ms is None else (gb * out["beta"]).sum())
    leaves = [x, c, M, sg] + ([ms] if ms is not None else [])
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    grad = {k: (torch.zeros_like(t) if g is None else g).numpy() for k, t, g in zip(GRADS, leaves, grads)}
    with torch.no_grad():
        G = gd[:, None] + go
        dq = torch.where(valid & (q_raw <= 1e8), -0.5 * G * o, torch.zeros((), dtype=f))
        dw = 2.0 * w * dq[..., None]
        t_ds = (M[j] * dw[..., None, :]).abs().sum(-1)                  # [N,K,3]: sum_a |M[b][a] dw_a|
        t_dM = (s[..., :, None] * dw[..., None, :]).abs()               # [N,K,3,3]
        t_sig = torch.where(valid, (G * density_factor * e).abs(), torch.zeros((), dtype=f))
        t_m = torch.where(valid, (gb / K).abs()[:, None].expand(N, K), torch.zeros((), dtype=f))
        flat = j.reshape(-1)
        add = lambda t, shape: torch.zeros(shape, dtype=f).index_add_(0, flat, t.reshape((N * K,) + tuple(shape[1:])))
        count = add(valid.to(f), (P,))
        total = {"x": (t_ds * valid[..., None]).sum(1), "centers": add(t_ds * valid[..., None], (P, 3)), "inv_scaled_rotation": add(t_dM * valid[..., None, None], (P, 3, 3)),
                 "strengths": add(t_sig, (P,)), "min_scaling": add(t_m, (P,))}
        n = {"x": 3 * valid.sum(1).to(f)[:, None].expand(N, 3), "centers": 3 * count[:, None].expand(P, 3), "inv_scaled_rotation": count[:, None, None].expand(P, 3, 3),
             "strengths": count, "min_scaling": count}
    out = {k: (None if v is None else v.detach().numpy()) for k, v in out.items()}
    out.update(grad=grad, unit={k: ((n[k] + 3) * EPS * total[k]).numpy() for k in total})
    return out


def fixture_truth(name: str, with_beta: bool) -> dict:
    """The truth of a fixture's call; ``with_beta``: the beta output and its upstream gradient included (``'average'`` fixtures)."""
    key = (name, with_beta)
    if key not in _cache:
        fx = fixture(name)
        _cache[key] = truth(fx["x"], fx["idx"], fx["points"], fx["inv_scaled_rotation"], fx["strengths"], fx["min_scaling"] if with_beta else None,
                            fx["density_factor"], fx["g_density"], fx["g_opacities"], fx["g_beta"] if with_beta else None)
    return _cache[key]


def reference_grads(name: str, with_beta: bool) -> dict:
    """The reference's fp32 gradients of a fixture under the op's names."""
    fx = fixture(name)
    tag = "grad_all" if with_beta else "grad_do"
    out = {"x": fx[tag + ".x"], "centers": fx[tag + ".points"], "inv_scaled_rotation": fx[tag + ".inv_scaled_rotation"],
           "strengths": fx[tag + ".strengths"].reshape(-1)}
    if with_beta:
        out["min_scaling"] = scaling_grad_to_min(fx, fx[tag + ".scaling"])
    return out


def _fixture_calls():
    return [(name, with_beta) for name in FIXTURES for with_beta in ((False, True) if fixture(name)["beta_mode"] == "average" else (False,))]


def reference_forward_errors(name: str) -> dict:
    """Largest absolute error of the reference's own fp32 outputs on a fixture (beta only where the op computes it)."""
    fx = fixture(name)
    avg = fx["beta_mode"] == "average"
    t = fixture_truth(name, avg)
    err = {"density": np.abs(fx["out.density"] - t["density"]).max(), "opacities": np.abs(fx["out.closest_gaussian_opacities"] - t["opacities"]).max()}
    if avg:
        err["beta"] = np.abs(fx["out.beta"] - t["beta"]).max()
    return err


def forward_bars(name: str) -> dict:
    return {k: 4.0 * v for k, v in reference_forward_errors(name).items()}


def forward_bars_relative() -> dict:
    """Per output: the largest forward bar of the fixtures relative to the tensor's largest magnitude there."""
    if "rel" not in _cache:
        rel: dict = {}
        for name in FIXTURES:
            t = fixture_truth(name, fixture(name)["beta_mode"] == "average")
            for k, bar in forward_bars(name).items():
                rel[k] = max(rel.get(k, 0.0), bar / np.abs(t[k]).max())
        _cache["rel"] = rel
    return _cache["rel"]


def gradient_factors() -> dict:
    """``c`` per gradient tensor: 4 x the largest error / unit ratio of the reference's own fp32 gradients over the fixtures."""
    if "c" not in _cache:
        c: dict = {}
        for name, with_beta in _fixture_calls():
            t, ref = fixture_truth(name, with_beta), reference_grads(name, with_beta)
            for k, g in ref.items():
                unit = t["unit"][k]
                live = unit > 0
                c[k] = max(c.get(k, 0.0), 4.0 * float((np.abs(g - t["grad"][k])[live] / unit[live]).max()))
        _cache["c"] = c
    return _cache["c"]


def check_forward(got: dict, want: dict, bars: dict = None, label: str = "") -> None:
    """``got`` / ``want``: density, opacities, beta (None = not computed).  ``bars`` None: the fixtures' relative bars at this case's scale."""
    for k in ("density", "opacities", "beta"):
        if got.get(k) is None:
            continue
        scale = float(np.abs(want[k]).max()) if want[k].size else 0.0
        bar = bars[k] if bars is not None else forward_bars_relative()[k] * scale
        err = float(np.abs(np.asarray(got[k], np.float64) - want[k]).max()) if want[k].size else 0.0
        print(f"{label} {k}: error {err:.3e}, bar {bar:.3e}, scale {scale:.3e}")
        assert err <= bar, (label, k, err, bar)


def check_grads(got: dict, want: dict, label: str = "") -> None:
    """``got``: name -> array (only those present are checked); ``want``: a ``truth`` result."""
    c = gradient_factors()
    for k, g in got.items():
        if g is None:
            continue
        g = np.asarray(g, np.float64).reshape(want["grad"][k].shape)
        err, bound = np.abs(g - want["grad"][k]), c[k] * want["unit"][k]
        ratio = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
        print(f"{label} d{k}: largest error / bound {ratio:.3f} (c = {c[k]:.2f})")
        assert np.all(err <= bound), (label, k, ratio)
