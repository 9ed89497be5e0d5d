"""Writes tests/golden/field/ref_*.npz: recorded runs of the REFERENCE's own ``SuGaR.get_field_values`` and ``SuGaR.compute_density``
(``sugar/sugar_scene/sugar_model.py:1118-1187``, ``:1216-1239``), fp32 on the CPU -- inputs, outputs and autograd gradients.

Build container only (needs the reference tree; ``python tests/golden/make_field_fixtures.py`` from the repository root).  The unbound
methods run on a stub that carries what they read: ``points``, ``scaling``, ``strengths``, ``knn_idx``, ``beta_mode``, a
``get_covariance`` that returns a precomputed matrix (so that it is a leaf with a gradient of its own) and the reference's ``get_beta``.
Gradients are those of ``sum(g_density * density) + sum(g_opacities * closest_gaussian_opacities) [+ sum(g_beta * beta)]`` with recorded
random weights: ``grad_do.*`` without the beta term, ``grad_all.*`` with it.  The reference's ``sdf`` output is recorded but not
differentiated (it yields NaN gradients wherever a density was renormalised to 1)."""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

from shims import reference_env   # noqa: E402

OUT = os.path.join(HERE, "field")
CASES = {"average_k16": dict(P=300, N=257, K=16, beta_mode="average", density_factor=1.0, seed=21),
         "weighted_k16": dict(P=300, N=200, K=16, beta_mode="weighted_average", density_factor=1.0, seed=22),
         "average_k5_factor": dict(P=120, N=130, K=5, beta_mode="average", density_factor=0.7, seed=23),
         # few terms per sum: what the reference's own fp32 gradient does when nothing averages out
         "average_k1": dict(P=40, N=130, K=1, beta_mode="average", density_factor=1.0, seed=24),
         "weighted_k3_factor": dict(P=50, N=130, K=3, beta_mode="weighted_average", density_factor=1.3, seed=25),
         # far fewer samples than Gaussians: most Gaussians are reached only as somebody's far neighbour, where exp() multiplies the
         # rounding of its argument by q / 2
         "average_k16_sparse": dict(P=300, N=64, K=16, beta_mode="average", density_factor=1.0, seed=26)}
LEAVES = ("x", "points", "inv_scaled_rotation", "strengths", "scaling")


def cloud(P, N, K, seed):
    """A cloud in the unit cube with scales near the point spacing, samples scattered around the points, true nearest neighbours."""
    g = np.random.default_rng(seed)
    points = g.uniform(0, 1, (P, 3))
    scaling = np.exp(g.normal(np.log(0.6 * P ** (-1 / 3)), 0.35, (P, 3)))
    q = g.normal(size=(P, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, a, b, c = q.T
    R = np.stack([1 - 2 * (b * b + c * c), 2 * (a * b - w * c), 2 * (a * c + w * b), 2 * (a * b + w * c), 1 - 2 * (a * a + c * c), 2 * (b * c - w * a),
                  2 * (a * c - w * b), 2 * (b * c + w * a), 1 - 2 * (a * a + b * b)], 1).reshape(P, 3, 3)
    M = R / scaling[:, None, :]                                          # R diag(1 / s)
    strengths = 1 / (1 + np.exp(-g.normal(1.0, 1.5, (P, 1))))
    x = points[g.integers(0, P, N)] + g.normal(0, 1.0, (N, 3)) * scaling.mean() * 1.2
    d = ((x[:, None, :] - points[None]) ** 2).sum(-1)
    idx = np.argsort(d, axis=1, kind="stable")[:, :K]
    f = np.float32
    return dict(x=x.astype(f), points=points.astype(f), inv_scaled_rotation=M.astype(f), strengths=strengths.astype(f), scaling=scaling.astype(f),
                idx=idx.astype(np.int64))


def run(SuGaR, name, P, N, K, beta_mode, density_factor, seed):
    data = cloud(P, N, K, seed)
    t = {k: torch.tensor(data[k], requires_grad=True) for k in LEAVES}
    idx = torch.tensor(data["idx"])
    stub = types.SimpleNamespace(points=t["points"], scaling=t["scaling"], strengths=t["strengths"], knn_idx=None, beta_mode=beta_mode,
                                 knn_to_track=K, get_covariance=lambda **kw: t["inv_scaled_rotation"])
    stub.get_beta = types.MethodType(SuGaR.get_beta, stub)
    fields = SuGaR.get_field_values(stub, t["x"], closest_gaussians_idx=idx, density_factor=density_factor, return_sdf=True,
                                    return_closest_gaussian_opacities=True, return_beta=True)
    dens2, opac2 = SuGaR.compute_density(stub, t["x"], closest_gaussians_idx=idx, density_factor=density_factor,
                                         return_closest_gaussian_opacities=True)
    assert torch.equal(dens2, fields["density"]) and torch.equal(opac2, fields["closest_gaussian_opacities"])
    g = np.random.default_rng(seed + 1000)
    ups = {"g_density": g.normal(size=N).astype(np.float32), "g_opacities": g.normal(size=(N, K)).astype(np.float32),
           "g_beta": g.normal(size=N).astype(np.float32)}
    loss_do = (torch.tensor(ups["g_density"]) * fields["density"]).sum() + (torch.tensor(ups["g_opacities"]) * fields["closest_gaussian_opacities"]).sum()
    loss_all = loss_do + (torch.tensor(ups["g_beta"]) * fields["beta"]).sum()
    out = dict(data, beta_mode=np.array(beta_mode), density_factor=np.float64(density_factor), **ups)
    for key in ("density", "closest_gaussian_opacities", "beta", "sdf"):
        out["out." + key] = fields[key].detach().numpy().copy()
    for tag, loss in (("grad_do", loss_do), ("grad_all", loss_all)):
        grads = torch.autograd.grad(loss, [t[k] for k in LEAVES], retain_graph=True, allow_unused=True)
        for k, gr in zip(LEAVES, grads):
            out[f"{tag}.{k}"] = (torch.zeros_like(t[k]) if gr is None else gr).numpy().copy()
            assert np.isfinite(out[f"{tag}.{k}"]).all(), (name, tag, k)
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, f"ref_{name}.npz"), **out)
    d = out["out.density"]
    print(f"{name}: density up to {d.max():.3f}, {100 * (d >= 1).mean():.1f} % at or above 1, opacities up to {out['out.closest_gaussian_opacities'].max():.3f}")


def main():
    with reference_env.reference_tree():
        try:
            import diff_gaussian_rasterization  # noqa: F401
        except ImportError:     # the HIP library is not built: sugar_model.py:9 only needs the two names to exist
            sys.modules["diff_gaussian_rasterization"] = reference_env._Placeholder("diff_gaussian_rasterization")
        from sugar_scene.sugar_model import SuGaR
        for name, case in CASES.items():
            run(SuGaR, name, **case)


if __name__ == "__main__":
    main()
