"""Writes tests/golden/densify/ref_*.npz: recorded runs of the REFERENCE's own ``GaussianModel.densify_and_prune``
(``scene/gaussian_model.py:399-413``) on the CPU -- inputs, what its one ``torch.normal`` call returned, every output.

Build container only (needs the reference tree; ``python tests/golden/make_densify_fixtures.py`` from the repository root).  The
inputs keep every ``max(exp(scaling))`` and ``sigmoid(opacity)`` at least 1e-5 (relative) away from the bound it is compared with,
so that glibc's and the device's ``exp`` classify every row alike: the generator asserts it.  Case "d" carries
``densify_cases.inject_non_finite`` on top; its injected rows are what they are (a NaN, an infinity, exp(0): none of them a rounding
away from another class) and the assertion holds for all the others.  Tags on the command line rewrite those cases only."""
from __future__ import annotations

import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import densify_cases as C   # noqa: E402
from autovfx_amd import densify as D   # noqa: E402
from shims import reference_env   # noqa: E402

ARGS = types.SimpleNamespace(percent_dense=0.01, position_lr_init=1.6e-4, position_lr_final=1.6e-6, position_lr_delay_mult=0.01,
                             position_lr_max_steps=30_000, feature_lr=2.5e-3, opacity_lr=0.05, scaling_lr=5e-3, rotation_lr=1e-3)
CASES = {"a": dict(n=320, seed=11, steps=3, max_screen_size=None, extent=5.3), "b": dict(n=257, seed=12, steps=2, max_screen_size=20, extent=4.1),
         "c": dict(n=64, seed=13, steps=0, max_screen_size=20, extent=6.0),
         "d": dict(n=128, seed=14, steps=1, max_screen_size=20, extent=5.0, non_finite=True)}
MAX_GRAD, MIN_OPACITY = 0.0002, 0.005


def clear_of(values: torch.Tensor, bound: float) -> bool:
    return bool(((values - bound).abs() > 1e-5 * abs(bound)).all())


def run(gm, n, seed, steps, max_screen_size, extent, non_finite=False):
    m = gm.GaussianModel(3)
    for name, t in C.random_tensors(n, 3, seed).items():
        setattr(m, C.ATTRS[name], torch.nn.Parameter(t))
    m.spatial_lr_scale = 1.0
    m.training_setup(ARGS)
    C.train_steps(m, steps)
    C.fill_stats(m, seed + 100)
    plain = torch.ones(n, dtype=torch.bool)
    if non_finite:
        plain[torch.cat(list(C.inject_non_finite(m, MAX_GRAD).values()))] = False
    big = torch.exp(m._scaling.detach()).max(dim=1).values[plain]
    assert clear_of(big, ARGS.percent_dense * extent) and clear_of(big, 0.1 * extent) and clear_of(torch.sigmoid(m._opacity.detach())[plain], MIN_OPACITY)
    child_big = torch.exp(torch.log(torch.exp(m._scaling.detach()) / 1.6)).max(dim=1).values[plain]
    assert clear_of(child_big, 0.1 * extent)
    out = {"max_grad": MAX_GRAD, "min_opacity": MIN_OPACITY, "extent": extent, "percent_dense": ARGS.percent_dense,
           "max_screen_size": -1.0 if max_screen_size is None else float(max_screen_size), "steps": steps}
    for key, t in C.snapshot(m).items():
        out["in." + key] = t.detach().numpy().copy()
    real_normal, recorded = torch.normal, []

    def recording_normal(*a, **k):
        recorded.append(real_normal(*a, **k))
        return recorded[-1]

    torch.manual_seed(seed)
    torch.normal = recording_normal
    try:
        with torch.no_grad():
            m.densify_and_prune(MAX_GRAD, MIN_OPACITY, extent, max_screen_size)
    finally:
        torch.normal = real_normal
    assert len(recorded) == 1
    out["samples"] = recorded[0].numpy().copy()
    for key, t in C.snapshot(m).items():
        out["out." + key] = t.detach().numpy().copy()
    if non_finite:                                   # what the fixture is for: non-finite values among the kept rows and the children
        t = {k: torch.from_numpy(out["in." + k]) for k in ("accum", "denom", "scaling", "opacity")}
        counts = D.plan_host(t["accum"], t["denom"], t["scaling"], t["opacity"], MAX_GRAD, ARGS.percent_dense * extent, MIN_OPACITY,
                             0.1 * extent if max_screen_size else None)["counts"]
        children = out["out.scaling"][int(counts[0] + counts[1]):]
        assert len(children) and not np.isfinite(children).all() and np.isnan(out["out.scaling"]).any() and np.isnan(out["out.opacity"]).any()
    return out


def main():
    assert reference_env.available()
    with reference_env.reference_tree():
        gm = importlib.import_module("scene.gaussian_model")
        for tag, case in CASES.items():
            if sys.argv[1:] and tag not in sys.argv[1:]:
                continue
            out = run(gm, **case)
            os.makedirs(os.path.join(HERE, "densify"), exist_ok=True)
            path = os.path.join(HERE, "densify", f"ref_{tag}.npz")
            np.savez_compressed(path, **out)
            print(path, os.path.getsize(path), "rows", out["in.xyz"].shape[0], "->", out["out.xyz"].shape[0], "samples", out["samples"].shape)


if __name__ == "__main__":
    main()
