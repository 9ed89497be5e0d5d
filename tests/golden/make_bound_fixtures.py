"""Writes tests/golden/bound/ref_*.npz: recorded runs of the REFERENCE's own ``SuGaR.points``, ``SuGaR.scaling`` and ``SuGaR.quaternions``
(``sugar/sugar_scene/sugar_model.py:376-391``, ``:408-423``, ``:425-452``) on a model bound to a surface mesh, fp32 on the CPU -- the inputs,
the three outputs, and the autograd gradients into the vertices, ``_quaternions`` and ``_scales`` for a fixed upstream gradient.

Build container only (needs the reference tree; ``python tests/golden/make_bound_fixtures.py`` from the repository root).  The three
property getters are imported from the mounted tree and run on ``bound_cases.StubSuGaR`` objects, whose own properties are never
reached: the getters are called as ``SuGaR.<name>.fget(stub)``.  pytorch3d is not installed: ``matrix_to_quaternion`` in the reference
module's namespace is ``bound_cases.matrix_to_quaternion`` (the algorithm of pytorch3d 0.7.4, which ``sugar/environment.yml`` pins), and
the stub's ``surface_mesh`` is a ``StubMeshes`` whose ``faces_normals_list`` follows the forward of DESIGN.md 7j in torch.

Cases: a torus of 300 faces with 1, 3, 4 and 6 Gaussians per face, and one case per branch of ``matrix_to_quaternion``: 40 faces whose
frame is a small turn (candidate 0) or a near-half-turn about x, y or z (candidates 1, 2, 3)."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import bound_cases as BC          # noqa: E402
from shims import reference_env   # noqa: E402

OUT = os.path.join(HERE, "bound")
CASES = {**{f"torus_g{G}": lambda G=G: BC.torus_case(15, 10, G, seed=40 + G) for G in (1, 3, 4, 6)},
         **{f"branch_{k}": lambda k=k: BC.branch_case(k, 40, 3, seed=1) for k in range(4)}}


def run(SuGaR, name: str, case: dict) -> None:
    model = BC.StubSuGaR(case, requires_grad=True)
    out = {key: getattr(SuGaR, key).fget(model) for key in BC.OUTPUTS}
    loss = sum((out[key] * torch.from_numpy(case["grad_" + key])).sum() for key in BC.OUTPUTS)
    loss.backward()
    rec = dict(case)
    rec.update({"ref." + key: out[key].detach().numpy() for key in BC.OUTPUTS})
    rec.update({"ref.grad_verts": model._points.grad.numpy(), "ref.grad_complex": model._quaternions.grad.numpy(),
                "ref.grad_log_scales": model._scales.grad.numpy()})
    assert all(v.dtype in (np.float32, np.int64) for v in rec.values())
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, f"ref_{name}.npz")
    np.savez_compressed(path, **rec)
    k = BC.truth(case, grads=False)["q_abs"].argmax(1)
    print(f"{name}: {len(case['faces'])} faces x {case['bary'].shape[0]}, candidates taken {np.bincount(k, minlength=4).tolist()}, "
          f"{os.path.getsize(path)} bytes")


def main():
    with reference_env.reference_tree():
        try:
            import diff_gaussian_rasterization  # noqa: F401
        except ImportError:     # the HIP library is not built: sugar_model.py:9 only needs the two names to exist
            sys.modules["diff_gaussian_rasterization"] = reference_env._Placeholder("diff_gaussian_rasterization")
        import sugar_scene.sugar_model as sugar_model
        sugar_model.matrix_to_quaternion = BC.matrix_to_quaternion
        for name, make in CASES.items():
            run(sugar_model.SuGaR, name, make())


if __name__ == "__main__":
    main()
