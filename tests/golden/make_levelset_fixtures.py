"""Writes tests/golden/levelset/ref_*.npz: recorded runs of the REFERENCE's own ``SuGaR.compute_level_surface_points_from_camera_fast``
(``sugar/sugar_scene/sugar_model.py:1719-1954``), fp32 on the CPU -- the stub scene it ran on, what it returned, and the locals the
bars are derived from.

Build container only (needs the reference tree; ``python tests/golden/make_levelset_fixtures.py`` from the repository root).  The
unbound method runs on ``levelset_cases.StubModel`` with ``levelset_cases.StubCamera`` and ``StubRasterizer``: prepared ``zbuf`` /
``pix_to_face``, a pinhole ``unproject_points``.  ``quaternion_apply`` / ``quaternion_invert`` are the helper's (pytorch3d is not
installed), put into the reference module's namespace.  ``torch.randperm`` is wrapped to record its result (``perm``; empty when the
method did not call it).  The method's locals at its return -- the world points, ray directions, standard deviations, neighbour rows and
fp32 densities of the march -- are read with a profile hook (``ref.*``); the interpolated ``t`` and the crossing index of each level come
from one more run per level with the permutation replayed, which returns what the first run returned for that level."""
from __future__ import annotations

import os
import sys
from unittest import mock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import levelset_cases as LC       # noqa: E402
from shims import reference_env   # noqa: E402

OUT = os.path.join(HERE, "levelset")
CASES = {"k16_three_levels": dict(P=300, K=16, H=20, W=24, seed=31, levels=[0.1, 0.3, 0.5], n_surface_points=350, density_factor=1.0),
         "k16_every_pixel": dict(P=300, K=16, H=20, W=24, seed=32, levels=[0.1, 0.3, 0.5], n_surface_points=-1, density_factor=1.0),
         "k3_one_level": dict(P=300, K=3, H=24, W=20, seed=33, levels=[0.3], n_surface_points=300, density_factor=1.0),
         "k16_factor": dict(P=280, K=16, H=20, W=24, seed=34, levels=[0.1, 0.3, 0.5], n_surface_points=10_000, density_factor=0.7)}
KEYS = ("intersection_points", "pixel_idx", "gaussian_idx", "normals")


def run_reference(SuGaR, sc, levels, n_surface_points, density_factor, replay=None):
    """(outputs, locals at return, the permutation drawn or None)."""
    model = LC.StubModel(sc)
    rasterizer = LC.StubRasterizer(sc["zbuf"], sc["pix_to_face"])
    method = SuGaR.compute_level_surface_points_from_camera_fast
    seen, perms, real_randperm = {}, [], torch.randperm

    def randperm(n, *a, **k):
        perms.append(real_randperm(n, *a, **k) if replay is None else torch.tensor(replay))
        assert len(perms[-1]) == n
        return perms[-1]

    def profile(frame, event, arg):
        if event == "return" and frame.f_code is method.__code__:
            seen.update(frame.f_locals)

    with mock.patch("torch.randperm", randperm), torch.no_grad():
        sys.setprofile(profile)
        try:
            out = method(model, nerf_cameras=model.cameras, cam_idx=0, rasterizer=rasterizer, surface_levels=levels,
                         n_surface_points=n_surface_points, density_factor=density_factor, return_pixel_idx=True, return_gaussian_idx=True,
                         return_normals=True)
        finally:
            sys.setprofile(None)
    assert rasterizer.calls == 1 and len(perms) <= 1
    return out, seen, (perms[0].numpy() if perms else None)


def run(SuGaR, name, P, K, H, W, seed, levels, n_surface_points, density_factor):
    sc = LC.scene(P, K, H, W, seed)
    torch.manual_seed(seed)
    out, loc, perm = run_reference(SuGaR, sc, levels, n_surface_points, density_factor)
    n, S = loc["densities"].shape
    rec = dict(sc, levels=np.asarray(levels, np.float64), n_surface_points=np.int64(n_surface_points), density_factor=np.float64(density_factor),
               n_points_in_range=np.int64(S), range_size=np.float64(3.0), perm=np.zeros(0, np.int64) if perm is None else perm)
    rec["ref.origins"], rec["ref.dirs"] = loc["all_world_points"].numpy(), loc["camera_to_samples"].numpy()
    rec["ref.stds"], rec["ref.idx"], rec["ref.densities"] = loc["points_stds"].numpy(), loc["closest_gaussians_idx"].numpy(), loc["densities"].numpy()
    assert np.array_equal(loc["points_range"][..., 0].numpy(), torch.linspace(-3.0, 3.0, S).numpy()[None] * rec["ref.stds"][:, None])
    hit, a, t = np.zeros((len(levels), n), np.uint8), np.zeros((len(levels), n), np.int64), np.zeros((len(levels), n), np.float32)
    for l, level in enumerate(levels):
        for key in KEYS:
            rec[f"out{l}.{key}"] = out[level][key].numpy().copy()
        one, loc1, _ = run_reference(SuGaR, sc, [level], n_surface_points, density_factor, replay=perm)
        assert all(torch.equal(one[level][key], out[level][key]) for key in KEYS)
        keep = ~loc1["empty_pixels"].numpy()
        hit[l] = keep
        a[l][keep] = loc1["valid_first_point_above_level"].numpy()[:, 0]
        t[l][keep] = loc1["intersection_t"].numpy()
    rec["ref.hit"], rec["ref.a"], rec["ref.t"] = hit, a, t
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, f"ref_{name}.npz")
    np.savez_compressed(path, **rec)
    d = rec["ref.densities"]
    print(f"{name}: {n} rays of {H * W} pixels, densities up to {d.max():.3f}, {100 * (d >= 1).mean():.1f} % renormalised, hits per level "
          f"{hit.sum(1).tolist()}, {os.path.getsize(path)} bytes")


def main():
    with reference_env.reference_tree():
        try:
            import diff_gaussian_rasterization  # noqa: F401
        except ImportError:     # the HIP library is not built: sugar_model.py:9 only needs the two names to exist
            sys.modules["diff_gaussian_rasterization"] = reference_env._Placeholder("diff_gaussian_rasterization")
        import sugar_scene.sugar_model as sugar_model
        sugar_model.quaternion_apply, sugar_model.quaternion_invert = LC.quaternion_apply, LC.quaternion_invert
        for name, case in CASES.items():
            run(sugar_model.SuGaR, name, **case)


if __name__ == "__main__":
    main()
