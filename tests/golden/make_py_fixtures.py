"""Generate tests/golden/pypin/*.npz from the REFERENCE's own importable Python.  Run where the reference tree is mounted:

    python tests/golden/make_py_fixtures.py

The preprocess stage (K1) has restatements in the reference's Python: ``utils/sh_utils.py:eval_sh`` (render()'s
``convert_SHs_python`` branch), ``build_covariance_from_scaling_rotation`` / ``get_covariance`` (the ``compute_cov3D_python``
branch) and ``getWorld2View2`` / ``getProjectionMatrix`` / ``Camera`` (the matrices the rasterizer receives).  Each case builds a
reference ``GaussianModel`` from raw parameters and a reference ``Camera``, drives the reference's own
``gaussian_renderer.render()`` against a recording double of the rasterizer -- once with both Python-prep switches on, once
plain -- and stores:

* the raw parameters (``raw_*``) and the getters' outputs (``get_*``); the plain call must hand the rasterizer exactly these;
* the argument tuple of the Python-prep call: ``cov3D_precomp``, ``colors_precomp``, ``viewmatrix``, ``projmatrix``,
  ``campos``, ``tanfovx`` / ``tanfovy``, ``bg``, ``scale_modifier``, ``sh_degree``, ``image_width`` / ``image_height``;
* fp64 truths from the reference's own functions on the fp32 values the rasterizer receives: ``truth_sh_pre`` =
  ``eval_sh`` + 0.5 before the clamp, ``truth_sh_scale`` = 0.5 + sum_k |Y_k(d) sh_k| (the basis values Y_k from ``eval_sh``
  on one-hot coefficients), ``truth_cov3D`` = the model's ``covariance_activation`` (what ``get_covariance`` calls) of
  ``get_scaling``, ``float32(scale_modifier)`` and ``_rotation``, with its tensor factories forced to float64.

``cameras.npz`` holds more camera poses (translate / scale, non-square FoV, orbit poses) with the reference's matrices.
``build()`` returns every array without writing, for the drift test in tests/test_py_pin.py.
"""
import math
import os
import sys
from unittest import mock

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from autovfx_amd.cameras import focal2fov, fov2focal, orbit_c2w  # noqa: E402
from test_render_mirror import _RecordingRasterizer, _import_reference  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pypin")
C0 = 0.28209479177387814


class _on_cpu:
    """The reference hard-codes device='cuda' in tensor factories and calls ``.cuda()``; run it all on the CPU.  With
    ``f64`` the factories also make float64 tensors (whatever dtype the call asks for), for the fp64 truths."""

    def __init__(self, f64=False):
        self.f64 = f64

    def __enter__(self):
        real_zeros, real_like = torch.zeros, torch.zeros_like
        f64 = self.f64

        def zeros(*a, **k):
            k.pop("device", None)
            if f64:
                k["dtype"] = torch.float64
            return real_zeros(*a, **k)

        def zeros_like(t, **k):
            k.pop("device", None)
            return real_like(t, **k)

        self.ps = [mock.patch("torch.zeros", zeros), mock.patch("torch.zeros_like", zeros_like),
                   mock.patch("torch.Tensor.cuda", lambda t, *a, **k: t)]
        for p in self.ps:
            p.start()

    def __exit__(self, *a):
        for p in self.ps:
            p.stop()


# ---- cameras ----------------------------------------------------------------------------------------------------------------

def _orbit_pose(i, n=8, radius=4.0, theta=30.0):
    c2w = orbit_c2w(radius, n, theta)[i]
    w2c = np.linalg.inv(c2w)
    return np.transpose(w2c[:3, :3]), w2c[:3, 3]


def camera_specs():
    """(name, R, T, trans, scale, FoVx, FoVy, W, H): R / T as the reference's Camera takes them (R = camera-to-world rotation)."""
    specs = []
    for i, (W, H) in zip((1, 2, 5, 6), ((64, 48), (80, 45), (48, 64), (96, 40))):
        R, T = _orbit_pose(i)
        fovx = math.radians(60.0)
        specs.append((f"orbit{i}", R, T, np.zeros(3), 1.0, fovx, focal2fov(fov2focal(fovx, W), H), W, H))
    # looking along world +z from a centre set by translate / scale; non-square FoV (fy != fx)
    specs.append(("axis_trans_scale", np.eye(3), np.array([0.3, -0.2, 4.0]), np.array([0.25, -0.5, 1.5]), 1.3, 1.1, 0.7, 72, 40))
    # a tilted pose with translate / scale
    R, T = _orbit_pose(3, n=8, radius=3.0, theta=50.0)
    specs.append(("tilted_trans_scale", R, T, np.array([-1.0, 0.5, 0.25]), 0.8, 0.9, 1.2, 40, 56))
    return specs


def reference_camera(spec):
    cams = _import_reference("scene.cameras")
    name, R, T, trans, scale, fovx, fovy, W, H = spec
    with _on_cpu():
        cam = cams.Camera(colmap_id=0, R=R, T=T, FoVx=fovx, FoVy=fovy, image=None, gt_alpha_mask=None, image_name=name, uid=0,
                          trans=trans, scale=scale, data_device="cpu", image_height=H, image_width=W)
    return cam


def camera_arrays(spec):
    gu = _import_reference("utils.graphics_utils")
    cam = reference_camera(spec)
    name, R, T, trans, scale, fovx, fovy, W, H = spec
    return {"R": np.asarray(R, np.float64), "T": np.asarray(T, np.float64), "trans": np.asarray(trans, np.float64),
            "scale": np.float64(scale), "FoVx": np.float64(fovx), "FoVy": np.float64(fovy), "znear": np.float64(cam.znear),
            "zfar": np.float64(cam.zfar), "width": np.int32(W), "height": np.int32(H),
            "getWorld2View2": gu.getWorld2View2(R, T, trans, scale),
            "getProjectionMatrix": gu.getProjectionMatrix(cam.znear, cam.zfar, fovx, fovy).numpy(),
            "world_view_transform": cam.world_view_transform.numpy(), "projection_matrix": cam.projection_matrix.numpy(),
            "full_proj_transform": cam.full_proj_transform.numpy(), "camera_center": cam.camera_center.numpy()}


# ---- clouds -----------------------------------------------------------------------------------------------------------------

def _in_view(g, cam, P, z=(1.0, 8.0)):
    """P points inside the camera's frustum (view-space depth in ``z``), in world coordinates (float64)."""
    wv = cam.world_view_transform.numpy().astype(np.float64).T      # w2c
    c2w = np.linalg.inv(wv)
    tx, ty = math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)
    d = np.exp(g.uniform(np.log(z[0]), np.log(z[1]), P))
    v = np.stack((g.uniform(-0.95, 0.95, P) * tx * d, g.uniform(-0.95, 0.95, P) * ty * d, d, np.ones(P)), 1)
    return (v @ c2w.T)[:, :3]


def cloud(g, cam, P, M, kind="plain"):
    """Raw parameters as a trained model holds them: log scales, un-normalised quaternions, opacity logits, SH with a DC
    term that often drives a channel below zero (the clamp)."""
    xyz = _in_view(g, cam, P)
    ls = g.normal(-3.4, 0.5, (P, 3))
    rot = g.standard_normal((P, 4)) * g.uniform(0.5, 2.0, (P, 1))
    op = g.normal(0.0, 1.5, (P, 1))
    dc = g.normal(0.3, 0.9, (P, 1, 3))
    dc[::7] = -2.5 + g.normal(0.0, 0.5, (len(dc[::7]), 1, 3))                    # negative before the clamp
    dc[3::11] = -0.5 / C0 + g.normal(0.0, 0.02, (len(dc[3::11]), 1, 3))            # close to the clamp
    band = np.array([1.0] * 3 + [0.7] * 5 + [0.5] * 7)[:M - 1]
    rest = g.standard_normal((P, M - 1, 3)) * 0.3 * band[None, :, None]
    if kind == "edges":
        n = 0
        axis = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [-1, 0, 0, 0], [0, -1, 0, 0]], np.float64)
        rot[n:n + 6] = axis; n += 6
        rot[n:n + 6] = axis * 1.7; n += 6                                              # axis-aligned, not unit
        rot[n:n + 4] = [[1, 1e-7, -1e-8, 1e-9], [-1.7, 2e-7, 0, -1e-7], [0.3, 1e-6, 1e-6, 1e-6], [1e-3, 0, 0, 0]]; n += 4
        rot[n:n + 40, 0] = -np.abs(rot[n:n + 40, 0]); n += 40                          # negative w
        rot[n:] *= 1.7                                                                 # the rest: 1.7 times their norm
        ls[60:90] = np.linspace(-12.0, 3.0, 30)[:, None] + g.normal(0.0, 0.01, (30, 3))   # log-scales -12 .. 3
        for k, a in enumerate((1e1, 1e2, 1e3, 1e4)):                                    # anisotropy up to 1e4
            rows = slice(90 + 8 * k, 98 + 8 * k)
            ls[rows] = -2.5
            ls[rows, k % 3] -= math.log(a)
    if kind == "aniso":
        ls[:, :] = g.uniform(-12.0, 3.0, (P, 1)) + g.normal(0.0, 0.05, (P, 3))
        ls[::2, 2] = ls[::2, 0] - np.log(g.uniform(1.0, 1e4, len(ls[::2])))
        ls[1::4, 1] = ls[1::4, 0] + np.log(1e4)
        ls = np.clip(ls, -12.0, 3.0)
    f = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float32)
    return {"_xyz": f(xyz), "_scaling": f(ls), "_rotation": f(rot), "_opacity": f(op), "_features_dc": f(dc), "_features_rest": f(rest)}


def axis_cloud(g, cam, P, M):
    """Gaussians on the lines through the camera centre: exact zeros in the view direction.  The camera looks along world
    +z, so centre + t e_z (two zero components) and centre + t (a, 0, 1), centre + t (0, a, 1) (one) are in view; a few
    1e-3 from the centre (behind the near plane) and 1e3 away."""
    raw = cloud(g, cam, P, M)
    c = cam.camera_center.numpy().astype(np.float64)
    t = np.concatenate(([1e-3, 2e-3, 0.3, 1e3, 1e3], np.exp(g.uniform(np.log(0.5), np.log(20.0), 55))))
    a = g.uniform(-0.4, 0.4, len(t))
    d = np.zeros((3 * len(t), 3))
    d[0::3, 2] = 1.0
    d[1::3] = np.stack((a, 0 * a, np.ones_like(a)), 1)
    d[2::3] = np.stack((0 * a, a, np.ones_like(a)), 1)
    pts = c[None] + np.repeat(t, 3)[:, None] * d
    pts[0::3, :2] = c[:2]       # keep the two components exactly the centre's (so p - campos is exactly 0 there)
    pts[1::3, 1] = c[1]
    pts[2::3, 0] = c[0]
    n = len(pts)
    raw["_xyz"][:n] = torch.tensor(pts, dtype=torch.float32)
    ls = raw["_scaling"]
    ls[3:15] = torch.log(torch.tensor(10.0)) + ls[3:15] * 0.1       # the far ones big enough to cover a pixel
    return raw


# ---- one case ---------------------------------------------------------------------------------------------------------------

def cases():
    """(name, camera spec index, max_sh_degree, active degree, P, scale_modifier, kind, seed)."""
    return [("sh3_edges", 0, 3, 3, 400, 1.0, "edges", 1),
            ("sh3_active0", 1, 3, 0, 120, 1.0, "plain", 2),
            ("sh3_active1", 2, 3, 1, 120, 1.0, "plain", 3),
            ("sh3_active2", 3, 3, 2, 120, 1.0, "plain", 4),
            ("m1_deg0", 1, 0, 0, 150, 1.0, "plain", 5),
            ("m4_deg1", 2, 1, 1, 150, 1.0, "plain", 6),
            ("m9_deg2", 0, 2, 2, 150, 1.0, "plain", 7),
            ("axis_dirs_mod05", 4, 3, 3, 240, 0.5, "axis", 8),
            ("aniso_mod17", 5, 3, 3, 260, 1.7, "aniso", 9)]


def run_case(name, cam_index, max_deg, active, P, mod, kind, seed):
    gr = _import_reference("gaussian_renderer")
    gmod = _import_reference("scene.gaussian_model")
    shu = _import_reference("utils.sh_utils")
    spec = camera_specs()[cam_index]
    cam = reference_camera(spec)
    M = (max_deg + 1) ** 2
    g = np.random.default_rng(seed)
    raw = axis_cloud(g, cam, P, M) if kind == "axis" else cloud(g, cam, P, M, kind)
    pc = gmod.GaussianModel(max_deg)
    for k, v in raw.items():
        setattr(pc, k, v)
    pc.active_sh_degree = active
    bg = torch.tensor([0.1, 0.2, 0.3])

    calls = {}
    with _on_cpu(), mock.patch.object(gr, "GaussianRasterizer", _RecordingRasterizer), torch.no_grad():
        for mode, py in (("python", True), ("plain", False)):
            pipe = type("Pipe", (), {"convert_SHs_python": py, "compute_cov3D_python": py, "debug": False})
            _RecordingRasterizer.calls = []
            gr.render(cam, pc, pipe, bg, mod)
            calls[mode] = _RecordingRasterizer.calls[0]
        get = {"get_scaling": pc.get_scaling, "get_rotation": pc.get_rotation, "get_opacity": pc.get_opacity}
        feats = pc.get_features

    py, plain = calls["python"], calls["plain"]
    assert py["shs"] is None and py["scales"] is None and py["rotations"] is None
    assert plain["colors_precomp"] is None and plain["cov3D_precomp"] is None
    assert torch.equal(feats, torch.cat((raw["_features_dc"], raw["_features_rest"]), 1))
    for mine, theirs in ((plain["shs"], feats), (plain["scales"], get["get_scaling"]), (plain["rotations"], get["get_rotation"]),
                         (plain["opacities"], get["get_opacity"]), (plain["means3D"], raw["_xyz"]), (py["opacities"], get["get_opacity"]),
                         (py["means3D"], raw["_xyz"])):
        assert torch.equal(mine, theirs)
    for k, v in py["settings"].items():
        w = plain["settings"][k]
        assert (torch.equal(v, w) if isinstance(v, torch.Tensor) else v == w), k
    s = py["settings"]

    # fp64 truths, by the reference's own functions, of the fp32 values the rasterizer receives
    xyz64 = raw["_xyz"].double()
    cam64 = s["campos"].double()
    d = xyz64 - cam64[None]
    d = d / d.norm(dim=1, keepdim=True)
    sh64 = feats.double().transpose(1, 2).reshape(-1, 3, M)
    pre = shu.eval_sh(active, sh64, d) + 0.5
    scale = torch.full((P, 3), 0.5, dtype=torch.float64)
    for k in range(M):
        one = torch.zeros(P, 3, M, dtype=torch.float64)
        one[:, :, k] = 1.0
        scale += shu.eval_sh(active, one, d).abs() * sh64[:, :, k].abs()
    with _on_cpu(f64=True):
        cov64 = pc.covariance_activation(get["get_scaling"].double(), float(np.float32(mod)), raw["_rotation"].double())
    assert cov64.dtype == torch.float64

    out = {"raw" + k: v.numpy() for k, v in raw.items()}
    out.update({k: v.numpy() for k, v in get.items()})
    out.update({"max_sh_degree": np.int32(max_deg), "sh_degree": np.int32(s["sh_degree"]), "scale_modifier": np.float64(s["scale_modifier"]),
                "tanfovx": np.float64(s["tanfovx"]), "tanfovy": np.float64(s["tanfovy"]), "FoVx": np.float64(cam.FoVx),
                "FoVy": np.float64(cam.FoVy), "image_width": np.int32(s["image_width"]), "image_height": np.int32(s["image_height"]),
                "bg": s["bg"].numpy(), "viewmatrix": s["viewmatrix"].numpy(), "projmatrix": s["projmatrix"].numpy(),
                "campos": s["campos"].numpy(), "cov3D_precomp": py["cov3D_precomp"].numpy(),
                "colors_precomp": py["colors_precomp"].numpy(), "truth_sh_pre": pre.numpy(), "truth_sh_scale": scale.numpy(),
                "truth_cov3D": cov64.numpy(), "camera_index": np.int32(cam_index)})
    assert int(out["sh_degree"]) == active
    return out


def build():
    """{file name: {array name: array}} for every fixture, computed here and now."""
    torch.set_num_threads(1)     # one summation order for every run of the generator
    files = {}
    for case in cases():
        files[case[0]] = run_case(*case)
    cams = [camera_arrays(sp) for sp in camera_specs()]
    files["cameras"] = {k: np.stack([c[k] for c in cams]) for k in cams[0]}
    files["cameras"]["names"] = np.array([sp[0] for sp in camera_specs()])
    return files


def main():
    os.makedirs(OUT, exist_ok=True)
    total = 0
    for name, arrays in build().items():
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        total += size
        assert size <= 256 * 1024, (name, size)
        print(f"{name}: {size / 1024:.0f} KiB")
    assert total <= 1024 * 1024, total
    print(f"total {total / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
