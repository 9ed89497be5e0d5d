"""Shared by test_levelset.py, test_levelset_gpu.py and golden/make_levelset_fixtures.py: the stub scene the reference's own
``SuGaR.compute_level_surface_points_from_camera_fast`` ran on (a model, a camera and a rasterizer that carry what the method reads),
the fixtures of tests/golden/levelset, the float64 truth of autovfx_amd.levelset's contract, and the bars results are held to.

Truth: a dense torch restatement in float64 of the contract (gather, batched product, clamp, exp, sum over the slots, the ``>= 1``
renormalisation, first crossing, interpolation, the field's gradient at the crossing), on the fp32 inputs of the march.

Bars, all from the reference's own fp32 CPU results on the fixtures, none from the code under test:

* densities: 4 x the largest absolute error of the reference's fp32 densities against the truth -- on a fixture its own figure, on any
  other case the fixtures' largest figure relative to the largest density, times the case's largest density;
* t, per ray: ``c_t [(tau_a - tau_{a-1}) 2 bar_d / (d_a - d_{a-1}) + 2^-24 |t|]``: both ends of the crossed interval may move by the
  density bar, and the result is rounded;
* points, per component: ``c_p [bar_t |dirs| + 2^-24 (|origin_b| + |t dir_b|)]``;
* normals, per component: ``c_n (K + 3) 2^-24 sum_k |o_k (M_k w_k)| / |g|`` (the norm of each slot's term).

Each ``c`` is 4 x the largest ratio the reference's own fp32 result reaches on the fixtures: the 4 covers a 2-ulp device ``expf``
against glibc's and another summation order in the 3-term products (the allowance of DESIGN.md 7g).

Rays near a level: ``hit`` and the crossing index must equal the truth's, except on a ray where some ``d_s`` with ``s`` up to the
truth's crossing index (every ``s`` where the truth finds none) lies within the density bar of the level; such a ray is left out of that
level's comparison, and at most 1 % of a case's rays may be (:data:`NEAR_CAP`)."""
from __future__ import annotations

import glob
import os
import types

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "levelset")
FIXTURES = sorted(os.path.basename(p)[len("ref_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "ref_*.npz")))
EPS = 2.0 ** -24
NEAR_CAP = 0.01
F = np.float32
_cache: dict = {}


# ---- what pytorch3d would provide (it is not installed): quaternions with the real part first ----
def quaternion_invert(quaternion):
    return quaternion * quaternion.new_tensor([1, -1, -1, -1])


def quaternion_raw_multiply(a, b):
    aw, ax, ay, az = torch.unbind(a, -1)
    bw, bx, by, bz = torch.unbind(b, -1)
    return torch.stack((aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw), -1)


def quaternion_apply(quaternion, point):
    real = point.new_zeros(point.shape[:-1] + (1,))
    out = quaternion_raw_multiply(quaternion_raw_multiply(quaternion, torch.cat((real, point), -1)), quaternion_invert(quaternion))
    return out[..., 1:]


def quaternion_to_matrix(q):
    w, a, b, c = (q[:, i] for i in range(4))
    return np.stack([1 - 2 * (b * b + c * c), 2 * (a * b - w * c), 2 * (a * c + w * b), 2 * (a * b + w * c), 1 - 2 * (a * a + c * c),
                     2 * (b * c - w * a), 2 * (a * c - w * b), 2 * (b * c + w * a), 1 - 2 * (a * a + b * b)], 1).reshape(-1, 3, 3)


# ---- the stub scene ----
class StubCamera:
    """A pinhole camera with pytorch3d's two methods the march uses: view = (world - centre) R, ndc = focal view.xy / view.z."""

    def __init__(self, center, R, focal, device="cpu"):
        self.center = torch.tensor(np.asarray(center, F), device=device).reshape(1, 3)
        self.R = torch.tensor(np.asarray(R, F), device=device)
        self.focal = float(focal)

    def get_camera_center(self):
        return self.center

    def unproject_points(self, xy_depth, scaled_depth_input=False):
        assert scaled_depth_input is False
        z = xy_depth[..., 2:3]
        view = torch.cat((xy_depth[..., 0:2] * z / self.focal, z), -1)
        return view @ self.R.transpose(0, 1) + self.center


class StubRasterizer:
    """Returns the prepared fragments, fresh each call (the march fills the depth in place)."""

    def __init__(self, zbuf, pix_to_face, device="cpu"):
        self.zbuf, self.pix_to_face = torch.tensor(zbuf, device=device), torch.tensor(pix_to_face, device=device)
        self.calls = 0

    def __call__(self, mesh, cameras=None):
        self.calls += 1
        assert mesh.textures._maps_padded is not None
        return types.SimpleNamespace(zbuf=self.zbuf.clone()[None], pix_to_face=self.pix_to_face.clone()[None])


class StubModel:
    """What ``compute_level_surface_points_from_camera_fast`` reads of a SuGaR model."""

    def __init__(self, sc: dict, device="cpu"):
        put = lambda a: torch.tensor(a, device=device)
        self.device = torch.device(device)
        self.image_height, self.image_width = int(sc["H"]), int(sc["W"])
        self.points, self.scaling, self.quaternions, self.strengths = (put(sc[k]) for k in ("points", "scaling", "quaternions", "strengths"))
        self.knn_idx, self.knn_to_track = put(sc["knn_idx"]), int(sc["knn_idx"].shape[1])
        self.n_triangles_per_gaussian, self.sh_levels = int(sc["n_tri"]), 1
        self.primitive_types, self.triangle_scale = "diamond", 2.0
        self._M = put(inv_scaled_rotation(sc))
        self.mesh = types.SimpleNamespace(textures=types.SimpleNamespace(_maps_padded=None))
        self.cameras = types.SimpleNamespace(p3d_cameras=[StubCamera(sc["cam_center"], sc["cam_R"], sc["cam_focal"], device)])
        self.nerfmodel = types.SimpleNamespace(training_cameras=self.cameras)
        self.texture_calls = self.splat_calls = 0

    def get_texture_img(self, nerf_cameras=None, cam_idx=0, sh_levels=None):
        self.texture_calls += 1
        return torch.zeros(4, 4, 3, device=self.device)

    def splat_mesh(self, p3d_cameras):
        self.splat_calls += 1
        return types.SimpleNamespace(textures=types.SimpleNamespace(_maps_padded=None))

    def get_covariance(self, return_full_matrix=False, return_sqrt=False, inverse_scales=False):
        assert return_full_matrix and return_sqrt and inverse_scales
        return self._M


def inv_scaled_rotation(sc: dict) -> np.ndarray:
    """R diag(1 / s) in fp32: get_covariance(return_full_matrix=True, return_sqrt=True, inverse_scales=True)."""
    return (quaternion_to_matrix(sc["quaternions"].astype(np.float64)) / sc["scaling"].astype(np.float64)[:, None, :]).astype(F)


def scene(P: int, K: int, H: int, W: int, seed: int, hole_share: float = 0.1) -> dict:
    """A bumpy sheet of P Gaussians four units in front of a camera, and the fragments a mesh rasterizer would return for it: per pixel
    the Gaussian nearest to the pixel's ray and the depth of its centre; pixels whose ray misses the sheet, and a random share of the
    rest, have no depth."""
    g = np.random.default_rng(seed)
    u = g.uniform(-1, 1, (P, 2))
    view = np.stack([1.3 * u[:, 0], 1.1 * u[:, 1], 4 + 0.3 * np.sin(3 * u[:, 0]) * np.cos(2 * u[:, 1]) + g.normal(0, 0.03, P)], 1)
    R = np.linalg.qr(g.normal(size=(3, 3)))[0]
    if np.linalg.det(R) < 0:
        R[:, 0] = -R[:, 0]
    C = g.normal(0, 1, 3)
    points = view @ R.T + C
    spacing = np.sqrt(2.6 * 2.2 / P)
    scaling = np.exp(g.normal(np.log(0.6 * spacing), 0.35, (P, 3)))
    q = g.normal(size=(P, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    strengths = 1 / (1 + np.exp(-g.normal(1.0, 1.5, (P, 1))))
    near = np.argsort(((points[:, None, :] - points[None]) ** 2).sum(-1), axis=1, kind="stable")
    knn_idx = near[:, np.arange(K) % P]
    focal, m, n_tri, layers = 3.5, min(H, W), 2, 2
    ndc_x = W / m - np.arange(W) / (m - 1) * 2
    ndc_y = H / m - np.arange(H) / (m - 1) * 2
    rays = np.stack([np.broadcast_to(ndc_x[None, :], (H, W)) / focal, np.broadcast_to(ndc_y[:, None], (H, W)) / focal, np.ones((H, W))], -1)
    rays /= np.linalg.norm(rays, axis=-1, keepdims=True)
    along = (view[None, None] * rays[:, :, None, :]).sum(-1)                       # [H,W,P]
    off = np.linalg.norm(view[None, None] - along[..., None] * rays[:, :, None, :], axis=-1)
    who = off.argmin(-1)
    seen = (off.min(-1) < 1.5 * spacing) & (g.random((H, W)) >= hole_share)
    zbuf = np.full((H, W, layers), -1.0)
    pix = np.full((H, W, layers), -1, np.int64)
    zbuf[..., 0] = np.where(seen, view[who, 2], -1.0)
    pix[..., 0] = np.where(seen, who * n_tri + g.integers(0, n_tri, (H, W)), -1)
    return dict(H=np.int64(H), W=np.int64(W), n_tri=np.int64(n_tri), points=points.astype(F), scaling=scaling.astype(F), quaternions=q.astype(F),
                strengths=strengths.astype(F), knn_idx=knn_idx.astype(np.int64), zbuf=zbuf.astype(F), pix_to_face=pix, cam_center=C.astype(F),
                cam_R=R.astype(F), cam_focal=np.float64(focal))


def random_case(n: int, K: int, P: int, seed: int, bad_slots: bool = True) -> dict:
    """Rays for the op alone: the Gaussians of :func:`scene`, n rays that start near a Gaussian, point anywhere and carry that
    Gaussian's neighbour list (some slots -1 or P)."""
    sc = scene(P, K, 4, 4, seed)
    g = np.random.default_rng(seed + 500)
    first = g.integers(0, P, n)
    spread = float(sc["scaling"].mean())
    dirs = g.normal(size=(n, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    idx = sc["knn_idx"][first].copy()
    if bad_slots:
        idx[g.random((n, K)) < 0.1] = -1
        idx[g.random((n, K)) < 0.05] = P
    return dict(origins=(sc["points"][first] + g.normal(0, 0.5 * spread, (n, 3))).astype(F), dirs=dirs.astype(F),
                stds=np.exp(g.normal(np.log(spread), 0.3, n)).astype(F), idx=idx, centers=sc["points"], M=inv_scaled_rotation(sc),
                strengths=sc["strengths"], density_factor=1.0)


# ---- fixtures ----
def fixture(name: str) -> dict:
    if name not in _cache:
        with np.load(os.path.join(GOLDEN, f"ref_{name}.npz")) as z:
            d = {k: z[k] for k in z.files}
        d["levels"] = [float(v) for v in d["levels"]]
        for k in ("density_factor", "range_size"):
            d[k] = float(d[k])
        for k in ("n_surface_points", "n_points_in_range"):
            d[k] = int(d[k])
        _cache[name] = d
    return _cache[name]


def fixture_case(name: str) -> dict:
    """The march's own inputs on a fixture, as the reference computed them in fp32."""
    fx = fixture(name)
    return dict(origins=fx["ref.origins"], dirs=fx["ref.dirs"], stds=fx["ref.stds"], idx=fx["ref.idx"], centers=fx["points"],
                M=inv_scaled_rotation(fx), strengths=fx["strengths"], density_factor=fx["density_factor"])


# ---- the float64 truth ----
def truth(c: dict, levels, S: int = 21, range_size: float = 3.0) -> dict:
    f = torch.float64
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64))
    o, v, sd, cs, M, sg = (t64(c[k]) for k in ("origins", "dirs", "stds", "centers", "M", "strengths"))
    sg = sg.reshape(-1)
    idx = torch.tensor(np.asarray(c["idx"], np.int64))
    n, K = idx.shape
    P = cs.shape[0]
    valid = (idx >= 0) & (idx < P)
    j = idx.clamp(0, max(P - 1, 0))
    zero = torch.zeros((), dtype=f)

    def pairs(x):                     # x [n, m, 3] -> opacities [n, m, K], w [n, m, K, 3]
        s = x[:, :, None, :] - cs[j][:, None]
        w = (M[j].transpose(-1, -2)[:, None] @ s[..., None])[..., 0]
        e = torch.exp(-0.5 * (w * w).sum(-1).clamp(0.0, 1e8))
        return torch.where(valid[:, None], c["density_factor"] * sg[j][:, None] * e, zero), w

    taus = torch.linspace(-range_size, range_size, S).to(f)[None, :] * sd[:, None]
    d = pairs(o[:, None, :] + taus[..., None] * v[:, None, :])[0].sum(-1)
    d = torch.where(d >= 1, d / (d + 1e-12), d)
    out = {"densities": d.numpy(), "taus": taus.numpy(), "hit": [], "a": [], "t": [], "points": [], "normals": [], "slope": [], "terms": []}
    rows = torch.arange(n)
    for level in levels:
        lev = float(np.float32(level))
        above = d > lev
        a = above.to(torch.int8).argmax(1)
        hit = (d[:, 0] < lev) & (a > 0)
        at = torch.where(hit, a, torch.ones_like(a))
        d_a, d_b, tau_a, tau_b = d[rows, at], d[rows, at - 1], taus[rows, at], taus[rows, at - 1]
        t = torch.where(hit, (lev - d_b) / (d_a - d_b) * (tau_a - tau_b) + tau_b, zero)
        point = o + t[:, None] * v
        opac, w = pairs(point[:, None, :])
        term = opac[:, 0, :, None] * (M[j] @ w[:, 0, :, :, None])[..., 0]            # [n, K, 3]
        grad = term.sum(1)
        normal = -grad / grad.norm(dim=-1, keepdim=True).clamp(min=1e-12)
        keep = hit[:, None]
        for key, val in (("hit", hit), ("a", torch.where(hit, a, torch.zeros_like(a))), ("t", t), ("points", torch.where(keep, point, zero)),
                         ("normals", torch.where(keep, normal, zero)), ("slope", torch.where(hit, (tau_a - tau_b) / (d_a - d_b), zero)),
                         ("terms", torch.where(hit, term.norm(dim=-1).sum(1) / grad.norm(dim=-1).clamp(min=1e-300), zero))):
            out[key].append(val.numpy())
    for key in ("hit", "a", "t", "points", "normals", "slope", "terms"):
        out[key] = np.stack(out[key])
    out["K"], out["levels"] = K, [float(np.float32(x)) for x in levels]
    out["dir_norm"], out["origins"], out["dirs"] = v.norm(dim=-1).numpy(), o.numpy(), v.numpy()
    return out


def fixture_truth(name: str) -> dict:
    key = ("truth", name)
    if key not in _cache:
        fx = fixture(name)
        _cache[key] = truth(fixture_case(name), fx["levels"], fx["n_points_in_range"], fx["range_size"])
    return _cache[key]


# ---- the bars ----
def near_level(want: dict, bar_d: float) -> np.ndarray:
    """[L, n]: rays left out of a level's comparison."""
    d = want["densities"]
    S = d.shape[1]
    out = []
    for l, lev in enumerate(want["levels"]):
        last = np.where(want["hit"][l], want["a"][l], S - 1)
        upto = np.arange(S)[None, :] <= last[:, None]
        out.append(((np.abs(d - lev) <= bar_d) & upto).any(1))
    return np.stack(out)


def units(want: dict, bar_d: float, c_t: float = 1.0) -> dict:
    """Per ray and level, the bracketed expressions of the t, points and normals bars (``c_t`` enters the points')."""
    t_unit = want["slope"] * 2 * bar_d + EPS * np.abs(want["t"])
    p_unit = (c_t * t_unit * want["dir_norm"][None])[..., None] + EPS * (np.abs(want["origins"])[None] + np.abs(want["t"][..., None] * want["dirs"][None]))
    return {"t": t_unit, "points": p_unit, "normals": ((want["K"] + 3) * EPS * want["terms"])[..., None]}


def reference_density_error(name: str) -> float:
    return float(np.abs(fixture(name)["ref.densities"] - fixture_truth(name)["densities"]).max())


def density_bar(name: str) -> float:
    return 4.0 * reference_density_error(name)


def density_bar_relative() -> float:
    if "rel" not in _cache:
        _cache["rel"] = max(density_bar(n) / float(np.abs(fixture_truth(n)["densities"]).max()) for n in FIXTURES)
    return _cache["rel"]


def reference_dense(name: str) -> dict:
    """The reference's own fp32 results of a fixture as dense [L, n] arrays (rows of empty rays zero)."""
    fx = fixture(name)
    hit = fx["ref.hit"].astype(bool)
    out = {"hit": hit, "a": fx["ref.a"], "t": fx["ref.t"], "densities": fx["ref.densities"]}
    for key, tag in (("points", "intersection_points"), ("normals", "normals")):
        dense = np.zeros(hit.shape + (3,), F)
        for l in range(hit.shape[0]):
            dense[l][hit[l]] = fx[f"out{l}.{tag}"]
        out[key] = dense
    return out


def factors() -> dict:
    """``c_t``, ``c_p``, ``c_n``: 4 x the largest error / unit ratio of the reference's own fp32 results over the fixtures (rays near a
    level left out, as in every comparison)."""
    if "c" not in _cache:
        c = {"t": 0.0, "points": 0.0, "normals": 0.0}
        for key in ("t", "points", "normals"):            # t first: its factor is part of the points' unit
            for name in FIXTURES:
                want, ref, bar_d = fixture_truth(name), reference_dense(name), density_bar(name)
                live = want["hit"] & ref["hit"] & ~near_level(want, bar_d)
                unit = units(want, bar_d, c["t"] if key == "points" else 1.0)[key]
                err = np.abs(ref[key] - want[key])
                ratio = err[live] / np.broadcast_to(unit, err.shape)[live]
                c[key] = max(c[key], 4.0 * float(ratio.max()))
        _cache["c"] = c
    return _cache["c"]


def check(got: dict, want: dict, bar_d: float = None, label: str = "", normals: bool = True) -> None:
    """``got``: hit [L, n], t, points, normals, optionally a and densities; ``want``: a :func:`truth` result.  ``bar_d`` None: the
    fixtures' relative density bar at this case's scale."""
    if bar_d is None:
        bar_d = density_bar_relative() * float(np.abs(want["densities"]).max()) if want["densities"].size else 0.0
    c = factors()
    if got.get("densities") is not None and want["densities"].size:
        err = float(np.abs(np.asarray(got["densities"], np.float64) - want["densities"]).max())
        print(f"{label} densities: error {err:.3e}, bar {bar_d:.3e}")
        assert err <= bar_d, (label, "densities", err, bar_d)
    near = near_level(want, bar_d)
    n = max(want["hit"].shape[1], 1)
    print(f"{label} rays near a level: {near.sum(1).tolist()} of {want['hit'].shape[1]}; hits {want['hit'].sum(1).tolist()}")
    assert np.all(near.sum(1) <= NEAR_CAP * n), (label, "rays near a level", near.sum(1).tolist(), n)
    hit = np.asarray(got["hit"]).astype(bool)
    assert np.array_equal(hit[~near], want["hit"][~near]), (label, "hit", int((hit != want["hit"])[~near].sum()))
    if got.get("a") is not None:
        live = ~near & want["hit"]
        assert np.array_equal(np.asarray(got["a"])[live], want["a"][live]), (label, "crossing index")
    u = units(want, bar_d, c["t"])
    live = ~near
    for key in ("t", "points") + (("normals",) if normals else ()):
        err = np.abs(np.asarray(got[key], np.float64) - want[key])
        bound = np.broadcast_to(c[key] * u[key], err.shape)
        mask = np.broadcast_to(live if err.ndim == 2 else live[..., None], err.shape)
        ratio = float((err[mask] / np.maximum(bound[mask], 1e-300)).max()) if mask.any() and (err[mask] > 0).any() else 0.0
        print(f"{label} {key}: largest error / bound {ratio:.3f} (c = {c[key]:.2f})")
        assert np.all(err[mask] <= bound[mask]), (label, key, ratio)
        empty = mask & ~np.broadcast_to(want["hit"] if err.ndim == 2 else want["hit"][..., None], err.shape)
        assert np.all(np.asarray(got[key])[empty] == 0), (label, key, "an empty ray's row is not zero")
