"""The level-surface ray march of SuGaR's coarse mesh extraction, fused: ``SuGaR.compute_level_surface_points_from_camera_fast``
(``sugar/sugar_scene/sugar_model.py:1719-1954``, called once per training camera by ``sugar_extractors/coarse_mesh.py:246-340``).

For every kept pixel the reference samples the density field at ``n_points_in_range`` points along the pixel's ray, finds the first
crossing of each surface level, interpolates it and takes the field's gradient there as the normal -- with ``[n S, K, 3, 3]`` gathers in
passes of 2 M samples and one more gather per level.  :func:`level_surface` is one HIP kernel (``gsr_field.hip``, C ABI
``gsr_level_surface``): one lane per ray, the S running densities in registers, each packed 64-byte record read once per ray.  The
contract, per ray ``i``, plain fp32, left to right, nothing contracted:

* ``tau_s = range[s] stds[i]``, ``range = torch.linspace(-range_size, range_size, S)``; ``x_s = origins[i] + tau_s dirs[i]``;
* ``d_s`` = the density of :mod:`autovfx_amd.field` at ``x_s`` over the ray's K slots, k ascending, slots outside ``[0, P)`` skipped; then
  ``d_s = d_s / (d_s + 1e-12)`` where ``d_s >= 1`` (``:1879-1880``);
* per level ``l`` (``:1890-1908``): ``a`` = the smallest ``s`` with ``d_s > l``; the ray is empty unless ``d_0 < l`` and such an ``a``
  exists (it is then ``>= 1``); a NaN compares false both ways.  Otherwise ``t = (l - d_{a-1}) / (d_a - d_{a-1}) * (tau_a - tau_{a-1}) +
  tau_{a-1}`` and ``point = origins[i] + t dirs[i]``;
* normal at a hit (``:1923-1950``): ``g = sum_k o_k (M_j w)`` with ``w = M_j^T (point - c_j)`` and ``o_k`` the slot's opacity at
  ``point``, k ascending; ``normal = -(g / max(|g|, 1e-12))``;
* an empty ray has ``hit = 0`` and zeros for ``t``, its point and its normal.

There is no autograd (the extractor runs under ``no_grad``).  :func:`level_surface_host` restates the contract in numpy,
:func:`crossing_host` the selection and interpolation alone; :func:`drop_in_compute_level_surface_points_from_camera_fast` is what
``autovfx_amd.install()`` puts on ``SuGaR``.
"""
from __future__ import annotations

import ctypes
from typing import Callable, Optional

import numpy as np
import torch

from . import _takes
from .field import MAX_COUNT, MAX_K, _host_inputs, _host_pairs, _sum_ascending, field_values_host

MAX_S = 32
MAX_L = 8


def _levels_why_not(levels, n_points_in_range) -> Optional[str]:
    if isinstance(levels, torch.Tensor) or not isinstance(levels, (list, tuple)) or not all(
            isinstance(v, (int, float)) and not isinstance(v, bool) for v in levels):
        return f"levels must be a list of host numbers (got {type(levels).__name__})"
    if not 1 <= len(levels) <= MAX_L:
        return f"1..{MAX_L} levels per call (got {len(levels)})"
    if not isinstance(n_points_in_range, int) or isinstance(n_points_in_range, bool) or not 2 <= n_points_in_range <= MAX_S:
        return f"n_points_in_range must be an int in 2..{MAX_S} (got {n_points_in_range!r})"
    return None


def _why_not(origins, dirs, stds, idx, centers, inv_scaled_rotation, strengths, levels, n_points_in_range=21) -> Optional[str]:
    """None when the kernel takes the call, else the reason it does not."""
    named = tuple((name, t, torch.int64 if name == "idx" else torch.float32) for name, t in (
        ("origins", origins), ("dirs", dirs), ("stds", stds), ("idx", idx), ("centers", centers),
        ("inv_scaled_rotation", inv_scaled_rotation), ("strengths", strengths)))
    why = _takes.tensors(named, host="level_surface_host") or _takes.shaped("origins", origins, "[n, 3]", origins.dim() == 2 and origins.shape[1] == 3)
    if why is not None:
        return why
    n = origins.shape[0]
    why = (_takes.shaped("dirs", dirs, f"[n, 3] with n = {n}", tuple(dirs.shape) == (n, 3))
           or _takes.shaped("stds", stds, f"[n] with n = {n}", tuple(stds.shape) == (n,))
           or _takes.gaussians(n, idx, centers, inv_scaled_rotation, strengths, MAX_K))
    if why is not None:
        return why
    if n > MAX_COUNT or centers.shape[0] > MAX_COUNT:
        return f"{n} rays and {centers.shape[0]} Gaussians: at most 2^30 - 1 each"
    why = _levels_why_not(levels, n_points_in_range)
    if why is not None:
        return why
    if torch.is_grad_enabled():
        for name, t, _ in named:
            if t.requires_grad:
                return f"{name} requires a gradient and autograd is on: the ray march has no backward (the extractor runs under no_grad)"
    return _takes.capturing("the call allocates its scratch")


def _host_number(name, v) -> Optional[str]:
    if isinstance(v, torch.Tensor) or isinstance(v, bool) or not isinstance(v, (int, float)):
        return f"{name} must be a host number (got {type(v).__name__})"
    return None


def level_surface_takes(origins, dirs, stds, idx, centers, inv_scaled_rotation, strengths, levels, n_points_in_range=21, range_size=3.0,
                        density_factor=1.0, want_normals=True, want_densities=False) -> bool:
    """Whether :func:`level_surface` runs this call: CUDA float32 tensors on one device, ``origins`` / ``dirs [n, 3]``, ``stds [n]``,
    int64 ``idx [n, K]`` with ``1 <= K <= 64`` (any values: slots outside ``[0, P)`` are skipped), ``centers [P, 3]``,
    ``inv_scaled_rotation [P, 3, 3]``, ``strengths [P]`` or ``[P, 1]``, 1 to 8 host numbers as ``levels``, ``2 <= n_points_in_range <= 32``,
    host numbers as ``range_size`` and ``density_factor``, nothing that requires a gradient while autograd is on, not under graph
    capture.  Non-contiguous tensors are taken."""
    if _host_number("range_size", range_size) or _host_number("density_factor", density_factor):
        return False
    return _why_not(origins, dirs, stds, idx, centers, inv_scaled_rotation, strengths, levels, n_points_in_range) is None


def level_surface(origins, dirs, stds, idx, centers, inv_scaled_rotation, strengths, levels, n_points_in_range: int = 21,
                  range_size: float = 3.0, density_factor: float = 1.0, want_normals: bool = True, want_densities: bool = False) -> dict:
    """The contract above on the current stream, no host synchronisation after the 4 S bytes of ``range`` went to the device:
    ``{"hit": bool [L, n], "t": [L, n], "points": [L, n, 3], "normals": [L, n, 3] or None, "densities": [n, S] or None}``, dense per
    level, rows of empty rays zero.  A call :func:`level_surface_takes` rejects raises ``ValueError`` with the reason."""
    _takes.refuse("level_surface", _host_number("range_size", range_size) or _host_number("density_factor", density_factor)
                  or _why_not(origins, dirs, stds, idx, centers, inv_scaled_rotation, strengths, levels, n_points_in_range))
    from . import _lib

    o, v, sd, ix, cs, Ms, ss = _takes.cs(origins, dirs, stds, idx, centers, inv_scaled_rotation, strengths)
    n, K, P, S, L = int(o.shape[0]), int(ix.shape[1]), int(cs.shape[0]), int(n_points_in_range), len(levels)
    dev = o.device
    hit = torch.empty((L, n), dtype=torch.uint8, device=dev)
    t = torch.empty((L, n), dtype=torch.float32, device=dev)
    points = torch.empty((L, n, 3), dtype=torch.float32, device=dev)
    normals = torch.empty((L, n, 3), dtype=torch.float32, device=dev) if want_normals else None
    densities = torch.empty((n, S), dtype=torch.float32, device=dev) if want_densities else None
    if n > 0:
        rng = torch.linspace(-range_size, range_size, S).to(dev)          # (:1847: made on the host, then moved, so the reference's values)
        host_levels = (ctypes.c_float * MAX_L)(*[float(x) for x in levels])
        with torch.cuda.device(dev):
            scratch, nbytes = _lib.scratch("gsr_field_scratch_bytes", P, device=dev)
            _lib.call("gsr_level_surface", n, K, P, S, L, o.data_ptr(), v.data_ptr(), sd.data_ptr(), ix.data_ptr(), _lib.ptr(cs), _lib.ptr(Ms),
                      _lib.ptr(ss), float(density_factor), rng.data_ptr(), ctypes.byref(host_levels), hit.data_ptr(), t.data_ptr(), points.data_ptr(),
                      _lib.ptr(normals), _lib.ptr(densities), scratch.data_ptr(), nbytes, device=dev)
    return {"hit": hit.view(torch.bool), "t": t, "points": points, "normals": normals, "densities": densities}


# ---- the contract in numpy ----
def crossing_host(densities, taus, level):
    """``(hit bool [n], a int64 [n], t fp32 [n])`` of one level: the selection of ``:1890-1894`` and the interpolation of ``:1907`` on
    ``densities [n, S]`` and ``taus [n, S]``, fp32 in the reference's order.  ``a`` is the index of the first sample above the level
    (0 where there is none); ``t`` is 0 where the ray is empty."""
    d = np.asarray(densities, np.float32)
    tau = np.asarray(taus, np.float32)
    lev = np.float32(level)
    above = d > lev                       # (a NaN is neither above nor under)
    a = above.argmax(axis=1)
    hit = (d[:, 0] < lev) & (a > 0)
    rows, at = np.arange(d.shape[0]), np.where(hit, a, 1)
    d_a, d_b, tau_a, tau_b = d[rows, at], d[rows, at - 1], tau[rows, at], tau[rows, at - 1]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        t = (lev - d_b) / (d_a - d_b) * (tau_a - tau_b) + tau_b
    return hit, a.astype(np.int64), np.where(hit, t, np.float32(0)).astype(np.float32)


def level_surface_host(origins, dirs, stds, idx, centers, inv_scaled_rotation, strengths, levels, n_points_in_range: int = 21,
                       range_size: float = 3.0, density_factor: float = 1.0) -> dict:
    """The contract in numpy (fp32 elementwise, left to right): the keys of :func:`level_surface` plus ``"a" [L, n]`` (the crossing
    index) and ``"taus" [n, S]``."""
    f = np.float32
    o, v = np.asarray(origins, f).reshape(-1, 3), np.asarray(dirs, f).reshape(-1, 3)
    sd = np.asarray(stds, f).reshape(-1)
    n, S = o.shape[0], int(n_points_in_range)
    idx = np.asarray(idx, np.int64).reshape(n, -1)
    rng = torch.linspace(-range_size, range_size, S).numpy()
    with np.errstate(over="ignore", invalid="ignore", under="ignore", divide="ignore"):
        taus = rng[None, :] * sd[:, None]
        x = o[:, None, :] + taus[..., None] * v[:, None, :]
        d = field_values_host(x.reshape(-1, 3), np.repeat(idx, S, axis=0), centers, inv_scaled_rotation, strengths, None, density_factor)[0].reshape(n, S)
        d = np.where(d >= 1, d / (d + f(1e-12)), d).astype(f)
        _, _, c, M, sg, _, valid, j = _host_inputs(o, idx, centers, inv_scaled_rotation, strengths, None)
        out = {"hit": [], "a": [], "t": [], "points": [], "normals": [], "densities": d, "taus": taus}
        for level in levels:
            hit, a, t = crossing_host(d, taus, level)
            point = np.where(hit[:, None], o + t[:, None] * v, f(0)).astype(f)
            if c.shape[0] == 0:
                g = np.zeros((n, 3), f)
            else:
                _, w, _, e, Mj = _host_pairs(point, c, M, j)
                opac = np.where(valid, (f(density_factor) * sg[j]) * e, f(0)).astype(f)
                Mw = (Mj[..., :, 0] * w[..., 0:1] + Mj[..., :, 1] * w[..., 1:2]) + Mj[..., :, 2] * w[..., 2:3]
                g = np.stack([_sum_ascending(np.where(valid, opac * Mw[..., b], f(0))) for b in range(3)], axis=1)
            norm = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
            normal = -(g / np.maximum(norm, f(1e-12))[:, None])
            for key, val in (("hit", hit), ("a", a), ("t", t), ("points", point), ("normals", np.where(hit[:, None], normal, f(0)).astype(f))):
                out[key].append(val)
    for key in ("hit", "a", "t", "points", "normals"):
        out[key] = np.stack(out[key])
    return out


# ---- what install() puts on SuGaR ----
def _quaternion_invert(q):
    return q * q.new_tensor([1, -1, -1, -1])


def _quaternion_multiply(a, b):
    aw, ax, ay, az = torch.unbind(a, -1)
    bw, bx, by, bz = torch.unbind(b, -1)
    return torch.stack((aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw), -1)


def _quaternion_apply(q, point):
    """Rotate ``point [..., 3]`` by the quaternion ``q [..., 4]`` (real part first): the vector part of ``q (0, point) q^-1``."""
    p = torch.cat((point.new_zeros(point.shape[:-1] + (1,)), point), -1)
    return _quaternion_multiply(_quaternion_multiply(q, p), _quaternion_invert(q))[..., 1:]


def drop_in_compute_level_surface_points_from_camera_fast(original: Callable) -> Callable:
    """``SuGaR.compute_level_surface_points_from_camera_fast``: ``:1742-1851`` as the reference performs them, through ``self`` and the
    objects the caller handed in (the texture image, the splatted mesh, the caller's rasterizer -- pytorch3d's ``MeshRasterizer``, whose
    ``_C.rasterize_meshes`` is ``autovfx_amd.meshraster``'s under ``install()`` --, the depth fill, ``unproject_points``,
    ``knn_idx``, the per-Gaussian standard deviation; the two pixel tables as ``torch.arange`` expressions of the same fp32 values),
    then one :func:`level_surface` call in place of ``:1853-1950`` and the reference's compaction by boolean indexing: the same nested
    dict, dtypes, order and keys.  Whether the call is the kernel's is decided before anything is consumed -- ``torch.randperm`` in
    particular -- so a call that is not (the flat-Gaussian variants, ``just_use_depth_as_level``, ``use_gaussian_depth``, a CPU model, more than 32 samples, 8
    levels or 64 neighbours, graph capture, autograd on over parameters that require a gradient) runs ``original`` from an untouched
    state; should the tensors the model's own objects return turn out not to be the kernel's after the draw, the generator's state is
    put back before ``original`` runs.  ``quaternion_apply``, ``quaternion_invert``, ``RasterizationSettings`` and ``MeshRasterizer`` are the names the reference's
    own module imported, where it has them."""
    names = original.__globals__

    def why_original(self, surface_levels, n_points_in_range, range_size, density_factor, compute_flat_normals,
                     compute_intersection_for_flat_gaussian, just_use_depth_as_level, use_gaussian_depth) -> Optional[str]:
        if compute_intersection_for_flat_gaussian or compute_flat_normals or just_use_depth_as_level or use_gaussian_depth:
            return "a variant the drop-in does not perform"
        why = (_levels_why_not(surface_levels, n_points_in_range) or _host_number("range_size", range_size)
               or _host_number("density_factor", density_factor))
        if why is not None:
            return why
        params = [getattr(self, name, None) for name in ("points", "strengths", "scaling", "quaternions")]
        if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 for t in params):
            return "not a float32 model on a GPU"
        if torch.is_grad_enabled() and any(t.requires_grad for t in params):
            return "autograd is on"
        knn_idx = getattr(self, "knn_idx", None)
        K = getattr(self, "knn_to_track", None) or (knn_idx.shape[-1] if isinstance(knn_idx, torch.Tensor) else 0)
        if not 1 <= K <= MAX_K:
            return f"{K} neighbours"
        return _takes.capturing("the call allocates its scratch")

    def compute_level_surface_points_from_camera_fast(
            self, nerf_cameras=None, cam_idx=0, rasterizer=None, surface_levels=[0.1, 0.3, 0.5], n_surface_points=-1, primitive_types=None,
            triangle_scale=None, splat_mesh=True, n_points_in_range=21, range_size=3., n_points_per_pass=2_000_000, density_factor=1.,
            return_pixel_idx=False, return_gaussian_idx=False, return_normals=False, compute_flat_normals=False,
            compute_intersection_for_flat_gaussian=False, use_gaussian_depth=False, just_use_depth_as_level=False):
        def reference():
            return original(self, nerf_cameras=nerf_cameras, cam_idx=cam_idx, rasterizer=rasterizer, surface_levels=surface_levels,
                            n_surface_points=n_surface_points, primitive_types=primitive_types, triangle_scale=triangle_scale,
                            splat_mesh=splat_mesh, n_points_in_range=n_points_in_range, range_size=range_size,
                            n_points_per_pass=n_points_per_pass, density_factor=density_factor, return_pixel_idx=return_pixel_idx,
                            return_gaussian_idx=return_gaussian_idx, return_normals=return_normals, compute_flat_normals=compute_flat_normals,
                            compute_intersection_for_flat_gaussian=compute_intersection_for_flat_gaussian,
                            use_gaussian_depth=use_gaussian_depth, just_use_depth_as_level=just_use_depth_as_level)

        if why_original(self, surface_levels, n_points_in_range, range_size, density_factor, compute_flat_normals,
                        compute_intersection_for_flat_gaussian, just_use_depth_as_level, use_gaussian_depth) is not None:
            return reference()
        # ---- :1742-1851, the reference's statements ----
        if nerf_cameras is None:
            nerf_cameras = self.nerfmodel.training_cameras
        if primitive_types is not None:
            self.primitive_types = primitive_types
        if triangle_scale is not None:
            self.triangle_scale = triangle_scale
        if rasterizer is None:
            settings = names["RasterizationSettings"](image_size=(self.image_height, self.image_width), blur_radius=0.0, faces_per_pixel=10,
                                                      max_faces_per_bin=50_000)
            rasterizer = names["MeshRasterizer"](cameras=nerf_cameras.p3d_cameras[cam_idx], raster_settings=settings)
        p3d_cameras = nerf_cameras.p3d_cameras[cam_idx]
        textures_img = self.get_texture_img(nerf_cameras=nerf_cameras, cam_idx=cam_idx, sh_levels=self.sh_levels)
        mesh = self.splat_mesh(p3d_cameras) if splat_mesh else self.mesh
        mesh.textures._maps_padded = textures_img[None]
        fragments = rasterizer(mesh, cameras=p3d_cameras)
        depth = fragments.zbuf[0, ..., 0]
        no_depth_mask = depth < 0.
        depth[no_depth_mask] = depth.max() * 1.05

        # the two pixel tables (:1805-1812): x_tab[i][j] = i and y_tab[i][j] = j as fp32, through the reference's own operations
        H, W, dev = self.image_height, self.image_width, self.device
        rows = torch.arange(H, dtype=torch.float32, device=dev)
        cols = torch.arange(W, dtype=torch.float32, device=dev)
        ndc_x = W / min(W, H) - (cols / (min(W, H) - 1)) * 2
        ndc_y = H / min(W, H) - (rows / (min(W, H) - 1)) * 2
        ndc_points = torch.stack((ndc_x[None, :].expand(H, W), ndc_y[:, None].expand(H, W), depth), dim=-1).view(1, H * W, 3)

        fov_cameras = nerf_cameras.p3d_cameras[cam_idx]
        no_proj_mask = no_depth_mask.view(-1)
        ndc_points = ndc_points[0][~no_proj_mask][None]
        generator_state = torch.get_rng_state()          # (given back if the kernel turns out not to take what was built below)
        if n_surface_points == -1:
            n_surface_points = ndc_points.shape[1]
            ndc_points_idx = torch.arange(n_surface_points)
        else:
            n_surface_points = min(n_surface_points, ndc_points.shape[1])
            ndc_points_idx = torch.randperm(ndc_points.shape[1])[:n_surface_points]
            ndc_points = ndc_points[:, ndc_points_idx]
        all_world_points = fov_cameras.unproject_points(ndc_points, scaled_depth_input=False).view(-1, 3)

        gaussian_idx = fragments.pix_to_face[..., 0].view(-1) // self.n_triangles_per_gaussian
        gaussian_idx = gaussian_idx[~no_proj_mask][ndc_points_idx]
        closest_gaussians_idx = self.knn_idx[gaussian_idx]

        quaternion_apply = names.get("quaternion_apply", _quaternion_apply)
        quaternion_invert = names.get("quaternion_invert", _quaternion_invert)
        gaussian_to_camera = torch.nn.functional.normalize(fov_cameras.get_camera_center() - self.points, dim=-1)
        gaussian_standard_deviations = (self.scaling * quaternion_apply(quaternion_invert(self.quaternions), gaussian_to_camera)).norm(dim=-1)
        points_stds = gaussian_standard_deviations[closest_gaussians_idx[..., 0]]
        camera_to_samples = torch.nn.functional.normalize(all_world_points - fov_cameras.get_camera_center(), dim=-1)

        # ---- :1853-1950 in one launch ----
        inv_scaled_rotation = self.get_covariance(return_full_matrix=True, return_sqrt=True, inverse_scales=True)
        if not level_surface_takes(all_world_points, camera_to_samples, points_stds, closest_gaussians_idx, self.points, inv_scaled_rotation,
                                   self.strengths, list(surface_levels), n_points_in_range, range_size, density_factor):
            # what the model's own objects returned is not the kernel's (another dtype out of unproject_points, ...): the reference
            # runs from the generator state it would have found
            torch.set_rng_state(generator_state)
            return reference()
        with torch.no_grad():
            found = level_surface(all_world_points, camera_to_samples, points_stds, closest_gaussians_idx, self.points, inv_scaled_rotation,
                                  self.strengths, list(surface_levels), n_points_in_range, range_size, density_factor,
                                  want_normals=return_normals)
        all_outputs = {}
        for l, surface_level in enumerate(surface_levels):
            keep = found["hit"][l]
            outputs = {"intersection_points": found["points"][l][keep]}
            if return_pixel_idx:
                pixel_idx = torch.arange(H * W, dtype=torch.long, device=dev)
                outputs["pixel_idx"] = pixel_idx[~no_proj_mask][ndc_points_idx][keep]
            if return_gaussian_idx:
                outputs["gaussian_idx"] = gaussian_idx[keep]
            if return_normals:
                outputs["normals"] = found["normals"][l][keep]
            all_outputs[surface_level] = outputs
        return all_outputs

    return _takes.dressed(compute_level_surface_points_from_camera_fast, "compute_level_surface_points_from_camera_fast", original,
                          "SuGaR.compute_level_surface_points_from_camera_fast", "levelset")
