"""The triangle votes of object extraction on the GPU: the loop of ``extract_object_from_scene`` (``extract/extract_object.py:115-159``)
that casts a ray through every masked pixel of every tracked view against the scene mesh and counts, per face, the views that see it.

The reference asks trimesh for the first hits on the host, with the rays and the answers making a round trip through
``.cpu().numpy()`` per view; here a view is one :func:`autovfx_amd.meshquery.first_hits` call and nothing leaves the device.  The
other three ray sites of that file (``:424-434``, ``:476-482``, ``:563-606``) are single calls of ``first_hits`` and have no wrapper.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import torch

from . import meshquery


def ray_directions(h: int, w: int, K: torch.Tensor) -> torch.Tensor:
    """``get_ray_directions(h, w, K, flatten=False)`` of the reference (``gaussian_renderer/__init__.py:41-80``, through pixel centres):
    ``[h, w, 3]`` float32 in camera coordinates, ``((u - cx + 0.5) / fx, (v - cy + 0.5) / fy, 1)`` with ``u`` the column and ``v``
    the row."""
    v, u = torch.meshgrid(torch.arange(h, dtype=torch.float32, device=K.device), torch.arange(w, dtype=torch.float32, device=K.device),
                          indexing="ij")
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    return torch.stack([(u - cx + 0.5) / fx, (v - cy + 0.5) / fy, torch.ones_like(u)], -1)


def triangle_votes(scene: "meshquery.Scene", masks: Sequence, c2ws: Sequence, K, h: int, w: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """``scene``: a :class:`autovfx_amd.meshquery.Scene` over the scene mesh; ``masks``: one ``[h, w]`` mask per view (nonzero: the
    object); ``c2ws``: one 4x4 camera-to-world matrix per view; ``K``: the 3x3 intrinsics.  Returns ``(counter, counter_naive)``, two
    int32 ``[F]`` device tensors, the reference's ``TRIANGLES_VIEW_COUNTER`` and ``TRIANGLES_VIEW_COUNTER_NAIVE``:

    * ``counter_naive[f]`` = the views in which the ray of some masked pixel hits face ``f`` first (``t[idx] += 1`` with a repeated
      index counts once per view);
    * ``counter[f]`` = those of them in which the face's centre, ``(a + b + c) / 3`` projected with ``inverse(c2w)`` and ``K`` and
      rounded, also falls on a masked pixel of the view.

    A ray that hits nothing votes for no face.  (The reference hands trimesh's -1 to ``t[idx] += 1``, which is the mesh's last
    face.)  One ``first_hits`` call per view, on the masked pixels in row order; no array goes through the host inside the loop
    (torch's boolean indexing reads back a count, as it does in the reference)."""
    if len(masks) != len(c2ws):
        raise ValueError(f"triangle_votes: {len(masks)} masks and {len(c2ws)} poses")
    dev = scene.verts.device
    F = int(scene.faces.shape[0])
    K = torch.as_tensor(K, dtype=torch.float32).to(dev)
    counter = torch.zeros(F, dtype=torch.int32, device=dev)
    counter_naive = torch.zeros(F, dtype=torch.int32, device=dev)
    if F == 0:
        return counter, counter_naive
    directions = ray_directions(h, w, K)
    centres = scene.verts[scene.faces.clamp(0, max(0, int(scene.verts.shape[0]) - 1))].mean(dim=1)   # (an invalid face is never hit)
    with torch.no_grad():
        for mask, c2w in zip(masks, c2ws):
            mask = torch.as_tensor(mask).to(dev) != 0
            if tuple(mask.shape) != (h, w):
                raise ValueError(f"triangle_votes: a mask of {list(mask.shape)}, not [{h}, {w}]")
            c2w = torch.as_tensor(c2w, dtype=torch.float32).to(dev)
            rays_d = directions @ c2w[:3, :3].T
            rays_o = c2w[:3, 3].expand_as(rays_d)
            index_tri = meshquery.first_hits(rays_o[mask].reshape(-1, 3), rays_d[mask].reshape(-1, 3), scene.verts, scene.faces,
                                             plan=scene.plan, sort=False)[0]      # (pixels in row order run side by side)
            index_tri = index_tri[index_tri >= 0]
            counter_naive[index_tri] += 1
            # check again if the triangle centre is in the mask
            w2c = torch.inverse(c2w)
            xyz = centres[index_tri]
            xyz = torch.cat([xyz, torch.ones(xyz.size(0), 1, device=dev)], dim=1)
            xyz = torch.matmul(xyz, w2c.T)
            xyz = xyz[:, :3]
            xyz = xyz / xyz[:, 2].unsqueeze(1)
            uv = torch.matmul(xyz, K.T)
            uv = uv[:, :2].round().long()
            valid_uv_mask = (uv[:, 0] >= 0) & (uv[:, 0] < w) & (uv[:, 1] >= 0) & (uv[:, 1] < h)
            filtered_uv = uv[valid_uv_mask]
            in_mask_indices = torch.where(mask[filtered_uv[:, 1], filtered_uv[:, 0]])[0]
            in_mask = valid_uv_mask.nonzero().flatten()[in_mask_indices]
            counter[index_tri[in_mask]] += 1
    return counter, counter_naive
