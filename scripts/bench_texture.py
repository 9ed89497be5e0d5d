#!/usr/bin/env python
"""The texture bake of SuGaR's refined mesh (autovfx_amd/texture.py) timed on the GPU beside the reference-shaped torch code on the same
device, one JSON line per mesh size.  The comparator restates ``extract_texture_image_and_uv_from_gaussians``
(sugar/sugar_scene/sugar_model.py:2398-2614) without pytorch3d, which has no kernels for the MI355X: the initial fill with its
``[F, n, G, 3, 3]`` temporaries (``:2519-2536``) and, per camera, ``TexturesUV.sample_textures`` on the index map (interpolation, the flip
that copies the map, ``grid_sample``), the Phong pass under ambient light, ``softmax_rgb_blend`` of one layer, the boolean-mask gathers
and the six index operations with their ``nonzero`` (``:2596-2609``).

The scene: scripts/bench_meshraster.py's flat diamonds, ``--faces`` triangles, rasterized once by ``autovfx_amd.meshraster`` at ``--height`` x
``--width``; view v of ``--views`` sees those fragments rolled by 37 v columns and an RGBA image of its own, so the views' buffers (83 MB
each at 1080 x 1920) follow each other through more than twice the 256 MiB Infinity Cache and no view finds its data on the chip; the
atlas is shared by the views, as in the real call.  Every time is the median of ``--repeats`` windows between two device events, each of as many passes
over all views as fill 5 ms, after one warm-up pass.

* ``fill_ms`` / ``torch_fill_ms``: ``texture.fill`` against the restated ``:2519-2539`` (``null`` from 2e7 (face, texel, Gaussian) triples:
  its 3x3 products are a batched matrix product with one batch per triple, which torch cannot run at that many batches on this GPU,
  DESIGN.md 7h); ``fill_peak_mb`` / ``torch_fill_peak_mb``: the allocator's peak above what was held before the call.
* ``bake_ms_per_view``: ``gsr_texture_bake_view`` alone (claim + accumulate).
* ``tail_ms_per_view``: what the drop-in does per camera after the two renders: ``clamp``, the ``[..., :3]`` view, ``texture.bake_view``.
* ``torch_tail_ms_per_view``: the comparator's loop body on the same fragments; ``torch_sample_ms_per_view`` is its sampler and blend alone.
* ``tail_peak_mb`` / ``torch_tail_peak_mb``: peak above the inputs, the atlas, the counter and (for the comparator) the index map.
* ``count_equal``: both sides counted the same views per texel; ``texels_equal``: the share of texels with the same colour (the comparator's
  ``index_put`` leaves open which of a texel's pixels wins).

Usage: ``python scripts/bench_texture.py [--faces 200000 1000000 2000000] [--views 10] [--square 10] [--gaussians 1] [--repeats 10]``.
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, ROOT)
from autovfx_amd import _lib, texture                          # noqa: E402
from autovfx_amd.meshraster import rasterize_face_verts         # noqa: E402
from bench_meshraster import scene                              # noqa: E402


# ---- the comparator ----
def torch_fill(verts, faces, centers, M, features, offs, bary, A, S):
    F, G, T = faces.shape[0], centers.shape[0] // faces.shape[0], A * S
    faces_verts = verts[faces]
    all_bary = bary[None].expand(F // 2 + 1, -1, -1, -1).reshape(-1, bary.shape[-2], 3)[:F]
    positions = (all_bary[..., None] * faces_verts[:, None]).sum(dim=-2)[:, :, None]
    shift = positions - centers.reshape(-1, 1, G, 3)
    warped = M.reshape(-1, 1, G, 3, 3).transpose(-1, -2) @ shift[..., None]
    weights = torch.exp(-1. / 2 * (warped[..., 0] * warped[..., 0]).sum(dim=-1).clamp(min=0., max=1e8))
    pixel_features = features.reshape(F, G, 3)[:, None].expand(-1, weights.shape[1], -1, -1).gather(
        dim=-2, index=weights[..., None].argmax(dim=-2, keepdim=True).expand(-1, -1, -1, 3))[:, :, 0, :]
    grid = torch.cartesian_prod(torch.arange(A, device=verts.device), torch.arange(A, device=verts.device))[:, None] * S
    idx = torch.cat([(grid + offs[0][None])[:, None], (grid + offs[1][None])[:, None]], dim=1).view(-1, offs.shape[1], 2)[:F]
    img = torch.zeros(T, T, 3, device=verts.device)
    img[(idx[..., 0].long(), idx[..., 1].long())] = pixel_features
    return img.transpose(0, 1).flip(0) * 0.28209479177387814 + 0.5


def torch_sample_and_blend(index_map, pix, bary, zbuf, dists, face_uvs):
    """``renderer.shader(fragments, idx_mesh)[0, ..., :2]``: pix [1,H,W,1], bary [1,H,W,1,3]; index_map [1,T,T,3]."""
    N, H, W, K = pix.shape
    mask = pix >= 0
    att = face_uvs[pix.clamp(min=0)]
    uvs = (bary[..., None] * att).sum(dim=-2)
    uvs = torch.where(mask[..., None], uvs, torch.zeros_like(uvs)).permute(0, 3, 1, 2, 4).reshape(N * K, H, W, 2)
    maps = torch.flip(index_map.permute(0, 3, 1, 2), [2])
    texels = torch.nn.functional.grid_sample(maps, uvs * 2.0 - 1.0, mode="nearest", align_corners=True, padding_mode="border")
    colors = (1.0 * 1.0 + 0.0) * texels.reshape(N, K, 3, H, W).permute(0, 3, 4, 1, 2) + 0.0
    eps, sigma, gamma, znear, zfar = 1e-10, 1e-4, 1e-4, 1.0, 100.0
    prob_map = torch.sigmoid(-dists / sigma) * mask
    alpha = torch.prod((1.0 - prob_map), dim=-1)
    z_inv = (zfar - zbuf) / (zfar - znear) * mask
    z_inv_max = torch.max(z_inv, dim=-1).values[..., None].clamp(min=eps)
    weights_num = prob_map * torch.exp((z_inv - z_inv_max) / gamma)
    delta = torch.exp((eps - z_inv_max) / gamma).clamp(min=eps)
    denom = weights_num.sum(dim=-1)[..., None] + delta
    pixel_colors = torch.ones((N, H, W, 4), device=pix.device)
    pixel_colors[..., :3] = ((weights_num[..., None] * colors).sum(dim=-2) + delta * 0.0) / denom
    pixel_colors[..., 3] = 1.0 - alpha
    return pixel_colors[0, ..., :2]


def torch_tail(texture_img, texture_counter, index_map, rgba, pix, bary, zbuf, dists, face_uvs):
    rgb_img = rgba.clamp(min=0, max=1)[..., :3]
    idx_img = torch_sample_and_blend(index_map, pix, bary, zbuf, dists, face_uvs)
    update_mask = zbuf[0, ..., 0] > 0
    idx_to_update = idx_img[update_mask].round().long()
    at = (idx_to_update[..., 0], idx_to_update[..., 1])
    no_initialize_mask = texture_counter[at][..., 0] != 0
    texture_img[at] = no_initialize_mask[..., None] * texture_img[at]
    texture_img[at] = texture_img[at] + rgb_img[update_mask][..., 0:3]
    texture_counter[at] = texture_counter[at] + 1


# ---- timing ----
def timed(passes, repeats, per=1, window_ms=5.0):
    """Median milliseconds of ``passes()`` over ``per``: after one warm-up call, ``repeats`` windows of as many calls as fill ``window_ms``."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    passes()
    e0.record()
    passes()
    e1.record()
    e1.synchronize()
    batch = min(200, max(1, math.ceil(window_ms / max(e0.elapsed_time(e1), 1e-3))))
    out = []
    for _ in range(repeats):
        e0.record()
        for _ in range(batch):
            passes()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / (batch * per))
    return round(statistics.median(out), 4)


def peak_mb(call):
    """What ``call()`` allocates at its peak, above what is held now."""
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    call()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - held) / 2 ** 20, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, nargs="+", default=[200_000, 1_000_000, 2_000_000])
    ap.add_argument("--views", type=int, default=10)
    ap.add_argument("--square", type=int, default=10)
    ap.add_argument("--gaussians", type=int, default=1)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--size", type=float, default=0.02)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--no-torch", action="store_true", help="skip the comparator")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    H, W, S, G, views = args.height, args.width, args.square, args.gaussians, args.views
    with torch.no_grad():
        for n_faces in args.faces:
            fv, first, num, nbr = scene(n_faces // 2, H, W, args.size, dev)
            F = int(fv.shape[0])
            verts, faces = fv.reshape(-1, 3).contiguous(), torch.arange(3 * F, device=dev).view(F, 3)
            g = torch.Generator(device=dev).manual_seed(F)
            centers = (fv.mean(dim=1, keepdim=True) + args.size * torch.randn((F, G, 3), generator=g, device=dev)).reshape(F * G, 3).contiguous()
            M = torch.randn((F * G, 3, 3), generator=g, device=dev) / args.size
            features = torch.rand((F * G, 3), generator=g, device=dev) * 3 - 1.5
            verts_uv, faces_uv, T, A, offs, barys = texture.atlas(F, S, dev)
            face_uvs = verts_uv[faces_uv].contiguous()
            row = {"faces": F, "H": H, "W": W, "views": views, "square_size": S, "texture_size": T, "gaussians_per_face": G,
                   "device": torch.cuda.get_device_name(0)}

            # the fill
            do_fill = lambda: texture.fill(verts, faces, centers, M, features, offs, barys, A, S)
            row["fill_ms"], row["fill_peak_mb"] = timed(do_fill, args.repeats), peak_mb(do_fill)
            row["torch_fill_ms"] = row["torch_fill_peak_mb"] = None
            if not args.no_torch and F * offs.shape[1] * G < 20_000_000:
                do_torch_fill = lambda: torch_fill(verts, faces, centers, M, features, offs, barys, A, S)
                row["torch_fill_ms"], row["torch_fill_peak_mb"] = timed(do_torch_fill, args.repeats), peak_mb(do_torch_fill)
            fill = do_fill()

            # the views
            pix4, zbuf4, bary5, dists4 = rasterize_face_verts(fv, first, num, nbr, (H, W), 0.0, 1, None, 50_000, True, False, False)
            frames = []
            for v in range(views):
                roll = lambda t: torch.roll(t, 37 * v, dims=2).contiguous()
                frames.append(dict(pix=roll(pix4), bary=roll(bary5), zbuf=roll(zbuf4), dists=roll(dists4),
                                   rgba=torch.rand((H, W, 4), generator=g, device=dev) * 1.2 - 0.1))
            row["covered_pixels"] = int((pix4 >= 0).sum())
            del pix4, zbuf4, bary5, dists4
            tex, count, owner = fill.clone(), torch.zeros((T, T, 1), device=dev), texture.new_owner(T, dev)
            P = H * W

            def kernels():
                for f in frames:
                    _lib.call("gsr_texture_bake_view", P, F, T, f["pix"].data_ptr(), f["bary"].data_ptr(), f["zbuf"].data_ptr(), face_uvs.data_ptr(),
                              f["rgba"].data_ptr(), 4, tex.data_ptr(), count.data_ptr(), owner.data_ptr(), device=dev)

            def tail():
                for f in frames:
                    rgb_img = f["rgba"].clamp(min=0, max=1)
                    texture.bake_view(tex, count, owner, rgb_img[..., :3], f["pix"], f["bary"], f["zbuf"], face_uvs)

            row["bake_ms_per_view"] = timed(kernels, args.repeats, views)
            row["tail_ms_per_view"] = timed(tail, args.repeats, views)
            row["tail_peak_mb"] = peak_mb(tail)
            tex.copy_(fill), count.zero_()
            tail()
            assert bool((owner == -1).all())
            ours_tex, ours_count = tex / count.clamp(min=1), count.clone()
            row["texels_seen"] = int((count > 0).sum())
            del tex, count

            row["torch_tail_ms_per_view"] = row["torch_sample_ms_per_view"] = row["torch_tail_peak_mb"] = row["count_equal"] = row["texels_equal"] = None
            if not args.no_torch:
                index_map = torch.cartesian_prod(torch.arange(T, device=dev), torch.arange(T, device=dev)).reshape(T, T, 2)
                index_map = torch.cat([index_map, torch.zeros_like(index_map[..., 0:1])], dim=-1)[None].float()
                ref_tex, ref_count = fill.clone(), torch.zeros((T, T, 1), device=dev)

                def torch_views():
                    for f in frames:
                        torch_tail(ref_tex, ref_count, index_map, f["rgba"], f["pix"], f["bary"], f["zbuf"], f["dists"], face_uvs)

                def torch_samples():
                    for f in frames:
                        torch_sample_and_blend(index_map, f["pix"], f["bary"], f["zbuf"], f["dists"], face_uvs)

                row["torch_tail_ms_per_view"] = timed(torch_views, args.repeats, views)
                row["torch_sample_ms_per_view"] = timed(torch_samples, args.repeats, views)
                row["torch_tail_peak_mb"] = peak_mb(torch_views)
                ref_tex.copy_(fill), ref_count.zero_()
                torch_views()
                row["count_equal"] = bool(torch.equal(ref_count, ours_count))
                same = ((ref_tex / ref_count.clamp(min=1)) == ours_tex).all(dim=-1)
                row["texels_equal"] = round(float(same.float().mean()), 6)
                del index_map, ref_tex, ref_count, same
            print(json.dumps(row), flush=True)
            del frames, fill, ours_tex, ours_count


if __name__ == "__main__":
    main()
