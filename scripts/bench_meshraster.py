#!/usr/bin/env python
"""The triangle-mesh z-buffer of SuGaR's mesh extraction (autovfx_amd/meshraster.py) timed on the GPU, one JSON line per (Gaussians, K).
There is no comparator in this script: pytorch3d's ``rasterize_meshes`` is a CUDA kernel and does not run on the MI355X.

* scene: ``--gaussians`` flat diamonds of two triangles each, built on the device: centres uniform over a little more than the view of a
  pinhole camera at depths 2..10, a random orientation each, log-normal sizes around ``--size`` (world units; 0.02 is about 4 pixels at
  1080 x 1920 in the middle of the depth range), projected to pytorch3d's NDC (+x left, +y up, the shorter image side spans [-1, 1],
  z the view depth);
* ``count_ms``: ``gsr_mesh_raster_count`` -- the binning kernel, the scan and the host read of the pair total, so it is a host-visible
  time, measured with device events around a call that ends in a stream synchronise; ``raster_ms``: ``gsr_mesh_raster`` into
  preallocated outputs -- the list fill and the per-tile z-buffer; ``call_ms``: ``rasterize_face_verts`` whole, with its allocations.
  Median of ``--repeats`` device-event timings after ``--warmup`` untimed calls.  Per-kernel times come from a kernel trace of this
  script (``rocprofv3 --kernel-trace --stats``), not from here;
* ``pairs``: the (tile, face) pairs, the total length of the tile lists; ``listed_per_pixel``: the mean number of filled slots;
* ``bytes``: what the four kernels must move -- per face 36 B of vertices and 12 B of plan in the count and 12 B back in the fill, per
  pair 4 B written and 4 + 36 B read (the list entry and its face's vertices), per output slot 28 B -- and ``hbm_floor_ms`` = those
  bytes at ``--hbm-tbps`` (6.29 TB/s: the measured copy rate of the MI355X); ``share_of_hbm_rate`` = that over ``count_ms + raster_ms``;
* ``peak_mb``: ``torch.cuda.max_memory_allocated`` over one whole call, above what was allocated before it (outputs included).

Usage: ``python scripts/bench_meshraster.py [--gaussians 1000000 3000000] [--K 10 1] [--size 0.02] [--repeats 10] [--warmup 3]``.
"""
import argparse
import ctypes
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, ROOT)
from autovfx_amd import _lib                                    # noqa: E402
from autovfx_amd.meshraster import rasterize_face_verts         # noqa: E402
from bench_field import peak_mb                                 # noqa: E402
from bench_knn import time_gpu                                  # noqa: E402


def scene(P, H, W, size, dev):
    """``face_verts [2 P, 3, 3]`` and the three index tensors of one mesh."""
    g = torch.Generator(device=dev).manual_seed(P)
    rand = lambda *shape: torch.rand(*shape, generator=g, device=dev)
    randn = lambda *shape: torch.randn(*shape, generator=g, device=dev)
    aspect = W / H
    focal = 1.2                                                  # NDC units per unit of x / z
    z = 2.0 + 8.0 * rand(P)
    ndc = (rand(P, 2) * 2.2 - 1.1) * torch.tensor([max(aspect, 1.0), max(1.0 / aspect, 1.0)], device=dev)
    centre = torch.cat([ndc * z[:, None] / focal, z[:, None]], 1)
    u = torch.nn.functional.normalize(randn(P, 3), dim=1)
    v = torch.nn.functional.normalize(torch.cross(u, randn(P, 3), dim=1), dim=1)
    s = (size * torch.exp(0.5 * randn(P)))[:, None]
    a, b, c, d = centre + s * u, centre + s * v, centre - s * u, centre - s * v
    world = torch.stack([torch.stack([a, b, c], 1), torch.stack([c, d, a], 1)], 1).reshape(2 * P, 3, 3)
    depth = world[..., 2].clamp_min(1e-3)
    face_verts = torch.stack([focal * world[..., 0] / depth, focal * world[..., 1] / depth, world[..., 2]], -1).contiguous()
    F = 2 * P
    return (face_verts, torch.zeros(1, dtype=torch.int64, device=dev), torch.full((1,), F, dtype=torch.int64, device=dev),
            torch.full((F,), -1, dtype=torch.int64, device=dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, nargs="+", default=[1_000_000, 3_000_000])
    ap.add_argument("--K", type=int, nargs="+", default=[10, 1])
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--size", type=float, default=0.02)
    ap.add_argument("--hbm-tbps", type=float, default=6.29)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    H, W = args.height, args.width
    with torch.no_grad():
        for P in args.gaussians:
            fv, first, num, nbr = scene(P, H, W, args.size, dev)
            F = int(fv.shape[0])
            plan, plan_bytes = _lib.scratch("gsr_mesh_raster_plan_bytes", F, 1, H, W, device=dev)
            total = ctypes.c_int64(0)

            def count():
                _lib.call("gsr_mesh_raster_count", F, 1, fv.data_ptr(), first.data_ptr(), num.data_ptr(), H, W, 0, plan.data_ptr(), plan_bytes,
                          ctypes.byref(total), device=dev)

            count_ms = time_gpu(count, args.repeats, args.warmup)
            pairs, pair_bytes = _lib.scratch("gsr_mesh_raster_pair_bytes", total.value, device=dev)
            for K in args.K:
                outs = (torch.empty((1, H, W, K), dtype=torch.int64, device=dev), torch.empty((1, H, W, K), device=dev),
                        torch.empty((1, H, W, K, 3), device=dev), torch.empty((1, H, W, K), device=dev))

                def raster():
                    _lib.call("gsr_mesh_raster", F, 1, fv.data_ptr(), first.data_ptr(), num.data_ptr(), nbr.data_ptr(), H, W, 0.0, K, 1, 0, 0,
                              plan.data_ptr(), plan_bytes, total.value, pairs.data_ptr(), pair_bytes, *(o.data_ptr() for o in outs), device=dev)

                whole = lambda: rasterize_face_verts(fv, first, num, nbr, (H, W), 0.0, K, None, 50_000, True, False, False)
                row = {"gaussians": P, "faces": F, "H": H, "W": W, "K": K, "size": args.size, "device": torch.cuda.get_device_name(0)}
                row["count_ms"] = round(count_ms, 3)
                row["raster_ms"] = round(time_gpu(raster, args.repeats, args.warmup), 3)
                row["call_ms"] = round(time_gpu(whole, args.repeats, args.warmup), 3)
                row["pairs"] = int(total.value)
                row["listed_per_pixel"] = round(float((outs[0] >= 0).sum()) / (H * W), 2)
                row["bytes"] = 60 * F + 44 * int(total.value) + 28 * H * W * K
                row["hbm_floor_ms"] = round(row["bytes"] / (args.hbm_tbps * 1e9), 3)
                row["share_of_hbm_rate"] = round(row["hbm_floor_ms"] / (row["count_ms"] + row["raster_ms"]), 3)
                row["peak_mb"] = peak_mb(whole)
                assert math.isfinite(row["raster_ms"])
                print(json.dumps(row), flush=True)
                del outs


if __name__ == "__main__":
    main()
