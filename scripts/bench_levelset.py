#!/usr/bin/env python
"""The level-surface ray march of SuGaR's coarse mesh extraction (autovfx_amd/levelset.py) timed on the GPU, one JSON line per ray
count.  There is no torch comparator in this script: ``sugar_model.py:1853-1950`` written in torch, in the reference's passes of 2 M
samples (a batched 3x3 product over 32 M matrices), ended in a memory-access fault inside torch's own kernels on the MI355X before it
gave a time, and is not kept.

* scene: ``--points`` Gaussians in the unit cube with scales near their spacing and their ``--K`` nearest neighbours
  (``autovfx_amd.knn.knn_points``); a ray starts near a random Gaussian, carries that Gaussian's neighbour row and a standard deviation
  near the scales, as the extractor's rays do;
* ``kernel_ms``: ``gsr_level_surface`` alone into preallocated outputs (the pack of the P records and the march);
  ``fused_tail_ms``: what the drop-in does after the rays are built -- ``level_surface`` and the per-level compaction of points,
  normals, pixel and Gaussian indices by boolean indexing.  Median of ``--repeats`` device-event timings after ``--warmup``
  untimed calls; ``*_peak_mb``: ``torch.cuda.max_memory_allocated`` over one call, above what was allocated before it;
* ``bytes_per_ray``: what the kernel must move per ray -- 2 K records of 64 B (one walk for the densities, one for the normals), the
  8 K B index row, 28 B of ray, 29 B out per level -- and ``kernel_gbytes_per_s`` = rays x that / ``kernel_ms``; ``expf_per_ray`` =
  K (S + hits) evaluations of the pair.

Usage: ``python scripts/bench_levelset.py [--points 1000000] [--rays 100000 700000 2000000] [--K 16] [--repeats 10] [--warmup 3]``.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, ROOT)
from autovfx_amd import _lib                            # noqa: E402
from autovfx_amd.knn import knn_points                  # noqa: E402
from autovfx_amd.levelset import level_surface          # noqa: E402
from bench_field import peak_mb                         # noqa: E402
from bench_knn import time_gpu                          # noqa: E402

LEVELS = [0.1, 0.3, 0.5]
S = 21


def scene(P, K, dev):
    g = torch.Generator(device="cpu").manual_seed(P)
    centers = torch.rand(P, 3, generator=g)
    scaling = torch.exp(torch.randn(P, 3, generator=g) * 0.35 + np.log(0.6 * P ** (-1 / 3)))
    q = torch.nn.functional.normalize(torch.randn(P, 4, generator=g), dim=1)
    w, a, b, c = q.unbind(1)
    R = torch.stack([1 - 2 * (b * b + c * c), 2 * (a * b - w * c), 2 * (a * c + w * b), 2 * (a * b + w * c), 1 - 2 * (a * a + c * c), 2 * (b * c - w * a),
                     2 * (a * c - w * b), 2 * (b * c + w * a), 1 - 2 * (a * a + b * b)], 1).reshape(P, 3, 3)
    t = dict(centers=centers.to(dev), M=(R / scaling[:, None, :]).to(dev), strengths=torch.sigmoid(torch.randn(P, 1, generator=g) * 1.5 + 1.0).to(dev),
             scale=float(scaling.mean()))
    t["knn_idx"] = knn_points(t["centers"][None], t["centers"][None], K=K).idx[0].contiguous()
    return t


def rays(t, n, dev):
    g = torch.Generator(device="cpu").manual_seed(n)
    first = torch.randint(0, t["centers"].shape[0], (n,), generator=g).to(dev)
    r = dict(origins=t["centers"][first] + torch.randn(n, 3, generator=g).to(dev) * t["scale"] * 0.3,
             dirs=torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1).to(dev),
             stds=(torch.exp(torch.randn(n, generator=g) * 0.3) * t["scale"]).to(dev), gaussian_idx=first, pixel_idx=torch.arange(n, device=dev))
    r["idx"] = t["knn_idx"][first]
    return r


def fused_tail(t, r):
    found = level_surface(r["origins"], r["dirs"], r["stds"], r["idx"], t["centers"], t["M"], t["strengths"], LEVELS, S, 3.0, 1.0, want_normals=True)
    out = {}
    for l, level in enumerate(LEVELS):
        keep = found["hit"][l]
        out[level] = {"intersection_points": found["points"][l][keep], "pixel_idx": r["pixel_idx"][keep], "gaussian_idx": r["gaussian_idx"][keep],
                      "normals": found["normals"][l][keep]}
    return out


def kernel_alone(t, r):
    n, K, P, L, dev = r["origins"].shape[0], r["idx"].shape[1], t["centers"].shape[0], len(LEVELS), r["origins"].device
    hit = torch.empty((L, n), dtype=torch.uint8, device=dev)
    tt, points, normals = torch.empty((L, n), device=dev), torch.empty((L, n, 3), device=dev), torch.empty((L, n, 3), device=dev)
    rng = torch.linspace(-3.0, 3.0, S).to(dev)
    levels = (ctypes.c_float * 8)(*LEVELS)
    scratch, nbytes = _lib.scratch("gsr_field_scratch_bytes", P, device=dev)
    strengths = t["strengths"].contiguous()

    def run():
        _lib.call("gsr_level_surface", n, K, P, S, L, r["origins"].data_ptr(), r["dirs"].data_ptr(), r["stds"].data_ptr(), r["idx"].data_ptr(),
                  t["centers"].data_ptr(), t["M"].data_ptr(), strengths.data_ptr(), 1.0, rng.data_ptr(), ctypes.byref(levels), hit.data_ptr(),
                  tt.data_ptr(), points.data_ptr(), normals.data_ptr(), None, scratch.data_ptr(), nbytes, device=dev)
        return hit

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--rays", type=int, nargs="+", default=[100_000, 700_000, 2_000_000])
    ap.add_argument("--K", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    t = scene(args.points, args.K, dev)
    with torch.no_grad():
        for n in args.rays:
            r = rays(t, n, dev)
            row = {"P": args.points, "rays": n, "K": args.K, "S": S, "levels": LEVELS, "device": torch.cuda.get_device_name(0)}
            run = kernel_alone(t, r)
            row["kernel_ms"] = round(time_gpu(run, args.repeats, args.warmup), 3)
            hits = float(run().sum()) / n
            row["hits_per_ray"] = round(hits, 3)
            row["bytes_per_ray"] = 2 * args.K * 64 + 8 * args.K + 28 + 29 * len(LEVELS)
            row["kernel_gbytes_per_s"] = round(n * row["bytes_per_ray"] / row["kernel_ms"] / 1e6, 1)
            row["expf_per_ray"] = round(args.K * (S + hits), 1)
            row["fused_tail_ms"] = round(time_gpu(lambda: fused_tail(t, r), args.repeats, args.warmup), 3)
            row["fused_tail_peak_mb"] = peak_mb(lambda: fused_tail(t, r))
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
