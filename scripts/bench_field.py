#!/usr/bin/env python
"""SuGaR's density field (autovfx_amd/field.py) timed on the GPU against the reference-shaped torch expressions, one JSON line per
(P, call shape).

* call shapes: ``train`` (``get_field_values`` as the trainers call it: density, opacities and beta) and ``density`` (``compute_density``
  alone); ``--samples`` samples in random order, their ``--K`` nearest Gaussians from ``autovfx_amd.knn.knn_points``;
* ``fused_fwd_ms`` / ``fused_fwdbwd_ms``: ``field_values`` and ``field_values`` + ``backward()`` of a weighted sum of the outputs, gradients
  into the samples, centres, matrices, strengths and minimum scales; ``torch_*``: the same with the gather / batched product / exp / sum
  in torch.  Median of ``--repeats`` device-event timings after ``--warmup`` untimed calls; ``*_peak_mb``: ``torch.cuda.max_memory_allocated``
  over one call, above what was allocated before it;
* ``--only-fused``: no torch comparator (for a run under ``rocprofv3 --kernel-trace --stats``, whose per-kernel times give the achieved
  bytes per second: 64 B per (sample, neighbour), 8 K + 12 B per sample in, 4 (K + 2) B per sample out).

Usage: ``python scripts/bench_field.py [--points 1000000 3000000] [--samples 1000000] [--K 16] [--repeats 10] [--warmup 3] [--only-fused]``.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, ROOT)
from autovfx_amd.field import field_values           # noqa: E402
from autovfx_amd.knn import knn_points               # noqa: E402
from bench_knn import time_gpu                       # noqa: E402


def scene(P, N, K, dev):
    g = torch.Generator(device="cpu").manual_seed(P)
    centers = torch.rand(P, 3, generator=g)
    scaling = torch.exp(torch.randn(P, 3, generator=g) * 0.35 + np.log(0.6 * P ** (-1 / 3)))
    q = torch.nn.functional.normalize(torch.randn(P, 4, generator=g), dim=1)
    w, a, b, c = q.unbind(1)
    R = torch.stack([1 - 2 * (b * b + c * c), 2 * (a * b - w * c), 2 * (a * c + w * b), 2 * (a * b + w * c), 1 - 2 * (a * a + c * c), 2 * (b * c - w * a),
                     2 * (a * c - w * b), 2 * (b * c + w * a), 1 - 2 * (a * a + b * b)], 1).reshape(P, 3, 3)
    M = R / scaling[:, None, :]
    strengths = torch.sigmoid(torch.randn(P, 1, generator=g) * 1.5 + 1.0)
    x = centers[torch.randint(0, P, (N,), generator=g)] + torch.randn(N, 3, generator=g) * scaling.mean() * 1.2
    t = {k: v.to(dev).requires_grad_() for k, v in dict(x=x, centers=centers, M=M, strengths=strengths, scaling=scaling).items()}
    t["idx"] = knn_points(t["x"].detach()[None], t["centers"].detach()[None], K=K).idx[0].contiguous()
    t["weights"] = [torch.randn(N, device=dev), torch.randn(N, K, device=dev), torch.randn(N, device=dev)]
    return t


def fused(t, shape):
    train = shape == "train"
    m = t["scaling"].min(dim=-1)[0] if train else None
    return field_values(t["x"], t["idx"], t["centers"], t["M"], t["strengths"], m, 1.0, want_opacities=train, want_beta=train)


def dense(t, shape):
    idx = t["idx"]
    w = (t["M"][idx].transpose(-1, -2) @ (t["x"][:, None] - t["centers"][idx])[..., None])[..., 0]
    o = 1.0 * t["strengths"][idx][..., 0] * torch.exp(-0.5 * (w * w).sum(-1).clamp(0.0, 1e8))
    if shape != "train":
        return o.sum(-1), None, None
    return o.sum(-1), o, t["scaling"].min(dim=-1)[0][idx].mean(dim=1)


def with_backward(fn, t, shape):
    def run():
        for k in ("x", "centers", "M", "strengths", "scaling"):
            t[k].grad = None
        outs = fn(t, shape)
        sum((w * o).sum() for w, o in zip(t["weights"], outs) if o is not None).backward()
    return run


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[1_000_000, 3_000_000])
    ap.add_argument("--samples", type=int, default=1_000_000)
    ap.add_argument("--K", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only-fused", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for P in args.points:
        t = scene(P, args.samples, args.K, dev)
        for shape in ("train", "density"):
            row = {"P": P, "N": args.samples, "K": args.K, "shape": shape, "device": torch.cuda.get_device_name(0)}
            fns = [("fused", fused)] + ([] if args.only_fused else [("torch", dense)])
            for name, fn in fns:
                with torch.no_grad():
                    row[f"{name}_fwd_ms"] = round(time_gpu(lambda: fn(t, shape), args.repeats, args.warmup), 3)
                    row[f"{name}_fwd_peak_mb"] = peak_mb(lambda: fn(t, shape))
                row[f"{name}_fwdbwd_ms"] = round(time_gpu(with_backward(fn, t, shape), args.repeats, args.warmup), 3)
                row[f"{name}_fwdbwd_peak_mb"] = peak_mb(with_backward(fn, t, shape))
            if not args.only_fused:
                a, b = fused(t, shape)[0], dense(t, shape)[0]
                row["max_density_difference"] = float((a - b).detach().abs().max())
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
