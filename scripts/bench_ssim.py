#!/usr/bin/env python
"""The training loss's SSIM (``loss_utils.ssim``) timed on the GPU, both ways, one JSON line.

* per size: ``ssim_restated`` (the reference's graph: five depthwise conv2d and the elementwise ops) against the fused kernels
  (``autovfx_amd.ssim.ssim``), forward alone (no autograd: the metrics path) and forward + backward (the training path, the
  gradient for img1); the median of ``--regions`` device-event regions of ``--iters`` calls each, after ``--warmup`` untimed calls;
* ``c3_train_iteration``: one iteration of the reference's training loop with its real loss, ``0.8 L1 + 0.2 (1 - ssim)`` on
  ``renderer.render()``'s RGBA, plus ``backward()`` -- bench.py's ``training_render_iteration`` with the SSIM term it leaves out --
  with each of the two SSIMs, and with the L1 term alone for scale.

Usage: ``python scripts/bench_ssim.py [--regions 7] [--iters 10] [--warmup 3] [--steps 10]``.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from autovfx_amd.ssim import ssim, ssim_restated   # noqa: E402

SIZES = [("4x540x960", (4, 540, 960), True), ("4x1080x1920", (4, 1080, 1920), True), ("3x1080x1920", (3, 1080, 1920), True),
         ("1x4x1080x1920_per_image", (1, 4, 1080, 1920), False)]


def median_ms(fn, regions, iters, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(regions):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / iters)
    return round(statistics.median(times), 4)


def size_rows(dev, args):
    rows = {}
    for name, shape, size_average in SIZES:
        g = torch.Generator(device=dev).manual_seed(0)
        img = torch.rand(shape, device=dev, generator=g)
        gt = (img + 0.05 * torch.rand(shape, device=dev, generator=g)).clamp(0, 1)
        x = img.clone().requires_grad_(True)
        row = {}
        for side, fn in (("restated", ssim_restated), ("fused", ssim)):
            def fwd():
                with torch.no_grad():
                    fn(img, gt, 11, size_average)

            def fwd_bwd():
                x.grad = None
                v = fn(x, gt, 11, size_average)
                (1.0 - v).sum().backward()

            row[f"{side}_fwd_ms"] = median_ms(fwd, args.regions, args.iters, args.warmup)
            row[f"{side}_fwd_bwd_ms"] = median_ms(fwd_bwd, args.regions, args.iters, args.warmup)
        row["speedup_fwd"] = round(row["restated_fwd_ms"] / row["fused_fwd_ms"], 2)
        row["speedup_fwd_bwd"] = round(row["restated_fwd_bwd_ms"] / row["fused_fwd_bwd_ms"], 2)
        # HBM bytes the fused kernels cannot avoid: forward reads x, y and writes the three maps; backward reads the maps, x, y
        # and writes the gradient (4 bytes each)
        n = img.numel()
        row["fused_fwd_bwd_min_bytes"] = 4 * n * (2 + 3 + 3 + 2 + 1)
        rows[name] = row
    return rows


def c3_iteration(dev, args):
    import bench
    from autovfx_amd import renderer
    b = bench.Bench("c3", dev, None, boundary="op")
    m = bench.ReferenceGetters(b.cloud, b.cloud.sh_degree)
    params = ("_xyz", "_scaling", "_rotation", "_opacity", "_features_dc", "_features_rest")
    for k in params:
        setattr(m, k, getattr(m, k).detach().clone().requires_grad_(True))
    target = torch.rand(4, b.H, b.W, device=dev)
    frames = [(10 + 7 * j) % b.F for j in range(args.steps)]
    for f in frames:
        b.cam(f)

    def loop(fn):
        def run():
            for f in frames:
                for k in params:
                    getattr(m, k).grad = None
                img = renderer.render(b.cam(f), m, renderer.PipelineParams, b.bg)["render"]
                loss = (img - target).abs().mean()
                if fn is not None:
                    loss = 0.8 * loss + 0.2 * (1.0 - fn(img, target))
                loss.backward()
        return median_ms(run, args.regions, 1, 2) / len(frames)

    out = {"workload": b.name, "W": b.W, "H": b.H, "steps": len(frames),
           "loss": "0.8 L1 + 0.2 (1 - ssim) on render() RGBA (train.py:99, scene_representation.py:507-515 without LPIPS)"}
    out["l1_only_ms_per_iter"] = round(loop(None), 3)
    out["restated_ssim_ms_per_iter"] = round(loop(ssim_restated), 3)
    out["fused_ssim_ms_per_iter"] = round(loop(ssim), 3)
    out["speedup"] = round(out["restated_ssim_ms_per_iter"] / out["fused_ssim_ms_per_iter"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--skip-train", action="store_true", help="the sizes only (no renderer iteration)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ssim.py needs a GPU")
    dev = torch.device("cuda", 0)
    out = {"bench": "ssim", "device": torch.cuda.get_device_name(0), "sizes": size_rows(dev, args)}
    if not args.skip_train:
        out["c3_train_iteration"] = c3_iteration(dev, args)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
