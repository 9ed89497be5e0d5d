#!/usr/bin/env python
"""simple_knn's distCUDA2 (the mean squared distance to the three nearest neighbours, autovfx_amd/knn.py) timed on the GPU, one JSON
line per (P, distribution).

* ``hip_ms``: ``mean_dist3`` -- median of ``--repeats`` device-event timings of single calls, after ``--warmup`` untimed ones;
* ``brute_ms``: the contract as a chunked brute force in torch on the same GPU (P <= 100k only; its bits are compared too:
  ``brute_equal``);
* ``ckdtree_ms``: ``scipy.spatial.cKDTree(pts).query(pts, k=4, workers=16)`` on the CPU, tree build included, when scipy imports.
``comparators`` lists the ones that ran.  Distributions: ``cube`` (uniform in [-1, 1]^3), ``clusters`` (Gaussian blobs of sigma 0.05
and one far outlier per 10 000 points that stretches the bounds, as in a COLMAP cloud).

Usage: ``python scripts/bench_knn.py [--points 1000000 3000000] [--kinds cube clusters] [--repeats 10] [--warmup 3]``.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from autovfx_amd.knn import FLT_MAX, mean_dist3     # noqa: E402


def points(kind, P, seed=0):
    g = np.random.default_rng(seed)
    if kind == "cube":
        pts = g.uniform(-1, 1, (P, 3))
    elif kind == "clusters":
        k = max(1, P // 5000)
        pts = g.uniform(-5, 5, (k, 3))[g.integers(0, k, P)] + g.normal(0, 0.05, (P, 3))
        n_out = max(1, P // 10000)
        pts[g.choice(P, n_out, replace=False)] = g.uniform(-1, 1, (n_out, 3)) * 1e4
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(pts, dtype=np.float32)


def brute(pts, chunk=2048):
    P = pts.shape[0]
    big = torch.tensor(FLT_MAX, dtype=torch.float32, device=pts.device)
    three = torch.full((chunk,), 3.0, dtype=torch.float32, device=pts.device)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    out = torch.empty(P, dtype=torch.float32, device=pts.device)
    for a in range(0, P, chunk):
        b = min(P, a + chunk)
        q = pts[a:b]
        dx = x[None, :] - q[:, 0:1]
        d = dx * dx
        dy = y[None, :] - q[:, 1:2]
        d = d + dy * dy
        dz = z[None, :] - q[:, 2:3]
        d = d + dz * dz
        d[torch.arange(b - a, device=pts.device), torch.arange(a, b, device=pts.device)] = big
        d = torch.where(d < big, d, big)
        d = torch.cat([d, big.expand(b - a, 3)], 1)
        s = torch.topk(d, 3, dim=1, largest=False).values.sort(dim=1).values
        out[a:b] = ((s[:, 0] + s[:, 1]) + s[:, 2]) / three[:b - a]
    return out


def time_gpu(fn, repeats, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[1_000_000, 3_000_000])
    ap.add_argument("--kinds", nargs="+", default=["cube", "clusters"])
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-ckdtree", action="store_true")
    args = ap.parse_args()
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None
    dev = torch.device("cuda", 0)
    for P in args.points:
        for kind in args.kinds:
            host = points(kind, P)
            pts = torch.from_numpy(host).to(dev)
            row = {"P": P, "kind": kind, "comparators": []}
            row["hip_ms"] = round(time_gpu(lambda: mean_dist3(pts), args.repeats, args.warmup), 4)
            if P <= 100_000:
                row["brute_ms"] = round(time_gpu(lambda: brute(pts), 3, 1), 3)
                got, want = mean_dist3(pts), brute(pts)
                torch.cuda.synchronize()
                row["brute_equal"] = bool(torch.equal(got.view(torch.int32), want.view(torch.int32)))
                row["comparators"].append("torch_brute")
            if cKDTree is not None and not args.no_ckdtree:
                t0 = time.perf_counter()
                cKDTree(host).query(host, k=4, workers=16)
                row["ckdtree_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
                row["comparators"].append("scipy_ckdtree")
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
