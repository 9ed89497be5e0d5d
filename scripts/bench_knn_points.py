#!/usr/bin/env python
"""pytorch3d's knn_points (autovfx_amd/knn.py: the K nearest neighbours with indices) timed on the GPU, one JSON line per
(P, distribution, query).

* ``hip_ms``: ``knn_points`` at ``--K`` (default 16) -- median of ``--repeats`` device-event timings of single calls, after
  ``--warmup`` untimed ones.  ``query``: ``self`` (the same tensor twice, as ``SuGaR.reset_neighbors``) or ``cross`` (``--samples``
  points drawn around the cloud, as ``get_gaussians_closest_to_samples``);
* ``brute_ms``: the contract as a chunked brute force in torch on the same GPU (P <= 100k only; ``brute_equal``: its distances'
  bits are compared too);
* ``ckdtree_ms``: ``scipy.spatial.cKDTree(p2).query(p1, k=K, workers=16)`` on the CPU, tree build included, when scipy imports.
``comparators`` lists the ones that ran.  Distributions: ``cube`` (uniform in [-1, 1]^3), ``clusters`` (Gaussian blobs of sigma 0.05
and one far outlier per 10 000 points that stretches the bounds, as in a COLMAP cloud).

Usage: ``python scripts/bench_knn_points.py [--points 100000 1000000 3000000] [--kinds cube clusters] [--queries self cross]
[--samples 1000000] [--dense-samples] [--K 16] [--repeats 10] [--warmup 3] [--no-ckdtree]``.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, ROOT)
from autovfx_amd.knn import FLT_MAX, knn_points     # noqa: E402
from bench_knn import points, time_gpu               # noqa: E402


def brute(p1, p2, K, chunk=2048):
    inf = torch.tensor(float("inf"), dtype=torch.float32, device=p2.device)
    x, y, z = p2[:, 0], p2[:, 1], p2[:, 2]
    out = torch.empty(p1.shape[0], K, dtype=torch.float32, device=p2.device)
    for a in range(0, p1.shape[0], chunk):
        q = p1[a:a + chunk]
        dx = x[None, :] - q[:, 0:1]
        d = dx * dx
        dy = y[None, :] - q[:, 1:2]
        d = d + dy * dy
        dz = z[None, :] - q[:, 2:3]
        d = d + dz * dz
        d = torch.where(d < FLT_MAX, d, inf)
        out[a:a + chunk] = torch.topk(d, K, dim=1, largest=False, sorted=True).values
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[100_000, 1_000_000, 3_000_000])
    ap.add_argument("--kinds", nargs="+", default=["cube", "clusters"])
    ap.add_argument("--queries", nargs="+", default=["self", "cross"], choices=["self", "cross"])
    ap.add_argument("--samples", type=int, default=1_000_000)
    ap.add_argument("--dense-samples", action="store_true", help="cross query: no samples around the far outliers of `clusters`")
    ap.add_argument("--K", type=int, default=16)
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
            host2 = points(kind, P)
            p2 = torch.from_numpy(host2).to(dev)
            for query in args.queries:
                if query == "self":
                    host1, p1 = host2, p2
                else:
                    g = np.random.default_rng(1)
                    pick = g.integers(0, P, args.samples)
                    if args.dense_samples:   # the samples around a far outlier redrawn around one point of the dense part
                        dense = np.abs(host2).max(1) < 100
                        pick = np.where(dense[pick], pick, pick[np.argmax(dense[pick])])
                    host1 = np.ascontiguousarray(host2[pick] + g.normal(0, 0.02, (args.samples, 3)), dtype=np.float32)
                    p1 = torch.from_numpy(host1).to(dev)
                row = {"P": P, "kind": kind, "query": query, "P1": int(p1.shape[0]), "K": args.K, "dense_samples": args.dense_samples, "comparators": []}
                row["hip_ms"] = round(time_gpu(lambda: knn_points(p1[None], p2[None], K=args.K), args.repeats, args.warmup), 4)
                if P <= 100_000 and p1.shape[0] <= 100_000:
                    row["brute_ms"] = round(time_gpu(lambda: brute(p1, p2, args.K), 3, 1), 3)
                    got, want = knn_points(p1[None], p2[None], K=args.K).dists[0], brute(p1, p2, args.K)
                    torch.cuda.synchronize()
                    row["brute_equal"] = bool(torch.equal(got.view(torch.int32), want.view(torch.int32)))
                    row["comparators"].append("torch_brute")
                if cKDTree is not None and not args.no_ckdtree:
                    t0 = time.perf_counter()
                    cKDTree(host2).query(host1, k=args.K, workers=16)
                    row["ckdtree_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
                    row["comparators"].append("scipy_ckdtree")
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
