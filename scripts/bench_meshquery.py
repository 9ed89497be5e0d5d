#!/usr/bin/env python
"""The closest-triangle query (autovfx_amd/meshquery.py) timed on the GPU, one JSON line per measurement.

* ``kind: "query"`` -- per (faces, queries): ``plan_ms`` (``meshquery.plan``, the tree of one mesh) and ``query_ms``
  (``closest_triangles`` with that plan, closest points included, as a caller gets it: the queries' Morton sort and the answers' way
  back are in it), medians of ``--repeats`` device-event timings after ``--warmup`` untimed calls.  The mesh is a sphere of ``faces``
  nearly even triangles with a radial ripple; the queries are drawn around its surface (a random point of a random face, pushed off
  by a normal step of two edge lengths) in random order.  ``query_unsorted_ms``: the same batch without the sort, the
  kernel on the caller's random order; ``query_presorted_ms``: likewise on the batch already in Morton order, the
  kernel alone at its best.
  ``checked``: that many queries compared with the numpy restatement of the contract (its pruned mode: the brute force's answers
  in a fraction of its time), bit for bit (``check_equal``).
* ``kind: "melt_mask"`` -- one melting frame's mask, from the face centres (a host float32 array) to the mask over the object's
  Gaussians, in both modes of ``AUTOVFX_AMD_MELT_CLOSEST``: ``gpu_ms`` (upload, one query, flag scatter and gather, host clock around
  a device synchronise) and ``host_ms`` (``compute_closest_points`` of the process's ``open3d``, ``np.isin``, the mask's upload).
  Without ``open3d`` there is no host time: the line says so (``host: "open3d is not installed: not measured"``).

Usage: ``python scripts/bench_meshquery.py [--faces 100000 1000000] [--queries 60000 1000000 3000000] [--repeats 10] [--warmup 3]
[--check 512] [--gaussians 200000] [--centres 50000]``.
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
from autovfx_amd import meshquery     # noqa: E402


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


def time_host(fn, repeats, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(times)


def rippled_sphere(F):
    """About ``F`` faces (12 n^2): the six faces of a cube, n x n cells each, pushed onto a sphere whose radius ripples by 5 %."""
    n = max(1, int(np.ceil(np.sqrt(F / 12.0))))
    t = np.linspace(-1.0, 1.0, n + 1)
    u, v = np.meshgrid(t, t, indexing="ij")
    one = np.ones_like(u)
    cell = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).ravel()
    quad = np.stack((cell, cell + n + 1, cell + n + 2, cell, cell + n + 2, cell + 1), -1).reshape(-1, 3)
    verts, faces = [], []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            cols = [None, None, None]
            cols[axis], cols[(axis + 1) % 3], cols[(axis + 2) % 3] = sign * one, u, v
            p = np.stack(cols, -1).reshape(-1, 3)
            p /= np.linalg.norm(p, axis=1, keepdims=True)
            p *= (1.0 + 0.05 * np.sin(9.0 * p[:, 0]) * np.cos(7.0 * p[:, 1]))[:, None]
            faces.append(quad + sum(len(x) for x in verts))
            verts.append(p)
    return np.concatenate(verts).astype(np.float32), np.concatenate(faces).astype(np.int64)


def around(verts, faces, n, reach, seed):
    g = np.random.default_rng(seed)
    t = verts[faces[g.integers(0, faces.shape[0], n)]]
    w = g.dirichlet((1.0, 1.0, 1.0), n).astype(np.float32)
    return ((t * w[:, :, None]).sum(1) + g.normal(0.0, reach, (n, 3))).astype(np.float32)


def melt_mask_gpu(scene, ids_gaussians, centres):
    """What ``frame_loop._MeltingPlan._mask`` does in ``gpu`` mode."""
    ids = scene.compute_closest_points(centres)["primitive_ids"]
    F = int(scene.plan.F)
    flags = torch.zeros(F + 1, dtype=torch.uint8, device=ids.device)
    flags[torch.where(ids >= 0, ids, F)] = 1
    flags[F] = 0
    return flags[ids_gaussians].to(torch.bool)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--queries", type=int, nargs="+", default=[60_000, 1_000_000, 3_000_000])
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--check", type=int, default=512, help="queries compared with the numpy restatement per mesh (0: none)")
    ap.add_argument("--gaussians", type=int, default=200_000, help="melt_mask: Gaussians of the object")
    ap.add_argument("--centres", type=int, default=50_000, help="melt_mask: faces of the frame's melting mesh")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    try:
        import open3d as o3d
    except ImportError:
        o3d = None
    for F in args.faces:
        verts, faces = rippled_sphere(F)
        edge = float(np.linalg.norm(verts[faces[:, 0]] - verts[faces[:, 1]], axis=1).mean())
        tv, tf = torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev)
        plan_ms = time_gpu(lambda: meshquery.plan(tv, tf), args.repeats, args.warmup)
        plan = meshquery.plan(tv, tf)
        for n in args.queries:
            host_q = around(verts, faces, n, 2.0 * edge, seed=n)
            q = torch.from_numpy(host_q).to(dev)
            row = {"kind": "query", "faces": int(faces.shape[0]), "verts": int(verts.shape[0]), "queries": n, "mean_edge": round(edge, 6),
                   "plan_bytes": int(plan.buffer.numel()), "plan_ms": round(plan_ms, 4)}
            run = lambda pts, sort=True: (meshquery.closest_triangles(pts, tv, tf, plan=plan, return_points=True) if sort else
                                          meshquery._query(pts, plan, True, sort_queries=False))
            row["query_ms"] = round(time_gpu(lambda: run(q), args.repeats, args.warmup), 4)
            row["query_unsorted_ms"] = round(time_gpu(lambda: run(q, False), max(3, args.repeats // 3), 1), 4)
            sorted_q = q[meshquery.morton_order(q)].contiguous()
            row["query_presorted_ms"] = round(time_gpu(lambda: run(sorted_q, False), args.repeats, args.warmup), 4)
            if args.check and n == args.queries[0]:
                got = [t[:args.check].cpu().numpy() for t in run(q)]
                want = meshquery.closest_triangles_host(host_q[:args.check], verts, faces, pruned=True)
                row["checked"] = args.check
                row["check_equal"] = bool(np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
                                          and np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)))
            print(json.dumps(row), flush=True)

        # one melting frame's mask: the object's Gaussians around this mesh, the frame's mesh a shrunk part of it
        g = np.random.default_rng(F)
        host_xyz = around(verts, faces, args.gaussians, edge, seed=3)
        part = g.permutation(faces.shape[0])[:min(args.centres, faces.shape[0])]
        centres = (verts[faces[part]].mean(axis=1) * 0.98).astype(np.float32)
        scene = meshquery.Scene(verts, faces, device=dev)
        ids_gaussians = scene.compute_closest_points(torch.from_numpy(host_xyz).to(dev))["primitive_ids"]
        ids_gaussians = torch.where(ids_gaussians >= 0, ids_gaussians, scene.plan.F)
        row = {"kind": "melt_mask", "faces": int(faces.shape[0]), "gaussians": args.gaussians, "centres": int(centres.shape[0])}
        row["gpu_ms"] = round(time_host(lambda: melt_mask_gpu(scene, ids_gaussians, centres), args.repeats, args.warmup), 4)
        row["gpu_kept"] = int(melt_mask_gpu(scene, ids_gaussians, centres).sum())
        if o3d is None:
            row["host"] = "open3d is not installed: not measured"
        else:
            ray = o3d.t.geometry.RaycastingScene()
            ray.add_triangles(o3d.core.Tensor.from_numpy(verts), o3d.core.Tensor.from_numpy(faces.astype(np.uint32)))
            ids_host = ray.compute_closest_points(o3d.core.Tensor.from_numpy(host_xyz))["primitive_ids"].cpu().numpy()

            def host_mask():
                ids = ray.compute_closest_points(o3d.core.Tensor.from_numpy(centres))["primitive_ids"].cpu().numpy()
                return torch.from_numpy(np.isin(ids_host, ids)).to(dev)

            row["host"] = "open3d " + getattr(o3d, "__version__", "?")
            row["host_ms"] = round(time_host(host_mask, args.repeats, args.warmup), 4)
            row["host_kept"] = int(host_mask().sum())
            row["ids_equal_fraction"] = round(float((ids_host.astype(np.int64) == ids_gaussians.cpu().numpy()).mean()), 6)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
