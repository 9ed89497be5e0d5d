#!/usr/bin/env python
"""The first-hit ray cast (autovfx_amd/meshquery.py: first_hits) timed on the GPU, one JSON line per measurement.

* ``kind: "camera"`` -- per mesh: a 1920 x 1080 pinhole camera inside the mesh, one ray per pixel (``first_hits`` with the mesh's
  plan, barycentrics included, as a caller gets it: the rays' ordering and the answers' way back are in it): ``cast_ms``;
  ``cast_as_given_ms``: the kernel on the rays in row-major pixel order, without the ordering.  Medians of ``--repeats`` device-event
  timings after ``--warmup`` untimed calls.  The mesh is ``bench_meshquery.rippled_sphere``.
* ``kind: "random"`` -- per mesh: ``--rays`` rays from points inside the mesh in random directions, in random order: ``cast_ms`` (asked
  sorted, the sort and the way back in it), ``cast_as_given_ms`` (the kernel on the random order), ``order_ms`` (``ray_order`` alone)
  and, the yardstick, ``closest_ms``: ``closest_triangles`` on the same mesh and plan for as many query points (the rays' true hit
  points pushed off by two edge lengths, in random order, its own sort in it).
  ``checked``: that many rays compared with the numpy restatement of the contract (pruned mode), bit for bit (``check_equal``).
* ``kind: "votes"`` -- per mesh: ``extract.triangle_votes`` over ``--views`` views of ``--view-size`` pixels from inside the mesh,
  masks that keep about half of the pixels; host clock around a device synchronise: ``votes_ms`` and ``per_view_ms``.

No trimesh or Open3D time is taken: the line says whether either is installed.

Usage: ``python scripts/bench_meshrays.py [--faces 100000 1000000] [--rays 1000000] [--views 100] [--view-size 480 640] [--repeats 10]
[--warmup 3] [--check 128]``.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from autovfx_amd import extract, meshquery     # noqa: E402
from bench_meshquery import rippled_sphere, time_gpu, time_host     # noqa: E402


def look_around(k, dev):
    """The k-th camera-to-world matrix of a turn around the y axis at the origin, with a little nod."""
    a, b = 2.0 * np.pi * k / 17.0, 0.3 * np.sin(0.7 * k)
    ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    c2w = np.eye(4)
    c2w[:3, :3] = ry @ rx
    c2w[:3, 3] = (0.1 * np.cos(a), 0.05, 0.1 * np.sin(a))
    return torch.tensor(c2w, dtype=torch.float32, device=dev)


def installed(name):
    try:
        __import__(name)
        return True
    except ImportError:
        return False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--view-size", type=int, nargs=2, default=[480, 640], metavar=("H", "W"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--check", type=int, default=128, help="rays compared with the numpy restatement per mesh (0: none)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    others = {name: installed(name) for name in ("trimesh", "open3d")}
    for F in args.faces:
        verts, faces = rippled_sphere(F)
        edge = float(np.linalg.norm(verts[faces[:, 0]] - verts[faces[:, 1]], axis=1).mean())
        tv, tf = torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev)
        plan = meshquery.plan(tv, tf)
        base = {"faces": int(faces.shape[0]), "verts": int(verts.shape[0]), "host_libraries_installed": others}
        cast = lambda o, d: meshquery.first_hits(o, d, tv, tf, plan=plan, return_bary=True)
        as_given = lambda o, d: meshquery._cast(o, d, plan, True, order=None)

        # a 1080p camera inside the mesh
        h, w = 1080, 1920
        K = torch.tensor([[1000.0, 0, w / 2], [0, 1000.0, h / 2], [0, 0, 1]], device=dev)
        c2w = look_around(3, dev)
        d = (extract.ray_directions(h, w, K) @ c2w[:3, :3].T).reshape(-1, 3).contiguous()
        o = c2w[:3, 3].expand_as(d).contiguous()
        row = dict(base, kind="camera", rays=h * w)
        row["cast_ms"] = round(time_gpu(lambda: cast(o, d), args.repeats, args.warmup), 4)
        row["cast_as_given_ms"] = round(time_gpu(lambda: as_given(o, d), args.repeats, args.warmup), 4)
        row["hit_fraction"] = round(float((cast(o, d)[0] >= 0).float().mean()), 4)
        print(json.dumps(row), flush=True)

        # random rays from inside, in random order
        g = np.random.default_rng(F)
        n = args.rays
        host_o = (0.5 * g.uniform(-1, 1, (n, 3)) / np.sqrt(3.0)).astype(np.float32)
        host_d = g.normal(size=(n, 3)).astype(np.float32)
        o, d = torch.from_numpy(host_o).to(dev), torch.from_numpy(host_d).to(dev)
        row = dict(base, kind="random", rays=n)
        row["cast_ms"] = round(time_gpu(lambda: cast(o, d), args.repeats, args.warmup), 4)
        row["cast_as_given_ms"] = round(time_gpu(lambda: as_given(o, d), max(3, args.repeats // 3), 1), 4)
        row["order_ms"] = round(time_gpu(lambda: meshquery.ray_order(o, d, tv), args.repeats, args.warmup), 4)
        face_idx, t, _ = cast(o, d)
        row["hit_fraction"] = round(float((face_idx >= 0).float().mean()), 4)
        near = torch.nan_to_num(o + t[:, None] * d, posinf=0.0) + 2.0 * edge * torch.randn((n, 3), device=dev)
        row["closest_ms"] = round(time_gpu(lambda: meshquery.closest_triangles(near, tv, tf, plan=plan, return_points=True), args.repeats,
                                           args.warmup), 4)
        if args.check:
            got = [x[:args.check].cpu().numpy() for x in cast(o, d)]
            want = meshquery.first_hits_host(host_o[:args.check], host_d[:args.check], verts, faces, pruned=True, chunk_elems=1 << 24)
            row["checked"] = args.check
            row["check_equal"] = bool(np.array_equal(got[0], want[0]) and all(np.array_equal(a.view(np.uint32), b.view(np.uint32))
                                                                             for a, b in zip(got[1:], want[1:])))
        print(json.dumps(row), flush=True)

        # the votes of object extraction
        vh, vw = args.view_size
        Kv = torch.tensor([[0.8 * vw, 0, vw / 2], [0, 0.8 * vw, vh / 2], [0, 0, 1]], device=dev)
        gen = torch.Generator(device=dev).manual_seed(F)
        blob = torch.rand((args.views, vh // 8 + 1, vw // 8 + 1), device=dev, generator=gen) < 0.5
        masks = [m.repeat_interleave(8, 0).repeat_interleave(8, 1)[:vh, :vw] for m in blob]
        c2ws = [look_around(k, dev) for k in range(args.views)]
        scene = meshquery.Scene(tv, tf, device=dev)
        votes_ms = time_host(lambda: extract.triangle_votes(scene, masks, c2ws, Kv, vh, vw), max(1, args.repeats // 3), 1)
        counter, naive = extract.triangle_votes(scene, masks, c2ws, Kv, vh, vw)
        row = dict(base, kind="votes", views=args.views, view_size=[vh, vw], masked_pixels=int(sum(int(m.sum()) for m in masks)),
                   votes_ms=round(votes_ms, 3), per_view_ms=round(votes_ms / max(1, args.views), 4), faces_voted=int((naive > 0).sum()),
                   faces_confirmed=int((counter > 0).sum()))
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
