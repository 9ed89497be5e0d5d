#!/usr/bin/env python
"""The mesh normal consistency loss (autovfx_amd/meshloss.py) timed on the GPU on closed jittered meshes, one JSON line per size, beside
the reference-shaped route on the same GPU: pytorch3d's statements restated in torch -- the hashed-edge ``unique`` with its inverse, the
sort of the ``3F`` incidences, ``bincount``, the ``.cpu()`` of the edge counts, the pair enumeration on the host, the copy of the pair
table back, three cross products, ``cosine_similarity`` and the weights.  pytorch3d itself is not a dependency of this repository.  The
host pair enumeration is vectorised in numpy where pytorch3d walks the counts serially on one core, which flatters the reference.

Per size (``--faces``; the faces in random order unless ``--ordered``):

* ``plan_ms``: ``gsr_normal_consistency_plan`` into preallocated outputs and scratch; ``forward_ms``: ``gsr_normal_consistency_forward``
  with the plan given; ``backward_ms``: ``gsr_normal_consistency_backward`` (it includes zeroing ``grad_verts``); ``forward_backward_ms``:
  the two queued one after the other.  These four use the rotation below.
* ``drop_in_ms`` / ``drop_in_backward_ms``: the whole call ``drop_in(original)(meshes)`` as ``autovfx_amd.install()`` places it -- the plan
  built per call, the outputs and the scratch allocated -- and that call plus ``loss.backward()``; ``plan_share`` = ``plan_ms`` over
  ``plan_ms + forward_ms + backward_ms``, the part of a training step's call that a cached plan would save.
* ``reference_ms`` / ``reference_backward_ms``: the reference-shaped route, forward and forward plus ``backward()``.  Both routes' whole
  calls are timed with the host clock around a device synchronise, ``--calls`` calls per window, since the reference's call blocks
  on the host; the median of ``--repeats`` windows.
* ``syncs_per_call`` / ``reference_syncs_per_call``: the synchronising calls torch reports for one whole call
  (``torch.cuda.set_sync_debug_mode``).
* ``peak_bytes`` / ``reference_peak_bytes``: the most memory one whole call with its backward holds beyond its inputs.
* ``forward_bytes`` = what the forward must move at least: 8 per incidence of the plan, 24 per face, 12 per vertex, each face row and
  vertex counted once; ``share_of_hbm_rate`` = ``forward_bytes`` at ``--hbm-tbps`` over ``forward_ms``; ``atomic_gbps`` = 48 bytes
  added per pair over ``backward_ms`` (scripts/bench_meshattrs.py reports the same figure for the face normals' backward).

Timing of the four kernel figures: every call works on one of ``sets`` copies of its buffers, taken in turn, enough copies that they hold
more than twice the 256 MiB Infinity Cache together, so that no call finds its data on the chip; ``batch`` calls sit between two device
events, enough for a window of ``--window-ms``; the median of ``--repeats`` windows after a warm-up round over every copy.

Usage: ``python scripts/bench_meshloss.py [--faces 200000 1000000 2000000] [--ordered] [--repeats 10] [--window-ms 5] [--calls 5]``.
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, ROOT)
from autovfx_amd import _lib, meshloss                          # noqa: E402
from bench_meshattrs import copies_for, time_rotating, torus    # noqa: E402


class Meshes:
    """What the drop-in asks of pytorch3d's ``Meshes``."""

    def __init__(self, verts, faces):
        self._verts, self._faces = verts, faces

    def __len__(self):
        return 1

    def verts_packed(self):
        return self._verts

    def faces_packed(self):
        return self._faces


def host_pairs(edge_num: np.ndarray) -> np.ndarray:
    """``find_verts`` vectorised: for every edge with c incidences from offset o, the pairs (o + i, o + j), i < j, in edge order."""
    offsets = np.cumsum(edge_num) - edge_num
    parts, keys = [], []
    for c in np.unique(edge_num):
        if c < 2:
            continue
        i, j = np.triu_indices(int(c), 1)
        o = offsets[edge_num == c]
        parts.append(np.stack((o[:, None] + i[None, :], o[:, None] + j[None, :]), -1).reshape(-1, 2))
        keys.append(np.repeat(o, len(i)))
    if not parts:
        return np.zeros((0, 2), np.int64)
    pairs, keys = np.concatenate(parts), np.concatenate(keys)
    return pairs if len(parts) == 1 else pairs[np.argsort(keys, kind="stable")]


def reference_route(meshes):
    """pytorch3d's ``mesh_normal_consistency`` for one mesh, statement by statement (``Meshes.edges_packed()``,
    ``faces_packed_to_edges_packed()`` and the loss)."""
    verts, faces = meshes.verts_packed(), meshes.faces_packed()
    V, F = verts.shape[0], faces.shape[0]
    v0, v1, v2 = faces.unbind(1)
    edges = torch.cat((torch.stack((v1, v2), 1), torch.stack((v2, v0), 1), torch.stack((v0, v1), 1)), 0)
    edges, _ = edges.sort(dim=1)
    unique, inverse = torch.unique(V * edges[:, 0] + edges[:, 1], return_inverse=True)
    edges_packed = torch.stack((unique // V, unique % V), 1)
    edge_idx = inverse.reshape(3, F).t().reshape(-1)
    vert_idx = faces.view(-1, 1, 3).expand(-1, 3, -1).reshape(-1, 3)
    edge_idx, edge_sort_idx = edge_idx.sort()
    vert_idx = vert_idx[edge_sort_idx]
    edge_num = edge_idx.bincount(minlength=edges_packed.shape[0])
    pairs = torch.from_numpy(host_pairs(edge_num.cpu().numpy())).to(verts.device)
    if pairs.shape[0] == 0:
        return torch.zeros((1,), dtype=torch.float32, device=verts.device, requires_grad=True)
    v0_idx, v1_idx = edges_packed.unbind(1)
    a, b = verts[v0_idx[edge_idx]], verts[v1_idx[edge_idx]]
    n = (torch.cross(b - a, verts[vert_idx[:, 0]] - a, dim=1) + torch.cross(b - a, verts[vert_idx[:, 1]] - a, dim=1)
         + torch.cross(b - a, verts[vert_idx[:, 2]] - a, dim=1))
    loss = 1 - torch.cosine_similarity(n[pairs[:, 0]], -n[pairs[:, 1]], dim=1)
    weights = torch.full((pairs.shape[0],), 1.0 / pairs.shape[0], dtype=torch.float32, device=verts.device)
    return (loss * weights).sum()


def time_whole(call, calls, repeats):
    """ms per call by the host clock: ``calls`` calls, then a device synchronise; the median of ``repeats`` windows after one warm-up."""
    call()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(calls):
            call()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3 / calls)
    return statistics.median(times)


def syncs_of(call):
    """The synchronising calls torch reports for one ``call``; None where the debug mode is not available."""
    try:
        torch.cuda.set_sync_debug_mode("warn")
    except Exception:
        return None
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            call()
        return sum(1 for w in seen if "synchroniz" in str(w.message).lower())
    finally:
        torch.cuda.set_sync_debug_mode("default")


def peak_of(call):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    call()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - before)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, nargs="+", default=[200_000, 1_000_000, 2_000_000])
    ap.add_argument("--ordered", action="store_true", help="keep the faces in grid order instead of a random one")
    ap.add_argument("--hbm-tbps", type=float, default=6.29)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--window-ms", type=float, default=5.0)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--no-reference", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    name = torch.cuda.get_device_name(0)
    ptrs = lambda *tensors: tuple(t.data_ptr() for t in tensors)
    drop_in = meshloss.drop_in(reference_route)

    for n_faces in args.faces:
        verts, faces = torus(n_faces, not args.ordered, dev)
        V, F = int(verts.shape[0]), int(faces.shape[0])
        n = 3 * F
        plan_bytes = int(_lib.lib.gsr_normal_consistency_plan_scratch_bytes(F))
        part_bytes = int(_lib.lib.gsr_normal_consistency_scratch_bytes(F))
        forward_bytes = 8 * n + 24 * F + 12 * V
        n_sets = copies_for(forward_bytes)
        grad_loss = torch.full((1,), 0.5, device=dev)
        u8 = lambda count: torch.empty(count, dtype=torch.uint8, device=dev)
        sets = [dict(verts=verts.clone(), faces=faces.clone(), order=torch.empty(n, dtype=torch.int32, device=dev),
                     partners=torch.empty(n, dtype=torch.int32, device=dev), pairs=torch.empty(1, dtype=torch.int64, device=dev),
                     plan_scratch=u8(plan_bytes), partials=u8(part_bytes), loss=torch.empty(1, device=dev),
                     grad_verts=torch.empty((V, 3), device=dev)) for _ in range(n_sets)]

        def plan(i):
            s = sets[i]
            _lib.call("gsr_normal_consistency_plan", V, F, *ptrs(s["faces"], s["order"], s["partners"], s["pairs"], s["plan_scratch"]), plan_bytes,
                      device=dev)

        def forward(i):
            s = sets[i]
            _lib.call("gsr_normal_consistency_forward", V, F, *ptrs(s["verts"], s["faces"], s["order"], s["partners"], s["pairs"], s["loss"]), None,
                      s["partials"].data_ptr(), part_bytes, device=dev)

        def backward(i):
            s = sets[i]
            _lib.call("gsr_normal_consistency_backward", V, F, *ptrs(s["verts"], s["faces"], s["order"], s["partners"], s["pairs"]),
                      grad_loss.data_ptr(), s["grad_verts"].data_ptr(), device=dev)

        def both(i):
            forward(i), backward(i)

        row = {"faces": F, "verts": V, "shuffled": not args.ordered, "sets": n_sets, "device": name}
        for key, call in (("plan_ms", plan), ("forward_ms", forward), ("backward_ms", backward), ("forward_backward_ms", both)):
            ms, batch = time_rotating(call, n_sets, args.repeats, args.window_ms)
            row[key], row[key.replace("_ms", "_batch")] = round(ms, 4), batch
        P = int(sets[0]["pairs"].item())
        row["pairs"] = P
        row["plan_share"] = round(row["plan_ms"] / (row["plan_ms"] + row["forward_ms"] + row["backward_ms"]), 3)
        row["forward_bytes"] = forward_bytes
        row["share_of_hbm_rate"] = round(forward_bytes / (args.hbm_tbps * 1e9) / row["forward_ms"], 3)
        row["atomic_gbps"] = round(48 * P / row["backward_ms"] / 1e6, 1)
        row["plan_scratch_bytes"] = plan_bytes

        leaf = verts.clone().requires_grad_(True)
        meshes = Meshes(leaf, faces)

        def with_backward(route):
            def call():
                leaf.grad = None
                route(meshes).backward()
            return call

        with torch.no_grad():
            row["drop_in_ms"] = round(time_whole(lambda: drop_in(meshes), args.calls, args.repeats), 4)
        row["drop_in_backward_ms"] = round(time_whole(with_backward(drop_in), args.calls, args.repeats), 4)
        row["syncs_per_call"] = syncs_of(with_backward(drop_in))
        row["peak_bytes"] = peak_of(with_backward(drop_in))
        ours_loss, ours_grad = float(drop_in(meshes).item()), None
        with_backward(drop_in)()
        ours_grad = leaf.grad.clone()
        if not args.no_reference:
            with torch.no_grad():
                row["reference_ms"] = round(time_whole(lambda: reference_route(meshes), args.calls, args.repeats), 4)
            row["reference_backward_ms"] = round(time_whole(with_backward(reference_route), args.calls, args.repeats), 4)
            row["reference_syncs_per_call"] = syncs_of(with_backward(reference_route))
            row["reference_peak_bytes"] = peak_of(with_backward(reference_route))
            with_backward(reference_route)()
            row["loss"], row["reference_loss"] = ours_loss, float(reference_route(meshes).item())
            row["max_abs_grad_diff"] = float((ours_grad - leaf.grad).abs().max())
            assert abs(row["loss"] - row["reference_loss"]) <= 1e-5 * max(1.0, abs(row["reference_loss"]))
            assert row["max_abs_grad_diff"] <= 1e-3 * float(leaf.grad.abs().max())
        print(json.dumps(row), flush=True)
        del sets, verts, faces, leaf, meshes, ours_grad


if __name__ == "__main__":
    main()
