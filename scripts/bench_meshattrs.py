#!/usr/bin/env python
"""Face areas / normals and face-attribute interpolation (autovfx_amd/meshattrs.py) timed on the GPU at the sizes of SuGaR's refinement and
texture extraction, one JSON line per configuration.  The comparator is the same expressions in torch on the same GPU -- indexing,
``torch.cross``, broadcast products and sums, ``index_add_`` -- because pytorch3d's operators are CUDA kernels and do not run on the MI355X
(DESIGN.md 7j).  The sums over the corners and channels are a product and ``sum`` where the issue behind this script named ``einsum``:
``einsum`` runs them as a batched matrix product with one batch per slot, and torch's batched product is not usable at 2e7 batches or
more on this GPU (K = 10).  The comparator is not run (``null``) where one of its intermediates would hold 2^31 elements or more.

* ``"op": "faces"``: a closed mesh of ``--faces`` triangles, every vertex in six faces (a torus cut into quads, each quad into two
  triangles; ``--shuffle`` puts the faces in random order).  ``forward_ms`` / ``backward_ms``: ``gsr_face_areas_normals`` /
  ``gsr_face_areas_normals_backward`` into preallocated outputs (the backward includes zeroing ``grad_verts``); ``torch_*_ms``: the torch
  expressions.  ``forward_bytes`` = what the call must move at least: 24 of indices and 16 written per face and 12 per vertex, each vertex
  counted once (its six faces find it in L2); ``gathered_bytes`` counts 36 of vertices per face instead; ``share_of_hbm_rate`` =
  ``forward_bytes`` at ``--hbm-tbps`` over ``forward_ms``; ``atomic_gbps`` = 36 bytes added per face over ``backward_ms``.
* ``"op": "interp"``: the fragments ``autovfx_amd.meshraster`` returns for ``--faces`` / 2 flat diamonds (scripts/bench_meshraster.py's
  scene) at ``--height`` x ``--width`` and each ``--K``, random attributes ``[F, 3, D]`` for each ``--D``.  ``forward_bytes`` = per slot 8
  of index, 12 of barycentrics and 4 D written, and 12 D of attributes per face that can be under a slot (``min(filled, F)``: each
  face's rows counted once); ``gathered_bytes`` counts 12 D per filled slot instead; ``atomic_gbps`` = 12 D bytes added per filled
  slot over ``backward_ms`` (which also holds the ``grad_bary`` kernel and the zeroing of ``grad_attrs``).
Timing: every call works on one of ``sets`` copies of its inputs and outputs, taken in turn, enough copies that they hold more than twice
the 256 MiB Infinity Cache together (one copy where a single one already does), so that no call finds its data on the chip; ``batch``
calls sit between two device events, enough for a window of ``--window-ms``, and the time is the window's over ``batch``; the median of
``--repeats`` windows after a warm-up round over every copy.

Usage: ``python scripts/bench_meshattrs.py [--faces 1000000 2000000] [--K 1 10] [--D 2 3 48] [--repeats 10] [--window-ms 5]``.
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
from autovfx_amd import _lib                                    # noqa: E402
from autovfx_amd.meshraster import rasterize_face_verts         # noqa: E402
from bench_meshraster import scene                              # noqa: E402


def torus(n_faces, shuffle, dev):
    """``verts [V, 3]``, ``faces [F, 3]``: ``F = 2 V``, every vertex in six faces."""
    nv = max(3, int(math.sqrt(n_faces / 4)))
    nu = max(3, n_faces // (2 * nv))
    g = torch.Generator(device=dev).manual_seed(n_faces)
    jitter = lambda: 0.2 * (2 * torch.rand(nu, nv, generator=g, device=dev) - 1)
    u = (torch.arange(nu, device=dev)[:, None] + jitter()) * (2 * math.pi / nu)
    v = (torch.arange(nv, device=dev)[None, :] + jitter()) * (2 * math.pi / nv)
    ring = 1.0 + 0.4 * torch.cos(v)
    verts = torch.stack((ring * torch.cos(u), ring * torch.sin(u), 0.4 * torch.sin(v)), -1).reshape(-1, 3).contiguous()
    i, j = torch.meshgrid(torch.arange(nu, device=dev), torch.arange(nv, device=dev), indexing="ij")
    at = lambda a, b: ((a % nu) * nv + (b % nv)).reshape(-1)
    faces = torch.stack((torch.stack((at(i, j), at(i + 1, j), at(i + 1, j + 1)), 1), torch.stack((at(i, j), at(i + 1, j + 1), at(i, j + 1)), 1)),
                        1).reshape(-1, 3)
    if shuffle:
        faces = faces[torch.randperm(len(faces), generator=g, device=dev)]
    return verts, faces.contiguous()


def torch_faces_forward(verts, faces):
    v0, v1, v2 = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    c = torch.cross(v1 - v0, v2 - v0, dim=1)
    n = c.norm(dim=1)
    return n / 2, c / n.clamp_min(1e-6)[:, None]


def torch_faces_backward(verts, faces, grad_areas, grad_normals):
    v0, v1, v2 = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    a, b = v1 - v0, v2 - v0
    c = torch.cross(a, b, dim=1)
    n = c.norm(dim=1, keepdim=True).clamp_min(1e-6)
    m = c / n
    gc = grad_areas[:, None] * m / 2 + (grad_normals - m * (m * grad_normals).sum(1, keepdim=True)) / n
    ga, gb = torch.cross(b, gc, dim=1), torch.cross(gc, a, dim=1)
    grad = torch.zeros_like(verts)
    grad.index_add_(0, faces[:, 0], -(ga + gb))
    grad.index_add_(0, faces[:, 1], ga)
    grad.index_add_(0, faces[:, 2], gb)
    return grad


def torch_interp_forward(pix, bary, attrs):
    held = pix >= 0
    return (bary[:, :, None] * attrs[pix.clamp_min(0)]).sum(1) * held[:, None]


def torch_interp_backward(pix, bary, attrs, grad_out):
    held = pix >= 0
    idx = pix.clamp_min(0)
    go = grad_out * held[:, None]
    grad_bary = (go[:, None, :] * attrs[idx]).sum(2)
    grad_attrs = torch.zeros_like(attrs).index_add_(0, idx, bary[:, :, None] * go[:, None, :])
    return grad_bary, grad_attrs


CACHE_BYTES = 256 << 20


def copies_for(nbytes):
    """How many copies of a call's buffers, used in turn, keep every call off the Infinity Cache."""
    return max(1, math.ceil(2 * CACHE_BYTES / nbytes))


def time_rotating(call, n_sets, repeats, window_ms):
    """``(ms per call, batch)``: ``call(i)`` works on buffer set i; see the module docstring."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(n_sets):
        call(i)
    e0.record()
    call(0)
    e1.record()
    e1.synchronize()
    batch = min(2000, max(n_sets, math.ceil(window_ms / max(e0.elapsed_time(e1), 1e-3))))
    times, k = [], 0
    for _ in range(repeats):
        e0.record()
        for _ in range(batch):
            call(k % n_sets)
            k += 1
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / batch)
    return statistics.median(times), batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, nargs="+", default=[1_000_000, 2_000_000])
    ap.add_argument("--K", type=int, nargs="+", default=[1, 10])
    ap.add_argument("--D", type=int, nargs="+", default=[2, 3, 48])
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--size", type=float, default=0.02)
    ap.add_argument("--shuffle", action="store_true")
    ap.add_argument("--ops", nargs="+", default=["faces", "interp"], choices=["faces", "interp"])
    ap.add_argument("--hbm-tbps", type=float, default=6.29)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--window-ms", type=float, default=5.0)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    H, W = args.height, args.width
    name = torch.cuda.get_device_name(0)
    ptrs = lambda *tensors: tuple(t.data_ptr() for t in tensors)

    def timed(row, key, call, n_sets):
        ms, batch = time_rotating(call, n_sets, args.repeats, args.window_ms)
        row[key], row[key.replace("_ms", "_batch")] = round(ms, 4), batch

    with torch.no_grad():
        for n_faces in args.faces if "faces" in args.ops else ():
            verts, faces = torus(n_faces, args.shuffle, dev)
            V, F = int(verts.shape[0]), int(faces.shape[0])
            g = torch.Generator(device=dev).manual_seed(1)
            ga, gn = torch.randn(F, generator=g, device=dev), torch.randn((F, 3), generator=g, device=dev)
            forward_bytes = 40 * F + 12 * V
            n_sets = copies_for(forward_bytes)
            sets = [dict(verts=verts.clone(), faces=faces.clone(), ga=ga.clone(), gn=gn.clone(), areas=torch.empty(F, device=dev),
                         normals=torch.empty((F, 3), device=dev), grad_verts=torch.empty((V, 3), device=dev)) for _ in range(n_sets)]

            def forward(i):
                s = sets[i]
                _lib.call("gsr_face_areas_normals", V, F, *ptrs(s["verts"], s["faces"], s["areas"], s["normals"]), device=dev)

            def backward(i):
                s = sets[i]
                _lib.call("gsr_face_areas_normals_backward", V, F, *ptrs(s["verts"], s["faces"], s["ga"], s["gn"], s["grad_verts"]), device=dev)

            row = {"op": "faces", "faces": F, "verts": V, "shuffled": args.shuffle, "sets": n_sets, "device": name}
            timed(row, "forward_ms", forward, n_sets)
            timed(row, "torch_forward_ms", lambda i: torch_faces_forward(sets[i]["verts"], sets[i]["faces"]), n_sets)
            timed(row, "backward_ms", backward, n_sets)
            timed(row, "torch_backward_ms", lambda i: torch_faces_backward(sets[i]["verts"], sets[i]["faces"], sets[i]["ga"], sets[i]["gn"]), n_sets)
            row["forward_bytes"], row["gathered_bytes"] = forward_bytes, 76 * F
            row["share_of_hbm_rate"] = round(forward_bytes / (args.hbm_tbps * 1e9) / row["forward_ms"], 3)
            row["atomic_gbps"] = round(36 * F / row["backward_ms"] / 1e6, 1)
            want = torch_faces_backward(verts, faces, ga, gn)
            row["max_abs_diff_to_torch"] = float((sets[0]["grad_verts"] - want).abs().max())
            assert math.isfinite(row["backward_ms"]) and row["max_abs_diff_to_torch"] <= 1e-3 * float(want.abs().max())
            print(json.dumps(row), flush=True)
            del verts, faces, ga, gn, want, sets

        for n_faces in args.faces if "interp" in args.ops else ():
            fv, first, num, nbr = scene(n_faces // 2, H, W, args.size, dev)
            F = int(fv.shape[0])
            for K in args.K:
                pix4, _, bary5, _ = rasterize_face_verts(fv, first, num, nbr, (H, W), 0.0, K, None, 50_000, True, False, False)
                pix, bary = pix4.reshape(-1), bary5.reshape(-1, 3)
                P, filled = int(pix.numel()), int((pix >= 0).sum())
                for D in args.D:
                    g = torch.Generator(device=dev).manual_seed(D)
                    attrs, grad_out = torch.rand((F, 3, D), generator=g, device=dev), torch.randn((P, D), generator=g, device=dev)
                    forward_bytes = P * (20 + 4 * D) + min(filled, F) * 12 * D
                    n_sets = copies_for(forward_bytes)
                    sets = [dict(pix=pix.clone(), bary=bary.clone(), attrs=attrs.clone(), grad_out=grad_out.clone(), out=torch.empty((P, D), device=dev),
                                 grad_bary=torch.empty((P, 3), device=dev), grad_attrs=torch.empty((F, 3, D), device=dev)) for _ in range(n_sets)]

                    def forward(i):
                        s = sets[i]
                        _lib.call("gsr_interp_face_attrs", P, F, D, *ptrs(s["pix"], s["bary"], s["attrs"], s["out"]), device=dev)

                    def backward(i):
                        s = sets[i]
                        _lib.call("gsr_interp_face_attrs_backward", P, F, D,
                                  *ptrs(s["pix"], s["bary"], s["attrs"], s["grad_out"], s["grad_bary"], s["grad_attrs"]), device=dev)

                    row = {"op": "interp", "faces": F, "H": H, "W": W, "K": K, "D": D, "slots": P, "filled": filled, "sets": n_sets, "device": name}
                    timed(row, "forward_ms", forward, n_sets)
                    timed(row, "backward_ms", backward, n_sets)
                    compared = P * 3 * D < 1 << 31                       # the comparator's largest intermediate, [P, 3, D]
                    row["torch_forward_ms"] = row["torch_backward_ms"] = None
                    if compared:
                        timed(row, "torch_forward_ms", lambda i: torch_interp_forward(sets[i]["pix"], sets[i]["bary"], sets[i]["attrs"]), n_sets)
                        timed(row, "torch_backward_ms",
                              lambda i: torch_interp_backward(sets[i]["pix"], sets[i]["bary"], sets[i]["attrs"], sets[i]["grad_out"]), n_sets)
                    row["forward_bytes"], row["gathered_bytes"] = forward_bytes, P * (20 + 4 * D) + filled * 12 * D
                    row["share_of_hbm_rate"] = round(forward_bytes / (args.hbm_tbps * 1e9) / row["forward_ms"], 3)
                    row["atomic_gbps"] = round(12 * D * filled / row["backward_ms"] / 1e6, 1)
                    assert math.isfinite(row["backward_ms"])
                    if compared:
                        want = torch_interp_backward(pix, bary, attrs, grad_out)[1]
                        row["max_abs_diff_to_torch"] = float((sets[0]["grad_attrs"] - want).abs().max())
                        assert row["max_abs_diff_to_torch"] <= 1e-3 * max(1.0, float(want.abs().max()))
                        del want
                    print(json.dumps(row), flush=True)
                    del attrs, grad_out, sets
                del pix4, bary5, pix, bary


if __name__ == "__main__":
    main()
