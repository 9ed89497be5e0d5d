#!/usr/bin/env python
"""The Gaussians bound to a surface mesh (autovfx_amd/bound.py: ``SuGaR.points``, ``scaling`` and ``quaternions``) timed on the GPU at the two
settings of SuGaR's refinement, one JSON line per configuration: ``--config F:G`` = faces : Gaussians per face, by default 400 000 : 6 (200 k
vertices, six per face) and 2 000 000 : 1 (1 M vertices).  The mesh is scripts/bench_meshattrs.py's torus (``F = 2 V``, every vertex in six
faces).  The comparator is the chain of torch operations in the reference's shape on the same GPU (``tests/bound_cases.StubSuGaR``, with
pytorch3d 0.7.4's ``matrix_to_quaternion`` restated); where it raises (out of memory, an index past 2^31) its figures are ``null`` and the
reason is recorded, nothing is extrapolated.

Per configuration:

* ``forward_ms``: ``gsr_bound_gaussians`` into preallocated outputs, ``all`` three and each one alone; ``forward_bytes``: what the call must
  move at least -- 24 of indices per face, 12 per vertex (each counted once: its six faces find it in L2), 16 read and 12 + 12 + 16 written per
  Gaussian -- and ``share_of_hbm_rate`` = those bytes at ``--hbm-tbps`` over the time (``gathered_bytes`` counts 36 of vertices per face);
* ``backward_ms``: ``gsr_bound_gaussians_backward`` with all three upstream gradients into preallocated outputs (zeroing ``grad_verts``
  included); ``atomic_gbps`` = 36 bytes added per face over it;
* ``node_*_ms`` / ``torch_*_ms``: through autograd, allocations included -- ``forward``: the three getters; ``forward_backward``: the three
  getters, ``(points g_p).sum() + (scaling g_s).sum() + (quaternions g_q).sum()`` and its ``backward()`` into the vertices, ``_quaternions`` and
  ``_scales`` -- for the drop-ins and for the torch chain;
* ``*_peak_mb``: ``torch.cuda.max_memory_allocated`` over one forward plus backward above what was allocated before it;
* ``*_syncs_per_access``: host synchronisations torch reports (``set_sync_debug_mode("warn")``) during one access to ``quaternions``
  (``node_sync_messages``: what it said about the drop-in's, if anything).

Timing as scripts/bench_meshattrs.py: every call works on one of ``sets`` copies of its buffers, taken in turn, enough copies that they hold
more than twice the 256 MiB Infinity Cache together; ``batch`` calls between two device events for a window of ``--window-ms``; the median
of ``--repeats`` windows after a warm-up round over every copy.

Usage: ``python scripts/bench_bound.py [--config 400000:6 2000000:1] [--repeats 10] [--window-ms 5] [--no-torch]``.
"""
import argparse
import json
import math
import os
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")]
import bound_cases as BC                                                   # noqa: E402
from autovfx_amd import _lib, bound                                        # noqa: E402
from bench_meshattrs import copies_for, time_rotating, torus               # noqa: E402

OUTPUTS = ("points", "scaling", "quaternions")


def syncs_during(fn) -> list:
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    said = [str(w.message).splitlines()[0][:160] for w in seen]
    return [m for m in said if "synchroniz" in m.lower() and "prototype feature" not in m]      # (not torch's one-time notice about the mode itself)


def peak_mb(fn) -> float:
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", nargs="+", default=["400000:6", "2000000:1"])
    ap.add_argument("--shuffle", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--hbm-tbps", type=float, default=6.29)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--window-ms", type=float, default=5.0)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    name = torch.cuda.get_device_name(0)
    ptr = lambda t: None if t is None else t.data_ptr()
    getters = {n: getattr(bound, "drop_in_" + n)(vars(BC.StubSuGaR)[n].fget) for n in OUTPUTS}
    originals = {n: vars(BC.StubSuGaR)[n].fget for n in OUTPUTS}

    for config in args.config:
        n_faces, G = (int(x) for x in config.split(":"))
        verts, faces = torus(n_faces, args.shuffle, dev)
        V, F = int(verts.shape[0]), int(faces.shape[0])
        N = F * G
        g = torch.Generator(device=dev).manual_seed(G)
        rand = lambda *shape: torch.randn(shape, generator=g, device=dev)
        bary = torch.from_numpy(BC.bary_of(G)).to(dev)
        base = dict(verts=verts, faces=faces, complex=rand(N, 2), log_scales=-4 + rand(N, 2), g_points=rand(N, 3), g_scaling=rand(N, 3),
                    g_quaternions=rand(N, 4))
        thickness = torch.full((1,), 3.7e-6, device=dev)
        forward_bytes = 24 * F + 12 * V + N * (16 + 40)
        n_sets = copies_for(forward_bytes)
        sets = []
        for _ in range(n_sets):
            s = {k: v.clone() for k, v in base.items()}
            s.update(points=torch.empty((N, 3), device=dev), scaling=torch.empty((N, 3), device=dev), quaternions=torch.empty((N, 4), device=dev),
                     grad_verts=torch.empty((V, 3), device=dev), grad_complex=torch.empty((N, 2), device=dev), grad_log_scales=torch.empty((N, 2), device=dev))
            model = BC.StubSuGaR.__new__(BC.StubSuGaR)
            vars(model).update(device=dev, binded_to_surface_mesh=True, editable=False, scale_activation=torch.exp,
                               _points=s["verts"].requires_grad_(True), _surface_mesh_faces=s["faces"], surface_triangle_bary_coords=bary[..., None],
                               n_gaussians_per_surface_triangle=G, _quaternions=s["complex"].requires_grad_(True),
                               _scales=s["log_scales"].requires_grad_(True), surface_mesh_thickness=thickness.reshape(()), _n_points=N)
            s["model"] = model
            sets.append(s)

        def forward(i, want=OUTPUTS):
            s = sets[i]
            _lib.call("gsr_bound_gaussians", V, F, G, ptr(s["verts"]), ptr(s["faces"]), ptr(bary), ptr(s["complex"]), ptr(s["log_scales"]), ptr(thickness),
                      0, *(ptr(s[n]) if n in want else None for n in OUTPUTS), device=dev)

        def backward(i):
            s = sets[i]
            _lib.call("gsr_bound_gaussians_backward", V, F, G, ptr(s["verts"]), ptr(s["faces"]), ptr(bary), ptr(s["complex"]), ptr(s["log_scales"]), 0,
                      ptr(s["g_points"]), ptr(s["g_scaling"]), ptr(s["g_quaternions"]), ptr(s["grad_verts"]), ptr(s["grad_complex"]),
                      ptr(s["grad_log_scales"]), device=dev)

        def access(which, i, grad):
            s = sets[i]
            m = s["model"]
            outs = [which[n](m) for n in OUTPUTS]
            if grad:
                m._points.grad = m._quaternions.grad = m._scales.grad = None
                sum((o * s["g_" + n]).sum() for o, n in zip(outs, OUTPUTS)).backward()
            return outs

        def timed(row, key, call):
            ms, batch = time_rotating(call, n_sets, args.repeats, args.window_ms)
            row[key], row[key.replace("_ms", "_batch")] = round(ms, 4), batch

        row = {"faces": F, "verts": V, "G": G, "gaussians": N, "shuffled": args.shuffle, "sets": n_sets, "device": name}
        with torch.no_grad():
            timed(row, "forward_ms", forward)
            for n in OUTPUTS:
                timed(row, f"forward_{n}_ms", lambda i, n=n: forward(i, (n,)))
            timed(row, "backward_ms", backward)
        row["forward_bytes"], row["gathered_bytes"] = forward_bytes, forward_bytes + 36 * F - 12 * V
        row["share_of_hbm_rate"] = round(forward_bytes / (args.hbm_tbps * 1e9) / row["forward_ms"], 3)
        row["atomic_gbps"] = round(36 * F / row["backward_ms"] / 1e6, 1)
        with torch.no_grad():
            timed(row, "node_forward_ms", lambda i: access(getters, i, False))
        timed(row, "node_forward_backward_ms", lambda i: access(getters, i, True))
        row["node_peak_mb"] = peak_mb(lambda: access(getters, 0, True))
        said = syncs_during(lambda: getters["quaternions"](sets[0]["model"]))
        row["node_syncs_per_access"], row["node_sync_messages"] = len(said), said
        for key in ("torch_forward_ms", "torch_forward_backward_ms", "torch_peak_mb", "torch_syncs_per_access", "max_abs_diff_to_torch"):
            row[key] = None
        if not args.no_torch:
            try:
                with torch.no_grad():
                    timed(row, "torch_forward_ms", lambda i: access(originals, i, False))
                timed(row, "torch_forward_backward_ms", lambda i: access(originals, i, True))
                row["torch_peak_mb"] = peak_mb(lambda: access(originals, 0, True))
                row["torch_syncs_per_access"] = len(syncs_during(lambda: originals["quaternions"](sets[0]["model"])))
                with torch.no_grad():
                    ours, theirs = access(getters, 0, False), access(originals, 0, False)
                    # (a row whose two largest q_abs tie within rounding may take another candidate: the same rotation, maybe the other sign)
                    diffs = [(a - b).abs().max() for a, b in zip(ours[:2], theirs[:2])]
                    diffs.append(torch.minimum((ours[2] - theirs[2]).abs().amax(1), (ours[2] + theirs[2]).abs().amax(1)).max())
                    row["max_abs_diff_to_torch"] = max(float(d) for d in diffs)
                assert row["max_abs_diff_to_torch"] <= 1e-3
            except (RuntimeError, torch.cuda.OutOfMemoryError) as e:
                row["torch_not_run"] = str(e).splitlines()[0][:200]
        assert math.isfinite(row["backward_ms"])
        print(json.dumps(row), flush=True)
        del sets, base, verts, faces
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
