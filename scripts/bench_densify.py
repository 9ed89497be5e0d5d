"""The densification of the training loops on one GPU: ``autovfx_amd.densify`` against the reference-shaped torch path.

* ``add_densification_stats`` at 1 M and 3 M Gaussians with 20 % visible: torch's two boolean-mask lines against one
  ``gsr_densify_stats`` launch; host wall time per call with a synchronisation at the end of each region (the torch path waits for
  the host inside every call), alternated, median of ``--regions``.
* ``densify_and_prune`` at 1 M and 3 M, SH degree 3, one Adam step taken (moments present), a few per cent cloned and split: the
  reference's four rewrites (tests/densify_cases.py restates them) against plan + one apply launch, each on a fresh copy of the same
  model, alternated, with and without the final ``empty_cache()`` in the timed region.
* the apply kernel alone (device events): bytes read + written over its time, as a fraction of ``--hbm-gbs``.

One JSON object on stdout.  Usage: ``python scripts/bench_densify.py [--regions 5] [--sizes 1000000,3000000]``.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch   # noqa: E402

THR, MIN_OP, EXTENT = 0.0002, 0.005, 5.0


def wall_ms(fn, iters=1):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sizes", default="1000000,3000000")
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_densify.py needs a GPU")
    import densify_cases as C
    from autovfx_amd import densify as D
    dev = "cuda"
    out = {"bench": "densify", "device": torch.cuda.get_device_name(0), "regions": args.regions, "stats": [], "densify_and_prune": []}
    for n in map(int, args.sizes.split(",")):
        # --- stats ---
        g = torch.Generator().manual_seed(n)
        m = C.Model(C.random_tensors(4, 0, 0, dev))
        m.xyz_gradient_accum, m.denom = torch.zeros(n, 1, device=dev), torch.zeros(n, 1, device=dev)
        vp = torch.zeros(n, 3, device=dev, requires_grad=True)
        vp.grad = (torch.randn(n, 3, generator=g) * 3e-4).to(dev)
        f = (torch.rand(n, generator=g) < 0.2).to(dev)
        runs = {"torch": lambda: m.reference_add_densification_stats(vp, f), "hip": lambda: D.add_densification_stats(m, vp, f)}
        times = {k: [] for k in runs}
        for k in runs:
            wall_ms(runs[k], 3)
        for _ in range(args.regions):
            for k in runs:
                times[k].append(wall_ms(runs[k], args.iters))
        row = {"n": n, "visible": 0.2, **{k + "_ms": round(statistics.median(v), 4) for k, v in times.items()}}
        row["speedup"] = round(row["torch_ms"] / row["hip_ms"], 2)
        out["stats"].append(row)
        # --- densify_and_prune ---
        base = C.Model(C.random_tensors(n, 3, 7, dev))
        C.train_steps(base, 1)
        C.fill_stats(base, zero_share=0.4)
        with torch.no_grad():
            base.xyz_gradient_accum *= 0.18          # a few per cent over the threshold
        real_empty_cache = torch.cuda.empty_cache
        row = {"n": n}
        for with_cache in (True, False):
            times = {"torch": [], "hip": []}
            for r in range(args.regions + 1):        # the first region warms both paths up
                for k in times:
                    mm = C.twin(base)
                    torch.manual_seed(1)
                    fn = (lambda: mm.reference_densify_and_prune(THR, MIN_OP, EXTENT, 20)) if k == "torch" else \
                         (lambda: D.densify_and_prune(mm, THR, MIN_OP, EXTENT, 20))
                    if not with_cache:
                        torch.cuda.empty_cache = lambda: None
                    try:
                        t = wall_ms(fn)
                    finally:
                        torch.cuda.empty_cache = real_empty_cache
                    if r:
                        times[k].append(t)
                    row["rows_out"] = mm._xyz.shape[0]
                    del mm
            tag = "with_empty_cache" if with_cache else "without_empty_cache"
            row[tag] = {k + "_ms": round(statistics.median(v), 3) for k, v in times.items()}
            row[tag]["speedup"] = round(row[tag]["torch_ms"] / row[tag]["hip_ms"], 2)
        # --- the apply kernel alone ---
        plan = D.plan_host(base.xyz_gradient_accum, base.denom, base._scaling.detach(), base._opacity.detach(), THR, 0.01 * EXTENT, MIN_OP, 0.1 * EXTENT)
        row["kept"], row["clones"], row["split"] = plan["counts"].tolist()[:3]
        mm = C.twin(base)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        import autovfx_amd._lib as _lib
        real_apply, spans = _lib.lib.gsr_densify_apply, []

        real_lib = _lib.lib

        def timed_apply(*a):
            ev[0].record()
            rc = real_apply(*a)
            ev[1].record()
            return rc

        class LibProxy:
            def __getattr__(self, name):
                return timed_apply if name == "gsr_densify_apply" else getattr(real_lib, name)

        _lib.lib = LibProxy()
        try:
            for _ in range(args.regions):
                mm = C.twin(base)
                torch.manual_seed(1)
                D.densify_and_prune(mm, THR, MIN_OP, EXTENT, 20)
                torch.cuda.synchronize()
                spans.append(ev[0].elapsed_time(ev[1]))
                n_out = mm._xyz.shape[0]
                del mm
        finally:
            _lib.lib = real_lib
        floats = 59 * 3                               # degree 3: 59 floats per Gaussian, parameter + two moments
        moved = n_out * floats * 4 + (row["kept"] * floats + (n_out - row["kept"]) * 59) * 4 + n_out * 4
        ms = statistics.median(spans)
        row["apply"] = {"ms": round(ms, 4), "bytes": moved, "gb_per_s": round(moved / ms / 1e6, 1), "hbm_fraction": round(moved / ms / 1e6 / args.hbm_gbs, 3)}
        out["densify_and_prune"].append(row)
        del base
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
