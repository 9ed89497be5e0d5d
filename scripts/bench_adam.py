#!/usr/bin/env python
"""The training loops' optimizer step timed on the GPU, three ways in the same run, one JSON line.

* per workload (C2: 1 M Gaussians, C3: 3 M; SH degree 3, the six groups of ``GaussianModel.training_setup``): ``torch.optim.Adam``
  as the reference builds it (foreach), ``torch.optim.Adam(fused=True)`` and ``autovfx_amd.optim.Adam`` (one ``gsr_adam_step``
  launch), each on its own copy of the parameters, timed in alternation: the median of ``--regions`` rounds, each round one
  device-event region of ``--iters`` steps per variant after ``--warmup`` untimed ones.  ``gbps`` is the per-step floor of the
  fused update (read p, g, m, v; write p, m, v: 28 bytes per element) over the step time;
* ``c3_train_iteration``: one reference iteration at C3 -- ``render()`` with grad, ``0.8 L1 + 0.2 (1 - ssim)`` (fused SSIM),
  ``backward()``, ``step()``, ``zero_grad(set_to_none=True)`` -- with torch's Adam and with this one, regions alternated.

Kernel times come from a separate run under ``rocprofv3 --kernel-trace --stats`` (``--skip-train`` keeps that run short).
Usage: ``python scripts/bench_adam.py [--regions 7] [--iters 20] [--warmup 5] [--steps 10] [--skip-train]``.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from autovfx_amd import optim as O   # noqa: E402

FLOATS = {"xyz": 3, "f_dc": 3, "f_rest": 45, "opacity": 1, "scaling": 3, "rotation": 4}   # 59 per Gaussian at SH degree 3
LRS = {"xyz": 1.6e-4, "f_dc": 2.5e-3, "f_rest": 2.5e-3 / 20.0, "opacity": 0.05, "scaling": 5e-3, "rotation": 1e-3}
WORKLOADS = (("c2", 1_000_000), ("c3", 3_000_000))
BYTES_PER_ELEMENT = 7 * 4


def groups(n, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    out = []
    for k, f in FLOATS.items():
        p = torch.nn.Parameter(torch.randn((n, f), generator=g, device=dev))
        p.grad = torch.randn((n, f), generator=g, device=dev) * 1e-3
        out.append({"params": [p], "lr": LRS[k], "name": k})
    return out


def event_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def step_rows(dev, args):
    rows = {}
    for name, n in WORKLOADS:
        variants = {"torch_foreach": lambda gs: torch.optim.Adam(gs, lr=0.0, eps=1e-15),
                    "torch_fused": lambda gs: torch.optim.Adam(gs, lr=0.0, eps=1e-15, fused=True),
                    "gsr_adam": lambda gs: O.Adam(gs, lr=0.0, eps=1e-15)}
        opts = {k: make(groups(n, dev, 0)) for k, make in variants.items()}
        assert O.kernel_takes(opts["gsr_adam"].param_groups, opts["gsr_adam"].state)
        for opt in opts.values():
            for _ in range(args.warmup):
                opt.step()
        torch.cuda.synchronize()
        times = {k: [] for k in opts}
        for _ in range(args.regions):
            for k, opt in opts.items():          # alternating, one region each per round
                times[k].append(event_ms(opt.step, args.iters))
        elements = n * sum(FLOATS.values())
        row = {"gaussians": n, "elements": elements, "floor_gb": round(elements * BYTES_PER_ELEMENT / 1e9, 3)}
        for k, ts in times.items():
            ms = statistics.median(ts)
            row[f"{k}_ms"] = round(ms, 4)
            row[f"{k}_spread_ms"] = [round(min(ts), 4), round(max(ts), 4)]
            row[f"{k}_gbps"] = round(elements * BYTES_PER_ELEMENT / (ms * 1e-3) / 1e9, 1)
        row["speedup_vs_foreach"] = round(row["torch_foreach_ms"] / row["gsr_adam_ms"], 2)
        row["speedup_vs_fused"] = round(row["torch_fused_ms"] / row["gsr_adam_ms"], 2)
        rows[name] = row
        del opts
        torch.cuda.empty_cache()
    return rows


def c3_iteration(dev, args):
    import bench
    from autovfx_amd import renderer
    from autovfx_amd.ssim import ssim
    b = bench.Bench("c3", dev, None, boundary="op")
    params = ("_xyz", "_scaling", "_rotation", "_opacity", "_features_dc", "_features_rest")
    names = {"_xyz": "xyz", "_scaling": "scaling", "_rotation": "rotation", "_opacity": "opacity", "_features_dc": "f_dc",
             "_features_rest": "f_rest"}
    target = torch.rand(4, b.H, b.W, device=dev)
    frames = [(10 + 7 * j) % b.F for j in range(args.steps)]
    for f in frames:
        b.cam(f)

    def setup(cls):
        m = bench.ReferenceGetters(b.cloud, b.cloud.sh_degree)
        for k in params:
            setattr(m, k, getattr(m, k).detach().clone().requires_grad_(True))
        opt = cls([{"params": [getattr(m, k)], "lr": LRS[names[k]], "name": names[k]} for k in params], lr=0.0, eps=1e-15)

        def run():
            for f in frames:
                img = renderer.render(b.cam(f), m, renderer.PipelineParams, b.bg)["render"]
                loss = 0.8 * (img - target).abs().mean() + 0.2 * (1.0 - ssim(img, target))
                loss.backward()
                opt.step()
                opt.zero_grad(set_to_none=True)
        for _ in range(2):
            run()
        return run

    runs = {"torch_adam": setup(torch.optim.Adam), "gsr_adam": setup(O.Adam)}
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(args.regions):          # alternating, one region each per round
        for k, run in runs.items():
            times[k].append(event_ms(run, 1) / len(frames))

    out = {"workload": b.name, "W": b.W, "H": b.H, "steps": len(frames),
           "iteration": "render() + 0.8 L1 + 0.2 (1 - ssim) + backward + step + zero_grad(set_to_none=True)"}
    for k, ts in times.items():
        out[f"{k}_ms_per_iter"] = round(statistics.median(ts), 3)
        out[f"{k}_spread_ms"] = [round(min(ts), 3), round(max(ts), 3)]
    out["saved_ms_per_iter"] = round(out["torch_adam_ms_per_iter"] - out["gsr_adam_ms_per_iter"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--skip-train", action="store_true", help="the optimizer steps only (no renderer iteration)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_adam.py needs a GPU")
    dev = torch.device("cuda", 0)
    out = {"bench": "adam", "device": torch.cuda.get_device_name(0), "steps": step_rows(dev, args)}
    if not args.skip_train:
        out["c3_train_iteration"] = c3_iteration(dev, args)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
