#!/usr/bin/env python
"""Wall time of one panorama (render_panorama.py:100-145) on the GPU, two ways, printed as one JSON line.

* ``dropin``: ``autovfx_amd.panorama.render_panorama`` -- the six faces in flight, the cube-to-equirect kernel, seven PNG file images
  built on the GPU, one device-to-host copy, files written by host threads -- and its parts timed on their own: ``faces``
  (render_cube_faces), ``resample`` (gsr_cube_to_equirect, LDR bytes), ``files`` (the faces' and the panorama's PNGs on the GPU, the
  copy and the writes);
* ``reference_shaped``: what the reference does, on the same GPU with this repository's render(): six blocking render() calls, each
  face quantised as save_image does, copied to the host and saved through PIL, ``c2e_host`` (the numpy restatement of ``c2e``) and
  the panorama saved through PIL.

Configuration: C2 (scenes.config_c2, 1M Gaussians), the camera centre at the origin, 1024^2 faces, a 1024 x 2048 panorama, files to
tmpfs (/dev/shm when it exists).  Every number is the median of ``--repeats`` host-clock timings, each ending in a device
synchronise, after ``--warmup`` untimed runs.  Usage: ``python scripts/bench_panorama.py [--repeats 5] [--warmup 2]``.
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from autovfx_amd import gaussian_model as gm        # noqa: E402
from autovfx_amd import panorama as pano             # noqa: E402
from autovfx_amd import renderer, scenes             # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--face", type=int, default=1024)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=2048)
    args = ap.parse_args()
    from PIL import Image

    dev = torch.device("cuda", 0)
    c = scenes.config_c2()
    model = gm.GaussianModel.from_activated(c.means3D, c.opacities, c.scales, c.rotations, c.shs, 3).to(dev)
    bg = torch.tensor([0.0, 0.0, 0.0], device=dev)
    pipe, center, S, H, W = renderer.PipelineParams, np.zeros(3), args.face, args.height, args.width
    base = tempfile.mkdtemp(prefix="bench_panorama_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    clock = time.perf_counter

    def sync_timed(fn):
        torch.cuda.synchronize()
        t0 = clock()
        out = fn()
        torch.cuda.synchronize()
        return clock() - t0, out

    def dropin_parts(k):
        t_faces, faces = sync_timed(lambda: pano.render_cube_faces(model, pipe, bg, center, S))
        planar = [faces[n]["render"] for n in pano.FACE_ORDER]
        t_resample, _ = sync_timed(lambda: pano.cube_to_equirect(planar, H, W, out_uint8=True))
        t_total, _ = sync_timed(lambda: pano.render_panorama(model, pipe, bg, center, os.path.join(base, f"d{k}"), H, W, face_size=S))
        return {"faces": t_faces, "resample": t_resample, "total": t_total}

    def reference_shaped(k):
        out_dir = os.path.join(base, f"r{k}")
        os.makedirs(out_dir, exist_ok=True)
        cams = pano.cube_map_cameras(center, S)
        t = {"renders_and_copies": 0.0, "face_saves": 0.0}
        torch.cuda.synchronize()
        t0 = clock()
        faces = {}
        with torch.no_grad():
            for name in pano.VIEW_ORDER:
                a = clock()
                img = renderer.render(cams[name].to(dev), model, pipe, bg)["render"]
                arr = img.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8).numpy()   # save_image's bytes
                faces[name] = img.permute(1, 2, 0).cpu().numpy()
                b = clock()
                Image.fromarray(arr).save(os.path.join(out_dir, name + ".png"))
                t["renders_and_copies"] += b - a
                t["face_saves"] += clock() - b
        a = clock()
        eq = pano.c2e_host(faces, H, W)
        t["c2e_host"] = clock() - a
        a = clock()
        Image.fromarray(np.clip(eq * 255, 0, 255).astype(np.uint8)).save(os.path.join(out_dir, "pano_ldr.png"))
        t["pano_save"] = clock() - a
        t["total"] = clock() - t0
        return t

    try:
        for k in range(args.warmup):
            dropin_parts(-1 - k)
            reference_shaped(-1 - k)
        runs_d, runs_r = [], []
        for k in range(args.repeats):       # alternated, so that both see the same state of the shared host
            runs_d.append(dropin_parts(k))
            runs_r.append(reference_shaped(k))
        med = lambda runs: {key: round(1e3 * statistics.median(r[key] for r in runs), 3) for key in runs[0]}
        d, r = med(runs_d), med(runs_r)
        d["files"] = round(d["total"] - d["faces"] - d["resample"], 3)   # the rest of the drop-in's call: PNG kernels, copy, writes
        sizes = {n: os.path.getsize(os.path.join(base, "d0", n + ".png")) for n in list(pano.VIEW_ORDER) + ["pano_ldr"]}
        print(json.dumps({"bench": "panorama", "config": {"scene": "C2", "gaussians": c.P, "center": [0, 0, 0], "face": S, "pano": [H, W],
                                                          "files_to": os.path.dirname(base), "repeats": args.repeats, "warmup": args.warmup},
                          "dropin_ms": d, "reference_shaped_ms": r, "speedup_total": round(r["total"] / d["total"], 1),
                          "dropin_file_bytes": sizes,
                          "device": torch.cuda.get_device_name(dev)}), flush=True)
    finally:
        shutil.rmtree(base, ignore_errors=True)


if __name__ == "__main__":
    main()
