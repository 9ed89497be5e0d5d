"""Builds libgsr_hip.so (the C-ABI rasterizer, include/gsr.h) for gfx950 with hipcc.

hipcc cross-compiles without a GPU, so this runs in the build container; the resulting .so is
git-ignored but travels to the GPU box with the repo snapshot.  Usage: ``python -m autovfx_amd.build``.
"""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT_DIR = os.path.join(HERE, "lib")
LIB = os.path.join(OUT_DIR, "libgsr_hip.so")
SOURCES = ["gsr_kernels.hip", "gsr_binning.hip", "gsr_blend.hip", "gsr_backward.hip", "gsr_radix.hip", "gsr_frameio.hip", "gsr_resample.hip", "gsr_layerio.hip", "gsr_layerfiles.hip", "gsr_panorama.hip", "gsr_tree.hip", "gsr_knn.hip", "gsr_meshquery.hip", "gsr_ssim.hip", "gsr_adam.hip", "gsr_densify.hip", "gsr_field.hip", "gsr_meshraster.hip", "gsr_meshattrs.hip", "gsr_meshloss.hip", "gsr_texture.hip", "gsr_bound.hip", "gsr_api.hip"]
HEADERS = [os.path.join(CSRC, "gsr_internal.h"), os.path.join(CSRC, "gsr_device.h"), os.path.join(CSRC, "gsr_inflate_core.h"),
           os.path.join(CSRC, "gsr_tree.h"), os.path.join(CSRC, "gsr_wave.h"), os.path.join(CSRC, "gsr_vec3.h"), os.path.join(HERE, "..", "include", "gsr.h")]
# -ffp-contract=off: the parity contract is fp32 in the reference's operation order;
# no -ffast-math: IEEE divide / sqrt, accurate expf.
# -fno-slp-vectorize: on gfx950 packed fp32 multiply / add issue at half rate (only the packed fma is full rate), so
# the SLP vectorizer's pairing of scalar fp32 work buys no issue slots and costs register shuffles.  Same-box A/B on
# MI355X: the backward kernels, long stretches of scalar fp32 algebra, are 10 % faster without it (VGPRs 117 -> 91 in
# preprocess_backward); the forward path is 0.5 % faster without it in the 3-stream regime, where vector issue is the
# contended resource, and 1.3 % slower single-stream, where it is memory-bound and the vectorizer's wider accesses
# help.  The one profitable pairing, the blend's compositing fma, is written with vector types.  Same IEEE results.
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize", "-Wall",
         "-Wno-unused-result", "-fvisibility=hidden", "-DNDEBUG"]
FILE_FLAGS = {}   # per-file additions, if a unit ever needs its own


EXAMPLES_DIR = os.path.join(HERE, "..", "examples")
EXAMPLES = ("render_raw", "render_stream", "train_step_raw")


def build_examples(force: bool = False, verbose: bool = False):
    """examples/*.cpp: the C ABI driven from plain C++ / HIP (no Python, no torch); linked against the in-tree library
    with a relative rpath so the binaries travel with the repository.  Returns their paths."""
    lib = build()
    out = []
    for name in EXAMPLES:
        src, exe = os.path.join(EXAMPLES_DIR, name + ".cpp"), os.path.join(EXAMPLES_DIR, "bin", name)
        if force or _stale(exe, [src, lib] + HEADERS):
            os.makedirs(os.path.dirname(exe), exist_ok=True)
            cmd = [hipcc(), "--offload-arch=gfx950", "-O2", "-std=c++17", src, "-o", exe, "-L", OUT_DIR, "-lgsr_hip",
                   "-Wl,-rpath,$ORIGIN/../../autovfx_amd/lib"]
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.check_call(cmd)
        out.append(exe)
    return out


def hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


def _stale(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = False, trace: bool = False, unfused: bool = False) -> str:
    """``trace=True`` builds libgsr_hip_trace.so: the same library with per-workgroup phase timestamps compiled
    into selected kernels (GSR_KERNEL_TRACE; see scripts/kernel_trace.py).  A profiling aid, never the default.
    ``unfused=True`` builds libgsr_hip_unfused.so: the blend's one fused multiply-add written as the reference's sources say it
    (GSR_UNFUSED_BLEND, gsr_blend.hip) -- a TEST build whose images must equal the reference kernels' bit for bit."""
    os.makedirs(OUT_DIR, exist_ok=True)
    cc = hipcc()
    objs, jobs = [], []
    tag = "_trace" if trace else "_unfused" if unfused else ""
    lib = LIB.replace(".so", tag + ".so")
    flags = FLAGS + (["-DGSR_KERNEL_TRACE=1"] if trace else []) + (["-DGSR_UNFUSED_BLEND=1"] if unfused else [])
    for src in SOURCES:
        sp = os.path.join(CSRC, src)
        # (only the blend differs in the unfused build: the other units' objects are shared with the product's)
        obj = os.path.join(OUT_DIR, src.replace(".hip", (tag if trace or src == "gsr_blend.hip" else "") + ".o"))
        objs.append(obj)
        if force or _stale(obj, [sp] + HEADERS + [__file__]):
            jobs.append([cc, "-x", "hip", *flags, *FILE_FLAGS.get(src, []), "-c", sp, "-o", obj])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)

    if jobs:
        with ThreadPoolExecutor(max_workers=len(jobs)) as ex:
            list(ex.map(run, jobs))
    if jobs or force or _stale(lib, objs):
        run([cc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib, *objs,
             "-Wl,--exclude-libs,ALL", "-lz"])      # zlib: gsr_layerfiles.hip (inflate, crc32 for the compositor's input files)
    return lib


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True, trace="--trace" in sys.argv, unfused="--unfused" in sys.argv))
