"""Run by tests/test_reach_lines_gpu.py::test_unfused_build_equals_the_reference_kernels_on_the_reach_scenes in a process of its
own with GSR_LIB = autovfx_amd/lib/libgsr_hip_unfused.so (as tests/blend_terms_unfused_check.py is run).  Renders the scenes of
tests/reach_lines_scenes.py with that build -- a full call and an inference call cut into two slabs -- and with the reference's own
kernels compiled for gfx950 without contraction (oracle/_ref/libgsr_ref_hip.so) and demands the SAME BITS in colour, depth, alpha
and radii.  Prints one JSON line per scene."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from autovfx_amd import _lib                                           # noqa: E402
from oracle import ref_hip                                             # noqa: E402

import reach_lines_scenes as rls                                       # noqa: E402
from helpers import hip_forward_inference, hip_forward_raw             # noqa: E402


def main():
    assert _lib.LIB_PATH.endswith("libgsr_hip_unfused.so"), _lib.LIB_PATH
    from diff_gaussian_rasterization import _C
    _C.set_alloc_poison("random")
    dev = torch.device("cuda", 0)
    bad = 0
    for size in rls.SIZES:
        cloud, cam, _ = rls.scene(*size)
        n_ref, c_ref, d_ref, a_ref, r_ref = ref_hip.forward(cloud.to(dev), cam.to(dev), torch.tensor(rls.BG, device=dev))
        torch.cuda.synchronize()
        want = {"color": c_ref, "depth": d_ref, "alpha": a_ref, "radii": r_ref}
        row = {"case": f"reach{size[0]}x{size[1]}", "num_rendered": int(n_ref), "pixels": int(a_ref.numel())}
        calls = (("full", hip_forward_raw(cloud, cam, cull=True, bg=rls.BG)),
                 ("inference", hip_forward_inference(cloud, cam, bg=rls.BG, slabs=2, slab_first=8)))
        for call, got in calls:
            for key, ref in want.items():
                diff = int((torch.from_numpy(got[key]).view(torch.int32) != ref.cpu().view(torch.int32).reshape(got[key].shape)).sum())
                row[f"{call}_{key}_words_differ"] = diff
                bad += diff
        print(json.dumps(row), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
