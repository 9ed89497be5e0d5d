"""The quadrant blend with the per-column and per-row terms of `power` staged per entry (gsr_blend.hip): while a wave stages a batch
of 64 list entries, the lane of an entry that reaches the quadrant takes the LDS slot of its rank among the reaching ones and
writes the entry's eight column pairs, eight row pairs and uniform words there; the walk visits the slots in order.  A batch with
more reaching entries than slots (32; 30 with a second feature set) is walked in rounds.  What can go wrong: the rank (a slot
written twice or not at all), the round loop (entries dropped or walked twice at the slot count; the next batch prefetched over a
round still to be built), the entry's index for the last-contributor count, a quadrant that stops in the middle of a round and
resumes in a later slab, lanes outside the image.

  * full calls, culling off: ``point_list``, ``ranges`` and ``n_contrib`` are the CPU oracle's, images within the contract of
    tests/test_parity_gpu.py (1e-4; these scenes get no allowance for threshold flips beyond its parts per million);
  * inference calls cut into depth slabs: every image, the radii and ``num_rendered`` are the full call's, bit for bit;
  * every call runs on poisoned allocations (``_C.set_alloc_poison``).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import cpu_oracle

import blend_terms_scenes as bts
from blend_terms_scenes import BG
from helpers import hip_forward_inference, hip_forward_raw, oracle_kwargs, settings_for
from test_expand_staging_gpu import full_call_equals_oracle, inference_equals_full
from test_parity_gpu import assert_images

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _poison():
    from diff_gaussian_rasterization import _C
    _C.set_alloc_poison("random")
    yield
    _C.set_alloc_poison(None)


def both_call_forms(name, cloud, cam, slab_opts=({}, {"slabs": 2, "slab_first": 8})):
    hip, ref = full_call_equals_oracle(name, cloud, cam)
    assert_images(name, hip, ref)
    out = []
    for opts in slab_opts:
        full, inf = inference_equals_full(f"{name} {opts}", cloud, cam, **opts)
        np.testing.assert_array_equal(full["color"].view(np.uint32), hip["color"].view(np.uint32), err_msg=f"{name}: tile culling changed the image")
        out.append(inf)
    return hip, ref, out


def extra_equals_second_pass(name, cloud, cam, slab_first):
    """The fused call with a second feature triple against the plain call and a second pass with colors_precomp = that triple, bit
    for bit; then the same as an inference call cut into slabs.  (tests/test_parity_gpu.py does this at size.)"""
    from autovfx_amd import _lib
    from diff_gaussian_rasterization import _C
    dev = "cuda:0"
    c = cloud.to(dev)
    st = settings_for(cam, dev, BG, 1.0, cloud.sh_degree)
    e = torch.Tensor([])
    extra = torch.rand((cloud.P, 3), generator=torch.Generator(device=dev).manual_seed(3), device=dev)
    args = lambda colors, sh: (st.bg, c.means3D, colors, c.opacities, c.scales, c.rotations, 1.0, e, st.viewmatrix, st.projmatrix,
                               st.tanfovx, st.tanfovy, st.image_height, st.image_width, sh, st.sh_degree, st.campos, False, False)
    _C.set_geometry_cache(False)
    _lib.set_option(_lib.OPT_SLAB_MIN_REST, 0)
    try:
        fused = _C.rasterize_gaussians_extra(*args(e, c.shs), extra)
        plain = _C.rasterize_gaussians(*args(e, c.shs))
        second = _C.rasterize_gaussians(*args(extra, e))
        _lib.set_option(_lib.OPT_SLABS, 0); _lib.set_option(_lib.OPT_SLAB_FIRST, slab_first)
        slabbed = _C.rasterize_gaussians_extra(*args(e, c.shs), extra, inference=True)
        torch.cuda.synchronize()
        n_slabs = len(_C.last_layout()["slab_pairs"])
    finally:
        _C.set_geometry_cache(None)
        _lib.set_option(_lib.OPT_SLABS, 2); _lib.set_option(_lib.OPT_SLAB_FIRST, 400); _lib.set_option(_lib.OPT_SLAB_MIN_REST, 3_000_000)
    same = lambda a, b: torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    assert fused[0] == plain[0] == slabbed[0], name
    for i in (1, 2, 3, 4):
        assert same(fused[i], plain[i]), (name, i)
    assert same(fused[8], second[1]), f"{name}: the second feature set's image is not the second pass's"
    for i in (1, 2, 3, 4, 8):
        assert same(slabbed[i], fused[i]), (name, i, n_slabs)
    return n_slabs


@pytest.mark.parametrize("k", bts.BOUNDARY_COUNTS)
def test_reaching_entries_at_slot_and_batch_boundaries(k):
    """k faint splats centred inside one quadrant: that quadrant stages all k, in one round less one slot, exactly one round, one
    round and one entry, ..., two batches and one entry; nothing saturates, so every pixel of it counts k contributors at most and
    its last contributor is the list's."""
    cloud, cam = bts.boundary_scene(k)
    hip, ref, _ = both_call_forms(f"boundary{k}", cloud, cam)
    tile = 1   # tile (1, 0) of the 2 x 2 grid
    assert ref["ranges"][tile][1] - ref["ranges"][tile][0] == k, "every splat is meant to be in the tile's list"
    assert hip["n_contrib"].reshape(32, 32)[8:16, 24:32].max() == k, "the quadrant's list is meant to be walked to its end"
    extra_equals_second_pass(f"boundary{k} second set", cloud, cam, slab_first=20)


@pytest.mark.parametrize("size", [(37, 29), (24, 16)])
def test_ranks_that_differ_per_quadrant_and_lanes_outside_the_image(size):
    cloud, cam = bts.seam_scene(*size, seed=7 if size[0] == 37 else 8)
    both_call_forms(f"seams{size}", cloud, cam)
    extra_equals_second_pass(f"seams{size} second set", cloud, cam, slab_first=8)


@pytest.mark.parametrize("slabs", [2, 3])
def test_saturation_inside_a_round_then_resumption_in_a_later_slab(slabs):
    cloud, cam = bts.saturation_scene()
    hip, ref, (inf,) = both_call_forms("saturation", cloud, cam, slab_opts=({"slabs": slabs, "slab_first": 8},))
    assert len(inf["slab_pairs"]) == slabs and all(p > 0 for p in inf["slab_pairs"][1:]), f"the later slabs' lists are meant to be walked: {inf['slab_pairs']}"
    nc = hip["n_contrib"].reshape(32, 48)
    assert nc[:16, :16].max() < 40, "tile (0, 0) is meant to stop inside the opaque stack"
    assert nc[:, 32:].max() > 0 and hip["alpha"][0, :, 32:].max() < 0.9999, "the pixels beside the stack are meant to stay live"
    n_slabs = extra_equals_second_pass("saturation second set", cloud, cam, slab_first=8)
    assert n_slabs > 1


@pytest.mark.parametrize("value", [float("nan"), float("inf")])
def test_non_finite_scale_gives_the_same_bits_in_both_call_forms(value):
    """One Gaussian with a non-finite scale among finite ones: the call returns, and the full and the inference call agree in
    every bit, NaN bits included (the comparison is on the words)."""
    cloud, cam = bts.seam_scene(24, 16, seed=9)
    cloud.scales[5, 0] = value
    for opts in ({}, {"slabs": 2, "slab_first": 8}):
        inference_equals_full(f"scale {value} {opts}", cloud, cam, **opts)


def test_unfused_build_equals_the_reference_kernels_on_the_slot_scenes():
    """The finite scenes above through the unfused test build (lib/libgsr_hip_unfused.so) against the reference's kernels compiled
    for gfx950 without contraction, bit for bit, in a process of its own (a process holds one build of the library).  The scene
    with a non-finite scale is left out: the reference converts a NaN radius to an integer, which leaves its rectangle undefined."""
    from oracle import ref_hip
    lib = os.path.join(ROOT, "autovfx_amd", "lib", "libgsr_hip_unfused.so")
    if not ref_hip.available():
        pytest.skip("oracle/_ref/libgsr_ref_hip.so not built")
    assert os.path.exists(lib), "lib/libgsr_hip_unfused.so is not built: run __graft_entry__.build()"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "blend_terms_unfused_check.py")], env=dict(os.environ, GSR_LIB=lib),
                       capture_output=True, text=True, timeout=300)
    rows = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    print(rows)
    assert r.returncode == 0 and len(rows) == len(bts.BOUNDARY_COUNTS) + 3, (r.stdout[-2000:], r.stderr[-2000:])
    assert all(row[k] == 0 for row in rows for k in row if k.endswith("_words_differ")), rows
