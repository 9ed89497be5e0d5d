"""The pair expansion with its records staged through LDS (expand_kernel): a workgroup fetches the offsets AND the records of a
chunk of items cooperatively and walks them from LDS.  What can go wrong is which items are staged (a record read past the
staged range), the chunk loop (a workgroup whose pairs span several chunks; a lane whose pairs straddle two), the compacted
item list of a later slab, and the digit histogram that reuses the records' LDS.

  * full calls, culling off: ``point_list``, tile keys, ``ranges`` and ``n_contrib`` are the CPU oracle's;
  * inference calls cut into depth slabs (culling on): every image is the full call's, bit for bit;
  * every call runs on poisoned allocations (``_C.set_alloc_poison``), so an unstaged record shows as a wrong list, not a fault.
"""
import math

import numpy as np
import pytest
import torch

from autovfx_amd import scenes
from autovfx_amd.scenes import GaussianCloud
from oracle import cpu_oracle

from helpers import hip_forward_inference, hip_forward_raw, oracle_kwargs

pytestmark = pytest.mark.gpu
BG = (0.2, 0.1, 0.3)
CHUNK = 768        # items staged at a time (gsr_binning.hip: expand_kernel kChunk)
WORKGROUP = 2048   # pairs of one workgroup


@pytest.fixture(autouse=True)
def _poison():
    from diff_gaussian_rasterization import _C
    _C.set_alloc_poison("random")
    yield
    _C.set_alloc_poison(None)


def cloud_of(means, scales, opac, seed=0):
    P = len(means)
    g = torch.Generator().manual_seed(seed)
    t = lambda a: torch.as_tensor(np.asarray(a, np.float32)).contiguous()
    q = torch.randn(P, 4, generator=g)
    shs = torch.cat((torch.randn(P, 1, 3, generator=g), 0.2 * torch.randn(P, 15, 3, generator=g)), 1).contiguous()
    return GaussianCloud(t(means), t(opac).reshape(P, 1), t(scales), (q / q.norm(dim=1, keepdim=True)).contiguous(), shs, None, 3)


def view_xy(cam, px, py, vz):
    """World x, y (the C1 camera has an identity rotation) of the point that lands on pixel (px, py) at view depth vz."""
    W, H = cam.image_width, cam.image_height
    return ((2.0 * px + 1.0) / W - 1.0) * cam.tanfovx * vz, ((2.0 * py + 1.0) / H - 1.0) * cam.tanfovy * vz


def one_pair_splats(cam, n, g, vz_lo, vz_hi):
    """n splats of a two-pixel radius at the centres of random tiles: one pair each, in random depth order."""
    gx, gy = (cam.image_width + 15) // 16, (cam.image_height + 15) // 16
    tx, ty = g.integers(0, gx - (cam.image_width % 16 != 0), n), g.integers(0, gy - (cam.image_height % 16 != 0), n)
    vz = g.uniform(vz_lo, vz_hi, n)
    x, y = view_xy(cam, tx * 16 + 8.0, ty * 16 + 8.0, vz)
    means = np.stack((x, y, vz - 4.0), 1).astype(np.float32)   # the camera sits at z = -4 looking down +z
    return means, np.full((n, 3), 0.0004, np.float32) * vz[:, None].astype(np.float32)


def full_call_equals_oracle(name, cloud, cam):
    ref = cpu_oracle.forward(intermediates=True, **oracle_kwargs(cloud, cam, bg=BG))
    hip = hip_forward_raw(cloud, cam, cull=False, bg=BG)
    np.testing.assert_array_equal(hip["point_list"], ref["point_list"], err_msg=f"{name}: point_list")
    np.testing.assert_array_equal(hip["tile_keys"], (ref["point_list_keys"] >> np.uint64(32)).astype(np.uint32), err_msg=f"{name}: tile keys")
    np.testing.assert_array_equal(hip["ranges"], ref["ranges"], err_msg=f"{name}: ranges")
    print(f"{name}: n_contrib differs from the oracle's on {int((hip['n_contrib'] != ref['n_contrib']).sum())} pixels")
    np.testing.assert_array_equal(hip["n_contrib"], ref["n_contrib"], err_msg=f"{name}: n_contrib")
    return hip, ref


def inference_equals_full(name, cloud, cam, **opts):
    full = hip_forward_raw(cloud, cam, cull=True, bg=BG)
    inf = hip_forward_inference(cloud, cam, bg=BG, **opts)
    for k in ("color", "depth", "alpha"):
        np.testing.assert_array_equal(inf[k].view(np.uint32), full[k].view(np.uint32), err_msg=f"{name}: {k} of the inference call")
    np.testing.assert_array_equal(inf["radii"], full["radii"], err_msg=f"{name}: radii")
    assert inf["num_rendered"] == full["num_rendered"]
    print(f"{name}: slab pairs {inf['slab_pairs']}, full call {full['live_pairs']} pairs")
    return full, inf


@pytest.mark.parametrize("n", [CHUNK - 1, CHUNK, CHUNK + 1, WORKGROUP - 1, WORKGROUP, WORKGROUP + 1, WORKGROUP + CHUNK + 1])
def test_pair_counts_at_chunk_and_workgroup_boundaries(n):
    """n one-pair splats: n items and n pairs, so the last chunk of the last workgroup holds one item less than, exactly, and one
    more than a full chunk / a full workgroup."""
    cam = scenes.c1_camera(64, 64)
    g = np.random.default_rng(n)
    means, scales = one_pair_splats(cam, n, g, 3.0, 6.0)
    cloud = cloud_of(means, scales, np.full((n, 1), 0.04, np.float32), seed=n)
    hip, ref = full_call_equals_oracle(f"boundary{n}", cloud, cam)
    assert hip["live_pairs"] == n == ref["num_rendered"], "the construction is meant to give one pair per splat"
    _, inf = inference_equals_full(f"boundary{n}", cloud, cam, slabs=2, slab_first=20)
    assert len(inf["slab_pairs"]) == 2 and inf["slab_pairs"][1] > 0, "the second slab's compacted list is meant to be walked"
    assert sum(inf["slab_pairs"]) == n


def test_many_one_pair_splats_behind_large_ones():
    """5 000 one-pair splats behind a few large ones: a workgroup's 2 048 pairs span more items than one chunk holds, and the
    large splats' pairs share workgroups with them."""
    cam = scenes.c1_camera(128, 64)
    g = np.random.default_rng(11)
    means, scales = one_pair_splats(cam, 5000, g, 4.0, 7.0)
    front = np.array([(0.0, 0.0, -1.5), (0.3, -0.1, -1.4), (-0.4, 0.1, -1.3), (0.1, 0.2, -1.2)], np.float32)
    means = np.concatenate((front, means))
    scales = np.concatenate((np.full((4, 3), 0.25, np.float32), scales))
    opac = np.concatenate((np.full((4, 1), 0.3, np.float32), np.full((5000, 1), 0.05, np.float32)))
    cloud = cloud_of(means, scales, opac, seed=1)
    hip, _ = full_call_equals_oracle("one-pair", cloud, cam)
    assert hip["live_pairs"] > 5000 + 4 * 20
    for slabs, first in ((2, 12), (3, 6)):
        _, inf = inference_equals_full(f"one-pair {slabs} slabs", cloud, cam, slabs=slabs, slab_first=first)
        assert len(inf["slab_pairs"]) == slabs


def test_one_splat_over_the_whole_image_then_small_ones():
    """One item that spans several workgroups: an oblique ellipse whose reference rectangle is all 3 072 tiles; with culling on
    its rows are runs of different lengths, entered through the binary search over the rows' counts.  Small splats follow."""
    cam = scenes.c1_camera(1024, 768)
    g = np.random.default_rng(12)
    P = 1500
    means = np.concatenate((g.uniform(-2.0, 2.0, (P, 2)), g.uniform(-0.5, 0.5, (P, 1))), 1).astype(np.float32)
    scales = np.exp(g.normal(math.log(0.01), 0.3, (P, 3))).astype(np.float32)
    means[0] = (0.0, 0.0, -2.0)
    scales[0] = (0.56, 0.27, 0.05)    # sigma of 248 x 120 pixels at view depth 2 ...
    opac = g.uniform(0.05, 0.5, (P, 1)).astype(np.float32)
    opac[0] = 0.4
    cloud = cloud_of(means, scales, opac, seed=2)
    cloud.rotations[0] = torch.tensor([math.cos(math.radians(15.0)), 0.0, 0.0, math.sin(math.radians(15.0))])   # ... turned by 30 degrees in the image
    hip, ref = full_call_equals_oracle("whole image", cloud, cam)
    assert ref["tiles_touched"][0] == 64 * 48
    full, inf = inference_equals_full("whole image", cloud, cam, slabs=2, slab_first=1)
    assert full["tight_rect"][0, 2] * full["tight_rect"][0, 3] > WORKGROUP and WORKGROUP < full["tiles_touched"][0] < ref["tiles_touched"][0]
    np.testing.assert_array_equal(full["color"].view(np.uint32), hip["color"].view(np.uint32), err_msg="whole image: tile culling changed the image")


def wall_scene(cam, wall_scale, wall_opacity, behind, seed):
    """A few large opaque splats in front of `behind` small ones."""
    g = np.random.default_rng(seed)
    means, scales = one_pair_splats(cam, behind, g, 4.0, 7.0)
    scales *= 30.0   # a sigma of two or three pixels: one to four pairs each
    wall = np.array([(0.0, 0.0, -2.0 + 0.01 * i) for i in range(10)], np.float32)
    means = np.concatenate((wall, means))
    scales = np.concatenate((np.full((10, 3), wall_scale, np.float32), scales))
    opac = np.concatenate((np.full((10, 1), wall_opacity, np.float32), np.full((behind, 1), 0.3, np.float32)))
    return cloud_of(means, scales, opac, seed=seed)


def test_later_slab_that_keeps_a_few_per_cent():
    """An opaque wall (ten splats with a sigma of 135 pixels at the image centre: T < 1e-4 within about 135 pixels of it)
    finishes all but the outermost tile columns in the first slab: the second keeps the pairs of those columns only -- fewer
    pairs per lane (the launch was sized for all of them) and the compacted item list."""
    cam = scenes.c1_camera(256, 128)
    cloud = wall_scene(cam, 1.22, 0.995, 6000, seed=21)
    full, inf = inference_equals_full("few per cent", cloud, cam, slabs=2, slab_first=12)
    assert len(inf["slab_pairs"]) == 2
    kept = inf["slab_pairs"][1] / max(1, full["live_pairs"])
    assert 0.0 < kept < 0.10, f"the second slab keeps {kept:.1%} of the call's pairs"
    # its launch is sized for the pairs the slab could have held, no fewer than the call's pairs behind the first slab: a lane's
    # share halves to four pairs once that many workgroups of 1 024 pairs cover what is left (gsr_internal.h: expand_pairs_per_lane)
    grid = -(-(full["live_pairs"] - inf["slab_pairs"][0]) // WORKGROUP)
    assert grid * (WORKGROUP // 2) >= inf["slab_pairs"][1], "the second slab was meant to be expanded with four pairs per lane"
    _, inf3 = inference_equals_full("few per cent, three slabs", cloud, cam, slabs=3, slab_first=12)
    assert len(inf3["slab_pairs"]) == 3


def test_later_slab_with_nothing_left():
    """The wall covers every pixel: the slab behind it lists nothing."""
    cam = scenes.c1_camera(128, 128)
    cloud = wall_scene(cam, 40.0, 0.995, 3000, seed=22)
    _, inf = inference_equals_full("nothing left", cloud, cam, slabs=2, slab_first=6)
    assert len(inf["slab_pairs"]) == 2 and inf["slab_pairs"][1] == 0
