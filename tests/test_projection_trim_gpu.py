"""The projection kernel after its trim (one definition per result, what crosses its divergent region cut down to seven values,
DPP wave scans): everything it writes, against the CPU oracle bit for bit, on the shapes where the rewritten parts can go wrong.

What is compared, per call (``check``):
  * radii, num_rendered; of the 32-byte raster record the centre, conic, opacity and depth of every Gaussian with a
    radius; ``rgb`` of the same Gaussians on SH calls -- BIT-EXACT against the oracle;
  * ``splat_bins`` with culling off, all four words: the tight rectangle is the reference's rectangle (origin and size, from a
    numpy restatement of getRect on the oracle's centres and radii; its area is the oracle's ``tiles_touched``), a mask is all ones over it, a splat of more than 64 tiles carries all ones in the high word and in the
    low word the tile rows of the large splats before it in its workgroup (the run-pool prefix: the wave scan);
  * the depth keys, through what the depth sort makes of them: the order of the emitting Gaussians is ascending (depth bits, id);
  * with culling on: the same public arrays, rectangles inside the reference's, masks inside the culling-off masks, and (small
    calls) per tile the reference's list minus pairs dead at every pixel -- tests/test_parity_gpu.py's own comparison;
  * raw-parameter calls (activations inside the kernel): against the oracle fed with PyTorch's activations on this device.
Non-finite and extreme inputs are compared with the oracle's per-Gaussian stage (``stage_reference``): the oracle restates the
reference for them, and rows without a radius are not compared (the reference leaves them undefined).
"""
import math

import numpy as np
import pytest
import torch

from autovfx_amd import scenes
from autovfx_amd.cameras import Camera
from autovfx_amd.scenes import GaussianCloud
from oracle import cpu_oracle

from helpers import hip_forward_raw, oracle_kwargs
from test_parity_gpu import assert_culled_lists

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BG = (0.1, 0.2, 0.3)


def origin_camera(width, height, fovx_deg=60.0):
    """A camera at the origin looking down +z: view z IS the mean's z, so denormal and huge depths can be placed exactly."""
    fovx = math.radians(fovx_deg)
    fovy = 2.0 * math.atan(math.tan(fovx / 2.0) * height / width)
    return Camera.from_Rt(np.eye(3), np.zeros(3), fovx, fovy, width, height, "origin")


def cloud_of(means, scales, quats=None, opac=None, seed=0, precomp=False):
    P = len(means)
    g = torch.Generator().manual_seed(seed)
    t = lambda a: torch.as_tensor(np.asarray(a, np.float32)).contiguous()
    if quats is None:
        q = torch.randn(P, 4, generator=g)
        quats = (q / q.norm(dim=1, keepdim=True)).numpy()
    if opac is None:
        opac = torch.sigmoid(torch.randn(P, 1, generator=g) * 1.5).numpy()
    shs = torch.cat((torch.randn(P, 1, 3, generator=g), 0.2 * torch.randn(P, 15, 3, generator=g)), 1).contiguous()
    cols = torch.rand(P, 3, generator=g).contiguous() if precomp else None
    return GaussianCloud(t(means), t(opac).reshape(P, 1), t(scales), t(quats), None if precomp else shs, cols, 3)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def raw_call(cloud, cam, cull):
    """The raw-parameter entry (preprocess_kernel<true>) as a full call, and the activations PyTorch computes on this device."""
    from autovfx_amd import _lib
    from diff_gaussian_rasterization import _C
    from helpers import decode_scratch
    c, camd = cloud.to(DEV), cam.to(DEV)
    ls, rot = torch.log(c.scales), (c.rotations * 1.5).contiguous()
    op = torch.logit(c.opacities.reshape(-1, 1).clamp(1e-6, 1 - 1e-6))
    bg = torch.tensor(BG, device=DEV)
    _lib.set_option(_lib.OPT_TILE_CULL, 1 if cull else 0)
    try:
        with torch.no_grad():
            out = _C.rasterize_gaussians_raw(bg, c.means3D, ls, rot, op, c.shs[:, :1].contiguous(), c.shs[:, 1:].contiguous(), 1.0,
                                             camd.world_view_transform, camd.full_proj_transform, camd.tanfovx, camd.tanfovy,
                                             cam.image_height, cam.image_width, 3, camd.camera_center, False, True, want_normal=False)
        torch.cuda.synchronize()
        lay = _C.last_layout()
    finally:
        _lib.set_option(_lib.OPT_TILE_CULL, 1)
    got = {"num_rendered": out[0], "color": out[1].cpu().numpy(), "radii": out[4].cpu().numpy()}
    got.update(decode_scratch(lay, out[5], out[6], out[7], cloud.P, cam.image_width, cam.image_height))
    act = GaussianCloud(cloud.means3D, torch.sigmoid(op).cpu(), torch.exp(ls).cpu(), torch.nn.functional.normalize(rot).cpu(), cloud.shs,
                        None, 3)
    return got, act


def check_against_oracle(name, got, ref, sh):
    np.testing.assert_array_equal(got["radii"], ref["radii"], err_msg=f"{name}: radii")
    assert got["num_rendered"] == ref["num_rendered"], f"{name}: num_rendered {got['num_rendered']} vs {ref['num_rendered']}"
    vis = ref["radii"] > 0
    for k in ("means2D", "conic_opacity", "depths") + (("rgb",) if sh else ()):
        np.testing.assert_array_equal(bits(got[k][vis]), bits(ref[k][vis]), err_msg=f"{name}: {k}")
    # depth keys: the emitting Gaussians in ascending (depth bits, id) order
    emits = np.flatnonzero((got["tight_rect"][:, 2] * got["tight_rect"][:, 3]) != 0)
    assert got["sorted_count"] == emits.size
    expect = emits[np.lexsort((emits, bits(got["depths"])[emits]))]
    np.testing.assert_array_equal(got["depth_order"][:emits.size], expect.astype(np.uint32), err_msg=f"{name}: depth order")
    assert (ref["radii"][emits] > 0).all(), f"{name}: a splat without a radius emits"


def check_bins_unculled(name, got, ref, cam):
    """splat_bins with culling off, every word: the reference's rectangle (origin and size), all-ones masks, run-pool prefixes of
    the large splats; zeros for a Gaussian that emits nothing."""
    w, h = got["tight_rect"][:, 2].astype(np.int64), got["tight_rect"][:, 3].astype(np.int64)
    area = w * h
    emits = ref["radii"] > 0
    rect = reference_rect(ref["means2D"], ref["radii"], cam.image_width, cam.image_height)
    np.testing.assert_array_equal(got["tight_rect"][emits].astype(np.int64), rect[emits], err_msg=f"{name}: rectangle (x0, y0, w, h)")
    assert (got["tight_rect"][~emits] == 0).all(), f"{name}: a Gaussian that emits nothing has a rectangle"
    np.testing.assert_array_equal(area[emits], ref["tiles_touched"][emits].astype(np.int64), err_msg=f"{name}: rectangle area")
    assert (area[~emits] == 0).all() and (got["live_mask"][~emits] == 0).all()
    small = emits & (area <= 64) & (area > 0)
    full = np.where(area[small] == 64, np.uint64(0xFFFFFFFFFFFFFFFF), (np.uint64(1) << area[small].astype(np.uint64)) - np.uint64(1))
    np.testing.assert_array_equal(got["live_mask"][small], full, err_msg=f"{name}: mask of a small splat with culling off")
    big = area > 64
    rows = np.where(big, h, 0)
    before = np.zeros_like(rows)
    for b0 in range(0, rows.size, 256):   # exclusive prefix inside each 256-Gaussian workgroup
        blk = rows[b0:b0 + 256]
        before[b0:b0 + 256] = np.cumsum(blk) - blk
    np.testing.assert_array_equal(got["live_mask"][big] >> np.uint64(32), np.full(int(big.sum()), 0xFFFFFFFF, np.uint64), err_msg=f"{name}: large splat, high word")
    np.testing.assert_array_equal(got["live_mask"][big] & np.uint64(0xFFFFFFFF), before[big].astype(np.uint64), err_msg=f"{name}: run-pool prefix")
    np.testing.assert_array_equal(got["tiles_touched"], ref["tiles_touched"], err_msg=f"{name}: pairs per splat")


def check_bins_culled(name, on, off):
    x0, y0, w, h = (on["tight_rect"][:, i].astype(np.int64) for i in range(4))
    X0, Y0, W_, H_ = (off["tight_rect"][:, i].astype(np.int64) for i in range(4))
    e = (w * h) != 0
    assert ((w * h)[~e] == 0).all() and (((W_ * H_) != 0) | ~e).all(), f"{name}: culling made a splat emit"
    assert (x0[e] >= X0[e]).all() and (y0[e] >= Y0[e]).all() and ((x0 + w)[e] <= (X0 + W_)[e]).all() and ((y0 + h)[e] <= (Y0 + H_)[e]).all(), \
        f"{name}: a tight rectangle leaves the reference's"
    small = e & (w * h <= 64)
    assert (on["live_mask"][small] != 0).all(), f"{name}: an emitting splat with an empty mask"
    pop = np.array([bin(int(m)).count("1") for m in on["live_mask"][small]], np.int64)
    assert (pop <= (w * h)[small]).all() and (on["live_mask"][small] >> (w * h)[small].astype(np.uint64).clip(max=63) <= 1).all()
    np.testing.assert_array_equal(on["tiles_touched"][small], pop.astype(np.uint32), err_msg=f"{name}: pairs of a masked splat = popcount(mask)")


def reference_rect(means2D, radii, W, H):
    """getRect (auxiliary.h:46-56) in fp32, as the oracle's tile_rect states it: x0, y0, width, height in tiles, [P, 4]."""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    r = radii.astype(np.float32)

    def f2i(v):   # round toward zero, saturating, NaN -> 0
        return np.where(np.isnan(v), 0.0, np.clip(np.trunc(v.astype(np.float64)), -2.0 ** 31, 2.0 ** 31 - 1)).astype(np.int64)

    with np.errstate(all="ignore"):
        px, py = means2D[:, 0].astype(np.float32), means2D[:, 1].astype(np.float32)
        x0, y0 = np.clip(f2i((px - r) / np.float32(16)), 0, gx), np.clip(f2i((py - r) / np.float32(16)), 0, gy)
        x1 = np.clip(f2i((px + r + np.float32(16) - np.float32(1)) / np.float32(16)), 0, gx)
        y1 = np.clip(f2i((py + r + np.float32(16) - np.float32(1)) / np.float32(16)), 0, gy)
    return np.stack((x0, y0, x1 - x0, y1 - y0), 1)


def reference_rect_area(means2D, radii, W, H):
    r = reference_rect(means2D, radii, W, H)
    return r[:, 2] * r[:, 3]


def stage_reference(act, cam):
    """The oracle's per-Gaussian stage alone, for clouds with non-finite or extreme members.  (The reference never emits the pairs
    of a splat whose covariance is NaN -- radius 0 -- although its scan counts them, so the key slots of those pairs keep what the
    allocation held; the oracle's full forward restates that too and may not be run on such a cloud.)  ``num_rendered`` is the
    sum of the rectangle areas of every Gaussian that reaches the end of the stage: the ones with a depth written."""
    ref = cpu_oracle.preprocess(**oracle_kwargs(act, cam, bg=BG))
    area = reference_rect_area(ref["means2D"], ref["radii"], cam.image_width, cam.image_height)
    done = bits(ref["depths"]) != 0
    assert (area[ref["radii"] > 0] > 0).all()
    ref["tiles_touched"] = np.where(ref["radii"] > 0, area, 0).astype(np.uint32)
    ref["num_rendered"] = int(area[done].sum())
    return ref


def check(name, cloud, cam, raw=False, lists=True, stage_only=False):
    """One scene through the kernel with culling off and on, against the oracle (``stage_only``: stage_reference)."""
    sh = cloud.colors_precomp is None
    if raw:
        off, act = raw_call(cloud, cam, cull=False)
        on, _ = raw_call(cloud, cam, cull=True)
    else:
        off = hip_forward_raw(cloud, cam, cull=False, bg=BG)
        on = hip_forward_raw(cloud, cam, cull=True, bg=BG)
        act = cloud
    ref = stage_reference(act, cam) if stage_only else cpu_oracle.forward(intermediates=True, **oracle_kwargs(act, cam, bg=BG))
    check_against_oracle(name + " cull off", off, ref, sh)
    check_against_oracle(name + " cull on", on, ref, sh)
    check_bins_unculled(name, off, ref, cam)
    check_bins_culled(name, on, off)
    if not stage_only:
        np.testing.assert_array_equal(off["point_list"], ref["point_list"], err_msg=f"{name}: point_list")
        np.testing.assert_array_equal(off["ranges"], ref["ranges"], err_msg=f"{name}: ranges")
    np.testing.assert_array_equal(bits(on["means2D"]), bits(off["means2D"]))
    for k in ("color",):
        np.testing.assert_array_equal(bits(on[k]), bits(off[k]), err_msg=f"{name}: {k} changed by tile culling")
    if lists and not stage_only and ref["num_rendered"] <= 60_000:
        assert_culled_lists(name, on, ref, cam.image_width, cam.image_height)
    return off, on, ref


@pytest.mark.parametrize("P", [1, 63, 64, 65, 255, 257, 1000])
def test_wave_and_workgroup_edges(P):
    """Clouds that end inside a wave, on its edge, inside a workgroup and just past one: activated and raw parameters, SH and
    precomputed colours, culling off and on."""
    cam = scenes.c1_camera(160, 112)
    base = scenes.config_c1(P=P, seed=40 + P)
    check(f"edges{P}", base, cam)
    check(f"edges{P} raw", base, cam, raw=True, lists=False)
    pre = cloud_of(base.means3D.numpy(), base.scales.numpy(), base.rotations.numpy(), base.opacities.numpy(), seed=P, precomp=True)
    check(f"edges{P} precomp", pre, cam, lists=False)


def test_first_waves_entirely_behind_the_camera():
    """Two whole waves and part of a third are culled at the near plane: their lanes carry zeros through the scans."""
    g = np.random.default_rng(3)
    P = 400
    means = g.uniform(-1, 1, (P, 3)).astype(np.float32)
    means[:150, 2] = g.uniform(-9.0, -4.5, 150)   # the camera sits at z = -4 looking down +z
    cloud = cloud_of(means, np.exp(g.normal(math.log(0.05), 0.4, (P, 3))), seed=1)
    off, _, ref = check("behind", cloud, scenes.c1_camera(192, 128))
    assert (ref["radii"][:150] == 0).all() and (ref["radii"][150:] > 0).sum() > 100


def test_mask_candidates_with_more_than_64_rows_in_one_wave():
    """About forty needles of 3 x 3 tiles in the first wave: its (splat, row) items exceed 64, so the flattened mask loop runs twice."""
    g = np.random.default_rng(5)
    P = 192
    means = np.concatenate((g.uniform(-1.2, 1.2, (P, 2)), g.uniform(-0.2, 0.2, (P, 1))), 1).astype(np.float32)
    scales = np.full((P, 3), 0.012, np.float32)
    needles = np.r_[0:40, 70:90]
    scales[needles] = (0.16, 0.025, 0.025)
    opac = np.full((P, 1), 0.6, np.float32)
    cloud = cloud_of(means, scales, opac=opac, seed=2)
    off, on, ref = check("rows>64", cloud, scenes.c1_camera(256, 256))
    w, h = on["tight_rect"][:64, 2].astype(int), on["tight_rect"][:64, 3].astype(int)
    cand = (w >= 2) & (h >= 2) & (w * h <= 64)
    assert h[cand].sum() > 64, f"the first wave has only {h[cand].sum()} candidate rows"
    assert (on["tiles_touched"][needles] < off["tiles_touched"][needles]).sum() > 20, "the needles' corner tiles were meant to be culled"


def test_large_splats_among_small_ones():
    """Splats above the 64-tile mask limit in the workgroups of small ones: their rows are a prefix over the workgroup (the wave
    scan and the cross-wave sum), in every wave and on both sides of a workgroup boundary."""
    g = np.random.default_rng(7)
    P = 600
    means = np.concatenate((g.uniform(-1.0, 1.0, (P, 2)), g.uniform(-0.3, 0.3, (P, 1))), 1).astype(np.float32)
    scales = np.exp(g.normal(math.log(0.02), 0.3, (P, 3))).astype(np.float32)
    large = np.array([0, 5, 63, 64, 100, 130, 200, 255, 256, 300, 511, 512, 599])
    scales[large] = g.uniform(0.5, 0.9, (large.size, 3))
    cloud = cloud_of(means, scales, seed=3)
    off, on, _ = check("large", cloud, scenes.c1_camera(256, 192), lists=False)
    for o in (off, on):
        assert ((o["tight_rect"][large, 2].astype(int) * o["tight_rect"][large, 3]) > 64).all()
    # culling keeps the prefixes consistent too
    rows = np.where((on["tight_rect"][:, 2].astype(int) * on["tight_rect"][:, 3]) > 64, on["tight_rect"][:, 3].astype(int), 0)
    for b0 in range(0, P, 256):
        blk = rows[b0:b0 + 256]
        big = np.flatnonzero(blk) + b0
        np.testing.assert_array_equal(on["live_mask"][big] & np.uint64(0xFFFFFFFF), (np.cumsum(blk) - blk)[big - b0].astype(np.uint64))


def test_quotients_at_the_near_plane_and_the_ends_of_the_exponent_range():
    """The quotients by vz and vz * vz (a hand-written form that shares the reciprocal between them was measured and not kept:
    scripts/experiments/shared_denominator_quotients.patch -- this is the test it has to pass): vz on both sides of 0.2 (ulp by
    ulp), denormal, and so large that vz * vz overflows or that 1 / vz is denormal; numerators that are zero, denormal and huge."""
    zs = [np.nextafter(np.float32(0.2), np.float32(k), dtype=np.float32) for k in (0, 1)] + [np.float32(0.2)]
    z = np.float32(0.2)
    for _ in range(4):
        z = np.nextafter(z, np.float32(1), dtype=np.float32)
        zs.append(z)
    zs += [np.float32(v) for v in (1e-40, 1e-38, 0.25, 1.0, 3.0, 1e4, 1e15, 1.5e19, 2e19, 1e30, 8.6e37, 1.8e38, 3.4e38)]
    xs = [np.float32(v) for v in (0.0, 1e-42, 1e-30, 0.01, -0.07, 1e10, -1e30, 3e38)]
    means = np.array([(x * (1 if abs(x) > 1 else zz if zz < 10 else 1), -x * 0.5, zz) for zz in zs for x in xs], np.float32)
    P = len(means)
    scales = np.tile(np.float32([0.02, 0.03, 0.01]), (P, 1)) * np.maximum(1.0, means[:, 2:3] * 0.05).astype(np.float32)
    cloud = cloud_of(means, scales, seed=4)
    off, _, ref = check("quotients", cloud, origin_camera(160, 112), stage_only=True)
    assert (ref["radii"] > 0).sum() >= 20 and (ref["radii"] == 0).sum() >= 16
    check("quotients raw", cloud, origin_camera(160, 112), raw=True, stage_only=True)


def test_non_finite_inputs():
    """NaN and infinite scales, a zero quaternion, infinite and NaN means among ordinary Gaussians: what the reference computes."""
    base = scenes.config_c1(P=300, seed=77)
    means, scales, quats = base.means3D.numpy().copy(), base.scales.numpy().copy(), base.rotations.numpy().copy()
    scales[3, 0] = np.nan; scales[10] = np.inf; scales[64, 1] = np.inf; scales[65, 2] = -np.inf
    quats[20] = 0.0; quats[70] = np.nan
    means[30, 0] = np.inf; means[31, 2] = np.inf; means[32, 1] = -np.inf; means[33] = np.nan; means[130, 2] = np.nan
    cloud = cloud_of(means, scales, quats, base.opacities.numpy(), seed=5)
    _, _, ref = check("non-finite", cloud, scenes.c1_camera(160, 112), stage_only=True)
    assert ref["radii"][10] == 0 and (ref["radii"] > 0).sum() > 200
