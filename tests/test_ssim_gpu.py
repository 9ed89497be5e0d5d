"""The fused SSIM (gsr_ssim.hip through autovfx_amd.ssim.ssim) on the GPU, held to a float64 truth: the value and the ``img1``
gradient must be no farther from it than twice the distance of the fp32 restatement (``ssim_restated``: the reference's own conv2d
graph) on the same device, measured as the scalar (or per-image vector) and as the max-abs gradient over elements.  Then the
properties a training loop relies on, and a short training loop through render().  Batches past the kernels' grid cap (65 536
workgroups, further tiles walked grid-stride) are held bit for bit to the same batch cut into calls below it; a grid of sizes sits on
the seams of the 32 x 16 tile and its 42 x 26 halo; and on frames made of regions the same rule is applied region by region."""
from __future__ import annotations

import ctypes

import pytest
import torch
import torch.nn.functional as F

from autovfx_amd import _lib, renderer, scenes
from autovfx_amd import ssim as S
from autovfx_amd.cameras import orbit_cameras
from autovfx_amd.frame_parallel import rasterize

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS32 = 2.0 ** -24


def truth(img1, img2, size_average, upstream):
    """SSIM in float64 from shifted-slice sums (no conv2d) with the reference's 2-D window (the fp32 outer product of
    gaussian(11, 1.5), as create_window builds it), and its img1 gradient by float64 autograd."""
    x = img1.detach().double().requires_grad_(True)
    y = img2.detach().double()
    taps = S.gaussian_window()
    w2 = (taps[:, None] @ taps[None, :]).double().tolist()
    H, W = x.shape[-2:]

    def blur(t):
        tp = F.pad(t, (5, 5, 5, 5))
        acc = torch.zeros_like(t)
        for i in range(11):
            for j in range(11):
                acc = acc + w2[i][j] * tp[..., i:i + H, j:j + W]
        return acc

    mx, my = blur(x), blur(y)
    exx, eyy, exy = blur(x * x), blur(y * y), blur(x * y)
    A1, A2 = 2 * mx * my + S.C1, 2 * (exy - mx * my) + S.C2
    B1, B2 = mx * mx + my * my + S.C1, (exx - mx * mx) + (eyy - my * my) + S.C2
    smap = A1 * A2 / (B1 * B2)
    val = smap.mean() if size_average else smap.flatten(1).mean(1)
    (grad,) = torch.autograd.grad(val, x, upstream.double())
    return val.detach(), grad


def value_and_grad(fn, img1, img2, size_average, upstream):
    x = img1.detach().clone().requires_grad_(True)
    val = fn(x, img2, 11, size_average)
    (grad,) = torch.autograd.grad(val, x, upstream)
    return val.detach(), grad


def check_against_truth(img1, img2, size_average=True, upstream=None):
    """Fused and restated against the truth; returns the fused (value, gradient)."""
    if upstream is None:
        upstream = torch.tensor(-0.2, device=img1.device)   # d(loss)/d(ssim) of 0.8 L1 + 0.2 (1 - ssim)
    ours_v, ours_g = value_and_grad(S.ssim, img1, img2, size_average, upstream)
    rest_v, rest_g = value_and_grad(S.ssim_restated, img1, img2, size_average, upstream)
    true_v, true_g = truth(img1, img2, size_average, upstream)
    assert ours_v.shape == rest_v.shape and ours_g.shape == img1.shape
    # Floors, both far below the quantities compared: the value is a mean of S in [-1, 1] rounded to fp32 at the end (a few units
    # of 2^-24); a gradient element is (g / M) times a sum of terms up to (|x| + |y|) * 2 / C2 in size whose fp32 rounding alone
    # is 2^-24 of that -- with img1 == img2 the truth is exactly 0 and both fp32 results are such residues.
    M = img1.numel() if size_average else img1[0].numel()
    floor_v = 4 * EPS32
    floor_g = 8 * EPS32 * float(upstream.abs().max()) / M * (float(img1.abs().max()) + float(img2.abs().max()) + 1.0) * 2 / S.C2
    err = lambda a, b: float((a.double() - b).abs().max())
    ev_ours, ev_rest = err(ours_v, true_v), err(rest_v, true_v)
    eg_ours, eg_rest = err(ours_g, true_g), err(rest_g, true_g)
    assert ev_ours <= 2 * ev_rest + floor_v, (ev_ours, ev_rest, floor_v)
    assert eg_ours <= 2 * eg_rest + floor_g, (eg_ours, eg_rest, floor_g, float(true_g.abs().max()))
    return ours_v, ours_g


def noise(shape, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.rand(shape, generator=g, device=DEV)


def check_regions_against_truth(img1, img2, regions, upstream=None):
    """check_against_truth's rule for the gradient, held on every region by itself: ``regions`` maps a name to a boolean [H, W] mask,
    the masks a partition of the image.  Per region, max|fused - truth| <= 2 max|restated - truth| + floor, the floor by the formula
    of check_against_truth from that region's own max|x| and max|y|.  The value (one number for the whole image) keeps its rule.
    Returns {name: (err_fused, err_restated, floor)}, the whole image under "all"."""
    if upstream is None:
        upstream = torch.tensor(-0.2, device=img1.device)
    ours_v, ours_g = value_and_grad(S.ssim, img1, img2, True, upstream)
    rest_v, rest_g = value_and_grad(S.ssim_restated, img1, img2, True, upstream)
    true_v, true_g = truth(img1, img2, True, upstream)
    assert ours_g.shape == img1.shape and ours_v.shape == rest_v.shape
    cover = sum(m.long() for m in regions.values())
    assert cover.shape == img1.shape[-2:] and bool((cover == 1).all()), "the regions must be a partition of the image"
    ev_ours, ev_rest = float((ours_v.double() - true_v).abs()), float((rest_v.double() - true_v).abs())
    assert ev_ours <= 2 * ev_rest + 4 * EPS32, (ev_ours, ev_rest)
    d_ours, d_rest = (ours_g.double() - true_g).abs(), (rest_g.double() - true_g).abs()
    scale = 8 * EPS32 * float(upstream.abs().max()) / img1.numel() * 2 / S.C2
    found = {}
    for name, mask in {**regions, "all": torch.ones_like(cover, dtype=torch.bool)}.items():
        assert int(mask.sum()) > 0, name
        m = mask.expand(img1.shape)
        floor_g = scale * (float(img1[m].abs().max()) + float(img2[m].abs().max()) + 1.0)
        found[name] = (float(d_ours[m].max()), float(d_rest[m].max()), floor_g)
    print("\n".join(f"region {k:>12}: {int(regions[k].sum()) if k in regions else cover.numel():7d} px  fused {a:.3e}  restated {b:.3e}"
                    f"  ratio {a / b if b else float('inf'):.3f}  floor {f:.3e}" for k, (a, b, f) in found.items()))
    bad = {k: v for k, v in found.items() if v[0] > 2 * v[1] + v[2]}
    assert not bad, bad
    return found


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("hw", [(1, 1), (5, 7), (10, 10), (1, 4099), (1081, 7), (540, 960)])
def test_noise_against_truth(C, hw):
    a, b = noise((C, *hw), 1), noise((C, *hw), 2)
    check_against_truth(a, 0.7 * a + 0.3 * b)


def test_full_hd_rgba_against_truth():
    a = noise((4, 1080, 1920), 3)
    check_against_truth(a, (a + 0.05 * noise((4, 1080, 1920), 4)).clamp(0, 1))


def test_batch_per_image_with_a_vector_upstream():
    a, b = noise((3, 4, 67, 45), 5), noise((3, 4, 67, 45), 6)
    b[1] = a[1]
    up = torch.tensor([-0.2, 0.5, 1.5], device=DEV)
    v, g = check_against_truth(a, b, size_average=False, upstream=up)
    assert v.shape == (3,) and float(v[1]) == pytest.approx(1.0, abs=1e-6)


def test_batch_mean():
    a, b = noise((3, 3, 40, 52), 7), noise((3, 3, 40, 52), 8)
    v, _ = check_against_truth(a, b, size_average=True)
    assert v.dim() == 0


def test_identical_images():
    a = noise((3, 64, 80), 9)
    v, g = check_against_truth(a, a.clone())
    assert float(v) == 1.0


@pytest.mark.parametrize("c1,c2", [(0.5, 0.5), (0.25, 0.75), (0.0, 1.0), (0.3, 0.7)])
def test_constant_images(c1, c2):
    check_against_truth(torch.full((3, 48, 50), c1, device=DEV), torch.full((3, 48, 50), c2, device=DEV))


def test_nhwc_view_as_the_sugar_trainers_build_it():
    """coarse_density.py:533-547: images held [H, W, 3], passed as .transpose(-1, -2).transpose(-2, -3) views."""
    hwc1, hwc2 = noise((2, 90, 70, 3), 10), noise((2, 90, 70, 3), 11)
    a, b = hwc1.transpose(-1, -2).transpose(-2, -3), hwc2.transpose(-1, -2).transpose(-2, -3)
    assert not a.is_contiguous()
    _, g = check_against_truth(a, b)
    ours = S.ssim(a, b)
    assert torch.equal(ours, S.ssim(a.contiguous(), b.contiguous()))


def rendered_pair():
    cloud, cam = scenes.config_c1(P=10_000, seed=0), scenes.c1_camera(256, 192)
    with torch.no_grad():
        color, _, alpha, _ = rasterize(cloud.to(DEV), cam.to(DEV), torch.tensor([0.1, 0.2, 0.3], device=DEV))
    gt = (color + 0.02 * torch.randn(color.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(12))).clamp(0, 1)
    return color.contiguous(), gt, alpha.reshape(alpha.shape[-2:])


def test_rendered_frame_against_a_perturbed_copy():
    color, gt, _ = rendered_pair()
    check_against_truth(color, gt)


def test_rendered_frame_background_and_covered_pixels_each_meet_the_bar():
    """The frame above, the rule held apart on the pixels no Gaussian reaches (alpha == 0: the flat background colour) and on the
    covered ones: over the whole frame one of the two sets both maxima."""
    color, gt, alpha = rendered_pair()
    check_regions_against_truth(color, gt, {"background": alpha == 0, "covered": alpha > 0})


def test_two_calls_are_bit_identical_on_any_stream():
    a, b = noise((4, 300, 500), 13), noise((4, 300, 500), 14)
    up = torch.tensor(-0.2, device=DEV)
    v0, g0 = value_and_grad(S.ssim, a, b, True, up)
    v1, g1 = value_and_grad(S.ssim, a, b, True, up)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        v2, g2 = value_and_grad(S.ssim, a, b, True, up)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(v0, v1) and torch.equal(g0, g1)
    assert torch.equal(v0, v2) and torch.equal(g0, g2)


def test_no_host_synchronisation():
    a, b = noise((2, 3, 128, 96), 15), noise((2, 3, 128, 96), 16)
    x = a.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = 0.8 * (x - b).abs().mean() + 0.2 * (1.0 - S.ssim(x, b))
        loss.backward()
        per = S.ssim(x, b, size_average=False)
        per.sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert x.grad is not None and bool(torch.isfinite(x.grad).all())


def test_no_grad_allocates_no_coefficient_maps():
    a, b = noise((3, 1080, 1920), 17), noise((3, 1080, 1920), 18)
    x = a.clone().requires_grad_(True)
    maps = 3 * a.numel() * 4
    torch.cuda.synchronize()
    for grad_on, cond in ((False, lambda d: d < maps // 8), (True, lambda d: d >= maps)):
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        with torch.set_grad_enabled(grad_on):
            v = S.ssim(x, b)
        torch.cuda.synchronize()
        assert cond(torch.cuda.max_memory_allocated() - base), (grad_on, torch.cuda.max_memory_allocated() - base)
        assert v.requires_grad == grad_on
        del v


def test_the_fallback_cases_on_the_gpu_are_the_restatement():
    a, b = noise((3, 20, 30), 19), noise((3, 20, 30), 20)
    assert torch.equal(S.ssim(a, b, window_size=7), S.ssim_restated(a, b, window_size=7))
    assert torch.equal(S.ssim(a.double(), b.double()), S.ssim_restated(a.double(), b.double()))
    with pytest.raises(Exception) as theirs:
        S.ssim_restated(a, b, size_average=False)
    with pytest.raises(theirs.type):
        S.ssim(a, b, size_average=False)


def test_training_loop_with_the_reference_loss():
    """0.8 L1 + 0.2 (1 - ssim) through render() with Adam, as the reference's loops: the loss goes down, and the loop with the
    restatement ends at the same loss to within optimisation noise."""
    from test_raw_autograd_gpu import PARAMS, leaves
    from test_raw_gpu import raw_model
    cam = orbit_cameras(12, 192, 120)[4].to(DEV)
    bg = torch.zeros(3, device=DEV)
    target = noise((4, 120, 192), 21)

    def loop(fn):
        m = leaves(raw_model(8_000, 404, nasty=False))
        opt = torch.optim.Adam([getattr(m, k) for k in PARAMS], lr=5e-3)
        losses = []
        for _ in range(10):
            img = renderer.render(cam, m, renderer.PipelineParams, bg)["render"]
            loss = 0.8 * (img - target).abs().mean() + 0.2 * (1.0 - fn(img, target))
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        return losses

    a, b = loop(S.ssim), loop(S.ssim_restated)
    assert a[-1] < a[0] and abs(a[-1] - b[-1]) < 2e-3 * abs(b[0]), (a, b)


# ---- tile seams: the tile is 32 x 16, its halo 5, the staged tile 42 x 26 ----

SEAM_H = (11, 15, 16, 17, 26, 27, 33)
SEAM_W = (11, 31, 32, 33, 37, 38, 42, 43, 65)


@pytest.mark.parametrize("W", SEAM_W)
@pytest.mark.parametrize("H", SEAM_H)
def test_sizes_on_the_tile_seams_against_truth(H, W):
    """Every pair of a height and a width around one tile, one tile and a pixel, one staged tile and one more: the last tile of a row
    or column one pixel wide or tall, alone or both at once (17 x 33), the halo reaching just to, or just past, the far edge.  Noise,
    so that the largest error over the image is a bar on every pixel."""
    a, b = noise((3, H, W), 30), noise((3, H, W), 31)
    check_against_truth(a, 0.7 * a + 0.3 * b)


@pytest.mark.parametrize("hw", [(1073, 1921), (1089, 1953)])
def test_full_frames_whose_last_tiles_are_one_pixel_wide_and_tall(hw):
    """67 x 16 + 1 rows and 60 x 32 + 1 columns (68 x 16 + 1 and 61 x 32 + 1): a one-pixel last tile row and column at frame scale."""
    assert hw[0] % 16 == 1 and hw[1] % 32 == 1
    a, b = noise((3, *hw), 32), noise((3, *hw), 33)
    check_against_truth(a, 0.7 * a + 0.3 * b)


# ---- frames made of regions: the bar on each region by itself ----

def mixed_frame(shift, device=DEV):
    """(4, 512, 768) in quadrants cut at row 256 + shift[0] and column 384 + shift[1]: flat 0.0 (a render's black background), flat
    0.5, a smooth ramp with +-0.01 noise, uniform noise; the second image is the first plus N(0, 0.02), clamped, as a ground-truth
    frame is to a render.  Pixels whose 10-pixel neighbourhood (the 11 taps of the forward, then of the backward) crosses a cut are
    a region of their own.  Returns (img1, img2, {name: [512, 768] mask})."""
    C, H, W = 4, 512, 768
    cy, cx = 256 + shift[0], 384 + shift[1]
    gen = torch.Generator(device=device).manual_seed(40)
    rows = torch.arange(H, device=device)[:, None].expand(H, W)
    cols = torch.arange(W, device=device)[None, :].expand(H, W)
    top, left = rows < cy, cols < cx
    ramp = 0.1 + 0.8 * (rows + cols).float() / (H + W - 2)
    ramp = ramp[None] * torch.tensor([1.0, 0.8, 0.6, 0.4], device=device)[:, None, None]
    ramp = ramp + 0.02 * (torch.rand((C, H, W), generator=gen, device=device) - 0.5)
    img1 = torch.rand((C, H, W), generator=gen, device=device)
    img1 = torch.where(~top & left, ramp, img1)
    img1 = torch.where(top & ~left, torch.full_like(img1, 0.5), img1)
    img1 = torch.where(top & left, torch.zeros_like(img1), img1).contiguous()
    img2 = (img1 + 0.02 * torch.randn((C, H, W), generator=gen, device=device)).clamp(0, 1)
    # rows cy - 10 .. cy + 9 see the other side of the cut between rows cy - 1 and cy, and the same for the columns
    border = ((rows >= cy - 10) & (rows <= cy + 9)) | ((cols >= cx - 10) & (cols <= cx + 9))
    regions = {"flat 0.0": top & left & ~border, "flat 0.5": top & ~left & ~border, "ramp": ~top & left & ~border,
               "noise": ~top & ~left & ~border, "borders": border}
    return img1, img2, regions


@pytest.mark.parametrize("shift", [(0, 0), (8, 16)], ids=["cuts_between_tiles", "cuts_inside_tiles"])
def test_mixed_frame_meets_the_bar_in_every_region(shift):
    """On a frame like a render the low-variance parts set both maxima of check_against_truth (B2 ~ C2 there: the gradient carries
    a factor 2 / C2; measured, the ramp and flat 0.5, where the restatement is 500 times farther from the truth than on noise), and
    an error in the textured part could hide below them.  Here every region answers for itself (figures: DESIGN.md 7c)."""
    img1, img2, regions = mixed_frame(shift)
    assert all(int(m.sum()) >= 10_000 for m in regions.values())   # the restatement's maximum over a region is a stable yardstick
    check_regions_against_truth(img1, img2, regions)


# ---- past the grid cap: 65 536 workgroups are launched, further tiles walked grid-stride ----

GRID_CAP = 1 << 16
# shape, tiles, images per call below the cap
PAST_THE_CAP = [((6000, 3, 17, 33), 72_000, 1000),      # planes of 2 x 2 ragged tiles: a workgroup's second tile is in another plane
                ((12000, 3, 17, 33), 144_000, 1000),    # more than twice the cap: some workgroups walk three tiles
                ((60, 4, 300, 500), 72_960, 20)]        # 304 tiles per plane do not divide the cap: another position of another plane
CAP_IDS = ["6000x3x17x33", "12000x3x17x33", "60x4x300x500"]


def tiles(shape):
    n, c, h, w = shape
    return n * c * ((w + 31) // 32) * ((h + 15) // 16)


def cap_pair(shape):
    a = noise(shape, 50)
    return a, (0.7 * a + 0.3 * noise(shape, 51)).contiguous()


def forward_maps(x, y, per_image):
    """gsr_ssim_forward called directly: (value, the three coefficient maps as one [3 * numel] tensor)."""
    n, c, h, w = x.shape
    out = torch.empty((n,) if per_image else (), dtype=torch.float32, device=x.device)
    coef = torch.empty(3 * x.numel(), dtype=torch.float32, device=x.device)
    nbytes = int(_lib.lib.gsr_ssim_scratch_bytes(n, c, h, w))
    scratch = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=x.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
    rc = _lib.lib.gsr_ssim_forward(n, c, h, w, x.data_ptr(), y.data_ptr(), S.WINDOW11, int(per_image), out.data_ptr(), coef.data_ptr(),
                                   scratch.data_ptr(), nbytes, stream)
    assert rc == 0, _lib.last_error()
    return out, coef


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("shape,count,per_call", PAST_THE_CAP, ids=CAP_IDS)
def test_past_the_grid_cap_each_image_has_the_bits_of_a_call_below_it(shape, count, per_call):
    """Per image, with an upstream gradient that differs per image: the values and the img1 gradient of one call over the whole batch
    equal, bit for bit, those of calls over consecutive slices that each stay below the cap.  Nothing of an image's result depends on
    where it sits in the batch: a tile's partial, the fixed-order sum of an image's partials and grad_out[image] / (C H W) are
    functions of the image alone.  Tiles walked in a second or third loop iteration that read or wrote the wrong place, or were not
    walked at all, differ."""
    assert tiles(shape) == count > GRID_CAP and tiles((per_call, *shape[1:])) < GRID_CAP and shape[0] % per_call == 0
    a, b = cap_pair(shape)
    up = 0.25 + torch.arange(shape[0], device=DEV, dtype=torch.float32) / shape[0]
    assert up.unique().numel() == shape[0]
    v, g = value_and_grad(S.ssim, a, b, False, up)
    for i in range(0, shape[0], per_call):
        sl = slice(i, i + per_call)
        vs, gs = value_and_grad(S.ssim, a[sl], b[sl], False, up[sl])
        assert same_bits(v[sl], vs), (i, float((v[sl] - vs).abs().max()))
        bad = (g[sl] != gs).flatten(1).any(1).nonzero().flatten()
        assert same_bits(g[sl], gs), (i, "images that differ", (bad[:8] + i).tolist(), float((g[sl] - gs).abs().max()))


@pytest.mark.parametrize("shape,count,per_call", PAST_THE_CAP, ids=CAP_IDS)
def test_past_the_grid_cap_the_mean_against_truth(shape, count, per_call):
    """The mean over the whole batch and its gradient, by the rule of every test here.  The float64 autograd of the truth peaks at
    5.4 GiB for the largest of the three (36 M elements), so it is taken in one piece."""
    assert tiles(shape) == count > GRID_CAP
    a, b = cap_pair(shape)
    v, _ = check_against_truth(a, b, size_average=True)
    assert v.dim() == 0


@pytest.mark.parametrize("shape,count,per_call", PAST_THE_CAP, ids=CAP_IDS)
def test_past_the_grid_cap_two_calls_are_bit_identical(shape, count, per_call):
    """Value, gradient, and the coefficient maps as gsr_ssim_forward writes them: a workgroup that staged its next tile into LDS
    another wave was still reading would most likely not do so the same way twice."""
    assert tiles(shape) == count > GRID_CAP
    a, b = cap_pair(shape)
    up = torch.tensor(-0.2, device=DEV)
    v0, g0 = value_and_grad(S.ssim, a, b, True, up)
    v1, g1 = value_and_grad(S.ssim, a, b, True, up)
    assert same_bits(v0, v1) and same_bits(g0, g1)
    maps = {}
    for per_image in (False, True):
        o0, maps[per_image] = forward_maps(a, b, per_image)
        o1, again = forward_maps(a, b, per_image)
        assert same_bits(o0, o1) and same_bits(maps[per_image], again), per_image
        assert bool(torch.isfinite(again).all())
        if not per_image:
            assert same_bits(o0, v0)            # the call the autograd function made
    assert same_bits(maps[False], maps[True])   # the maps are per pixel: how the values are averaged does not reach them
