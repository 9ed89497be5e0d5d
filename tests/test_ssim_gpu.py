"""The fused SSIM (gsr_ssim.hip through autovfx_amd.ssim.ssim) on the GPU, held to a float64 truth: the value and the ``img1``
gradient must be no farther from it than twice the distance of the fp32 restatement (``ssim_restated``: the reference's own conv2d
graph) on the same device, measured as the scalar (or per-image vector) and as the max-abs gradient over elements.  Then the
properties a training loop relies on, and a short training loop through render()."""
from __future__ import annotations

import pytest
import torch
import torch.nn.functional as F

from autovfx_amd import renderer, scenes
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


def test_rendered_frame_against_a_perturbed_copy():
    cloud, cam = scenes.config_c1(P=10_000, seed=0), scenes.c1_camera(256, 192)
    with torch.no_grad():
        color, _, _, _ = rasterize(cloud.to(DEV), cam.to(DEV), torch.tensor([0.1, 0.2, 0.3], device=DEV))
    gt = (color + 0.02 * torch.randn(color.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(12))).clamp(0, 1)
    check_against_truth(color.contiguous(), gt)


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
