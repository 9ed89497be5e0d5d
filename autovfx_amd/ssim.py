"""The structural similarity of the reference's training loss, ``loss_utils.ssim`` (``utils/loss_utils.py:33-62``), on the GPU.

Every training loop of the reference computes ``(1 - l) * l1_loss(image, gt) + l * (1 - ssim(image, gt))``.  :func:`ssim` has the
reference's signature and results; its forward and its gradient for ``img1`` are the HIP kernels of ``gsr_ssim.hip`` (C ABI
``gsr_ssim_forward`` / ``gsr_ssim_backward``): one pass over both images for the value and three coefficient maps,
one pass over the maps for the gradient, no host synchronisation, no atomics.

The kernels take the calls they were built for: CUDA fp32 tensors of one shape ``[C,H,W]`` or ``[N,C,H,W]`` on one device, window 11,
``size_average`` true (or false with a batch), no gradient for ``img2``, fewer than 2^31 elements.  Every other call goes to the
function being replaced -- under ``autovfx_amd.install()`` the reference's own ``ssim``, here :func:`ssim_restated` -- so a CPU
tensor, another dtype or window size, mismatched shapes give exactly the reference's result or its exception.
"""
from __future__ import annotations

import ctypes
import math
from typing import Callable

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib, _takes

WINDOW_SIZE = 11
SIGMA = 1.5
C1 = 0.01 ** 2
C2 = 0.03 ** 2
MAX_ELEMENTS = (1 << 31) - 1


def gaussian_window(size: int = WINDOW_SIZE, sigma: float = SIGMA) -> torch.Tensor:
    """The reference's ``gaussian(size, sigma)``: fp64 exponentials rounded to fp32, divided by their fp32 sum.  float32 ``[size]``."""
    taps = torch.tensor([math.exp(-(i - size // 2) ** 2 / float(2 * sigma ** 2)) for i in range(size)], dtype=torch.float32)
    return taps / taps.sum()


# the weights every kernel call gets (host memory: the C ABI copies them into the launch arguments)
WINDOW11 = (ctypes.c_float * WINDOW_SIZE)(*gaussian_window().tolist())


def ssim_restated(img1, img2, window_size=11, size_average=True):
    """The reference's ``ssim`` in PyTorch operations, the same ones in the same order (so the same bits on any device): five
    depthwise ``conv2d`` with the outer product of :func:`gaussian_window`, zero padding, the SSIM map, its mean (or per-image means)."""
    channel = img1.size(-3)
    taps = gaussian_window(window_size, SIGMA).unsqueeze(1)
    window = taps.mm(taps.t()).float()[None, None].expand(channel, 1, window_size, window_size).contiguous()
    if img1.is_cuda:
        window = window.cuda(img1.get_device())
    window = window.type_as(img1)

    def blur(t):
        return F.conv2d(t, window, padding=window_size // 2, groups=channel)

    mu1, mu2 = blur(img1), blur(img2)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    var1 = blur(img1 * img1) - mu1_sq
    var2 = blur(img2 * img2) - mu2_sq
    cov = blur(img1 * img2) - mu1_mu2
    smap = ((2 * mu1_mu2 + C1) * (2 * cov + C2)) / ((mu1_sq + mu2_sq + C1) * (var1 + var2 + C2))
    if size_average:
        return smap.mean()
    return smap.mean(1).mean(1).mean(1)


def _fused_takes(img1, img2, window_size, size_average) -> bool:
    if _takes.tensors((("img1", img1, torch.float32), ("img2", img2, torch.float32))) is not None or img1.shape != img2.shape:
        return False
    if img1.dim() not in (3, 4) or type(window_size) is not int or window_size != WINDOW_SIZE:
        return False
    if not size_average and img1.dim() != 4:
        return False
    if img2.requires_grad and torch.is_grad_enabled():
        return False
    return 0 < img1.numel() <= MAX_ELEMENTS


def _dims(t: torch.Tensor):
    return (1, *t.shape) if t.dim() == 3 else tuple(t.shape)


class _FusedSSIM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img1, img2, per_image, want_grad):
        x, y = _takes.cs(img1, img2)
        n, c, h, w = _dims(x)
        with torch.cuda.device(x.device):
            out = torch.empty((n,) if per_image else (), dtype=torch.float32, device=x.device)
            coef = torch.empty(3 * x.numel(), dtype=torch.float32, device=x.device) if want_grad else None
            nbytes = int(_lib.lib.gsr_ssim_scratch_bytes(n, c, h, w))
            scratch = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=x.device)
            _lib.call("gsr_ssim_forward", n, c, h, w, x.data_ptr(), y.data_ptr(), WINDOW11, int(per_image), out.data_ptr(),
                      _lib.ptr(coef), scratch.data_ptr(), nbytes, device=x.device)
        if want_grad:
            ctx.save_for_backward(x, y, coef)
            ctx.per_image = per_image
            ctx.shape = img1.shape
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x, y, coef = ctx.saved_tensors
        n, c, h, w = _dims(x)
        g = grad_out.detach().to(torch.float32).contiguous()
        grad = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.call("gsr_ssim_backward", n, c, h, w, x.data_ptr(), y.data_ptr(), coef.data_ptr(), WINDOW11, int(ctx.per_image),
                      g.data_ptr(), grad.data_ptr(), device=x.device)
        return grad.view(ctx.shape), None, None, None


def drop_in(fallback: Callable) -> Callable:
    """An ``ssim(img1, img2, window_size=11, size_average=True)`` that runs the kernels where they apply and ``fallback`` (same
    signature) everywhere else.  ``autovfx_amd.install()`` builds one per patched ``loss_utils`` module around the reference's own."""

    def ssim(img1, img2, window_size=11, size_average=True):
        if not _fused_takes(img1, img2, window_size, size_average):
            return fallback(img1, img2, window_size, size_average)
        # (needs_input_grad does not see torch.no_grad(): the maps are written only when a gradient can be asked for)
        return _FusedSSIM.apply(img1, img2, not size_average, img1.requires_grad and torch.is_grad_enabled())

    return _takes.dressed(ssim, "ssim", fallback, "loss_utils.ssim, the mean SSIM of img1 against img2 (per image with size_average=False)", "ssim")


ssim = drop_in(ssim_restated)
