"""Small scenes for the quadrant blend's slot staging (gsr_blend.hip: the entries of a 64-entry batch that reach a quadrant are
parked in up to SLOTS LDS slots in list order and walked from there; a batch with more is walked in rounds).  Shared by
tests/test_blend_terms_gpu.py and tests/blend_terms_unfused_check.py."""
import numpy as np
import torch

from autovfx_amd import scenes
from autovfx_amd.scenes import GaussianCloud

SLOTS = 32         # gsr_blend.hip: BlendSlots<false>::kCount
SLOTS_EXTRA = 30   # BlendSlots<true>::kCount (the second feature set's record takes the room of two slots)
BG = (0.2, 0.1, 0.3)
# one below, at and one above a round of either kernel; a batch of 64; two rounds and one entry; two batches and one entry
BOUNDARY_COUNTS = sorted({n + d for n in (SLOTS, SLOTS_EXTRA) for d in (-1, 0, 1)} | {63, 64, 65, 2 * SLOTS + 1, 2 * SLOTS_EXTRA + 1, 129})


def cloud_of(means, scales, opac, seed=0):
    P = len(means)
    g = torch.Generator().manual_seed(seed)
    t = lambda a: torch.as_tensor(np.asarray(a, np.float32)).contiguous()
    q = torch.randn(P, 4, generator=g)
    shs = torch.cat((torch.randn(P, 1, 3, generator=g), 0.2 * torch.randn(P, 15, 3, generator=g)), 1).contiguous()
    return GaussianCloud(t(means), t(opac).reshape(P, 1), t(scales), (q / q.norm(dim=1, keepdim=True)).contiguous(), shs, None, 3)


def splats(cam, px, py, vz, sigma_px):
    """Isotropic splats whose centres land on pixel coordinates (px, py) (pixel centres are at integers) at view depth vz, with a
    standard deviation of sigma_px pixels.  The C1 camera sits at z = -4 with an identity rotation."""
    px, py, vz, sigma_px = (np.asarray(a, np.float64) for a in (px, py, vz, sigma_px))
    W, H = cam.image_width, cam.image_height
    x = ((2.0 * px + 1.0) / W - 1.0) * cam.tanfovx * vz
    y = ((2.0 * py + 1.0) / H - 1.0) * cam.tanfovy * vz
    focal = W / (2.0 * cam.tanfovx)
    means = np.stack((x, y, vz - 4.0), 1).astype(np.float32)
    return means, np.repeat((sigma_px * vz / focal)[:, None], 3, 1).astype(np.float32)


def boundary_scene(k):
    """k faint splats (opacity 0.04: 0.96 ** 129 is far above the 1e-4 at which a pixel stops), all centred inside quadrant 3 of
    tile (1, 0) of a 32 x 32 image, with a sigma of 1.5 to 3 pixels: every one of them reaches that quadrant."""
    cam = scenes.c1_camera(32, 32)
    g = np.random.default_rng(1000 + k)
    means, scales = splats(cam, g.uniform(24.0, 31.0, k), g.uniform(8.0, 15.0, k), g.uniform(3.0, 6.0, k), g.uniform(1.5, 3.0, k))
    return cloud_of(means, scales, np.full((k, 1), 0.04, np.float32), seed=k), cam


def seam_scene(width, height, seed):
    """Eight splats of mixed size and opacity on every quadrant seam crossing and tile corner (pixel coordinates 7.5, 15.5, ...),
    in random depth order: every quadrant ranks a different subset of the shared list, and on these image sizes the quadrants
    at the right and bottom edges have lanes outside the image."""
    cam = scenes.c1_camera(width, height)
    g = np.random.default_rng(seed)
    xs, ys = np.arange(7.5, width, 8.0), np.arange(7.5, height, 8.0)
    px, py = (np.repeat(a.reshape(-1), 8) for a in np.meshgrid(xs, ys))
    n = len(px)
    means, scales = splats(cam, px, py, g.uniform(3.0, 6.0, n), g.uniform(0.6, 4.0, n))
    return cloud_of(means, scales, g.choice([0.04, 0.2, 0.6], (n, 1)).astype(np.float32), seed=seed), cam


def saturation_scene(seed=5):
    """48 x 32: forty nearly opaque splats with a sigma of ten pixels over tile (0, 0) -- its quadrants stop in the middle of a
    round, its neighbours' pixels stop one by one -- then 300 faint small splats everywhere, behind the stack and beside it."""
    cam = scenes.c1_camera(48, 32)
    g = np.random.default_rng(seed)
    m0, s0 = splats(cam, np.full(40, 7.5) + g.uniform(-1, 1, 40), np.full(40, 7.5) + g.uniform(-1, 1, 40), np.linspace(2.0, 2.4, 40), np.full(40, 10.0))
    m1, s1 = splats(cam, g.uniform(0.0, 47.0, 300), g.uniform(0.0, 31.0, 300), g.uniform(3.0, 6.0, 300), g.uniform(1.0, 3.0, 300))
    opac = np.concatenate((np.full((40, 1), 0.95, np.float32), np.full((300, 1), 0.06, np.float32)))
    return cloud_of(np.concatenate((m0, m1)), np.concatenate((s0, s1)), opac, seed=seed), cam


def finite_scenes():
    """(name, cloud, camera) of every scene above."""
    out = [(f"boundary{k}",) + boundary_scene(k) for k in BOUNDARY_COUNTS]
    out += [("seams37x29",) + seam_scene(37, 29, 7), ("seams24x16",) + seam_scene(24, 16, 8), ("saturation",) + saturation_scene()]
    return out
