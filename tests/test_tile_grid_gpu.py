"""Full renders across the tile-count boundaries of the tile sort.

The tile keys are bit_length(T) bits wide (gsr_api.hip: tile_key_bits), so the tile count decides how many radix passes the
tile sort makes (1 up to 255 tiles, 2 up to 65 535, 3 above), which buffer the sorted list ends up in (the caller picks the
expansion's output buffer by the parity of the pass count) and what the expansion's pre-count of the first digit covers.  Every
grid below goes through ``run_both`` (lists, keys and ranges bit for bit against the CPU oracle with culling off, culled lists
that are subsequences, inference calls equal to the full call); the 3-pass grids also through the backward in every mode.
The clouds fill the whole frustum, with splats pinned on the last tiles and around tile 65 536, so that the highest tile ids
hold lists; they are mostly splats of a few tiles (the oracle stays quick) plus some that span many tiles (the run pool).
"""
import ctypes

import numpy as np
import pytest
import torch

from autovfx_amd import scenes
from autovfx_amd.scenes import GaussianCloud

from test_backward_gpu import KEYS_SH, MODES, check_case
from test_oracle_backward import pixel_grads
from test_parity_gpu import report, run_both

pytestmark = pytest.mark.gpu


def tile_bits(T):
    return int(T).bit_length()


def tile_passes(T):
    return (tile_bits(T) + 7) // 8


def grid_of(W, H):
    gx, gy = (W + 15) // 16, (H + 15) // 16
    return gx, gy, gx * gy


# (W, H, small splats, large splats): what each grid pins in the comments
GRIDS = [
    (256, 240, 600, 8),            # T = 240: 8 tile bits, 1 pass, ordered blend off
    (4112, 16, 1500, 20),          # T = 257: 9 bits, 2 passes, the first ordered-blend size
    (4096, 4080, 30_000, 150),     # T = 65 280: 16 bits, the top of 2 passes
    (4096, 4096, 30_000, 150),     # T = 65 536: 17 bits, the first 3-pass grid (the third digit is constant)
    (7680, 4320, 40_000, 150),     # T = 129 600: 3 passes with tile ids >= 65 536 that hold lists
    (1_048_560, 32, 40_000, 150),  # T = 131 070: grid_x = 65 535 exactly, 3 passes
]


def grid_id(g):
    W, H = g[0], g[1]
    T = grid_of(W, H)[2]
    return f"{W}x{H}_T{T}_bits{tile_bits(T)}_passes{tile_passes(T)}"


def frustum_cloud(cam, small, large, seed, pinned_tiles=()):
    """Splats placed in screen space over the whole image at depths 2 - 6 in front of the camera (scenes.c1_camera: at z = -4
    looking down +z), sized in pixels: `small` of sigma 0.7 - 2.5 px (a few tiles each), `large` of 15 - 60 px, and one small
    splat on the centre of every tile in `pinned_tiles`."""
    rng = np.random.default_rng(seed)
    W, H = cam.image_width, cam.image_height
    gx = (W + 15) // 16
    tx, ty = cam.tanfovx, cam.tanfovy
    focal = W / (2.0 * tx)
    pins = np.asarray(sorted(set(int(t) for t in pinned_tiles)), np.int64)
    n = small + large + pins.size
    u, v = rng.uniform(0, W, n), rng.uniform(0, H, n)
    u[small + large:] = np.minimum((pins % gx) * 16 + 8, W - 1) + 0.25
    v[small + large:] = np.minimum((pins // gx) * 16 + 8, H - 1) + 0.25
    z = rng.uniform(2.0, 6.0, n)
    x = ((2.0 * u + 1.0) / W - 1.0) * tx * z
    y = ((2.0 * v + 1.0) / H - 1.0) * ty * z
    means = np.stack([x, y, z - 4.0], 1)
    sigma_px = rng.uniform(0.7, 2.5, n)
    sigma_px[small:small + large] = rng.uniform(15.0, 60.0, large)
    scales = (sigma_px * z / focal)[:, None] * np.exp(rng.normal(0.0, 0.3, (n, 3)))
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    opac = rng.uniform(0.15, 0.95, (n, 1))
    shs = np.concatenate([rng.standard_normal((n, 1, 3)), 0.2 * rng.standard_normal((n, 15, 3))], 1)
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
    return GaussianCloud(f32(means), f32(opac), f32(scales), f32(q), f32(shs), None, 3)


def pinned_for(T):
    """The first and the last tiles, and the tiles around the 16-bit boundary of the tile ids."""
    return [t for t in (0, 1, 255, 256, 65_534, 65_535, 65_536, 65_537, T - 2, T - 1) if 0 <= t < T]


@pytest.mark.parametrize("grid", GRIDS, ids=grid_id)
def test_lists_at_every_tile_sort_pass_count(grid):
    W, H, small, large = grid
    gx, gy, T = grid_of(W, H)
    assert gx <= 65535 and gy <= 65535
    cam = scenes.c1_camera(W, H)
    cloud = frustum_cloud(cam, small, large, seed=T, pinned_tiles=pinned_for(T))
    name = "grid_" + grid_id(grid)
    hip, ref = run_both(name, cloud, cam, bg=(0.05, 0.1, 0.15))
    tiles = (ref["point_list_keys"] >> np.uint64(32)).astype(np.int64)
    assert int(tiles.max()) == T - 1, "the last tile holds no list: the top of the key range went unused"
    if T > 65_536:
        assert int((tiles >= 65_536).sum()) > 1000, "too few pairs on tile ids above 16 bits"
    assert hip["point_list"].size == ref["num_rendered"] > 0
    report(name + ":grid", tiles=T, tile_bits=tile_bits(T), passes=tile_passes(T), pairs=int(ref["num_rendered"]),
           tiles_with_lists=int(np.unique(tiles).size))


THREE_PASS_GRIDS = [g for g in GRIDS if tile_passes(grid_of(g[0], g[1])[2]) == 3]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("grid", THREE_PASS_GRIDS, ids=grid_id)
def test_backward_on_three_pass_grids(grid, mode):
    """The backward walks the lists the 3-pass tile sort left in the slab's buffers: every gradient against the fp64 truth, the
    forward state against the oracle first (check_case), on a cloud sparse enough for the CPU backward."""
    W, H = grid[0], grid[1]
    T = grid_of(W, H)[2]
    cam = scenes.c1_camera(W, H)
    cloud = frustum_cloud(cam, 6000, 20, seed=T + 1, pinned_tiles=pinned_for(T))
    check_case("grid3_" + grid_id(grid), cloud, cam, pixel_grads(cam, 3), KEYS_SH, mode, bg=(0.2, 0.1, 0.0))


def test_grid_x_of_65536_is_refused_before_anything_is_written():
    """Width 1 048 561 = 65 536 tile columns, one more than the tile rectangles can hold: gsr_forward refuses it with "image too
    large" before it asks for scratch or launches anything -- the poisoned outputs stay as they were."""
    from autovfx_amd import _lib
    W, H = 1_048_561, 16
    assert grid_of(W, H)[0] == 65_536
    dev = "cuda:0"
    cam = scenes.c1_camera(W, H)
    c = frustum_cloud(cam, 64, 0, seed=5).to(dev)
    camd = cam.to(dev)
    bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    outs = [torch.full((3, H, W), -7.0, device=dev), torch.full((1, H, W), -7.0, device=dev),
            torch.full((1, H, W), -7.0, device=dev)]
    radii = torch.full((c.P,), -7, dtype=torch.int32, device=dev)
    asked = []
    cb = _lib.ALLOC_FN(lambda nbytes, user: asked.append(int(nbytes)) or None)
    torch.cuda.synchronize()
    rc = _lib.lib.gsr_forward(cb, None, cb, None, cb, None, c.P, 3, 16, bg.data_ptr(), W, H, c.means3D.data_ptr(),
                              c.shs.data_ptr(), None, c.opacities.data_ptr(), c.scales.data_ptr(), 1.0, c.rotations.data_ptr(),
                              None, camd.world_view_transform.data_ptr(), camd.full_proj_transform.data_ptr(),
                              camd.camera_center.data_ptr(), cam.tanfovx, cam.tanfovy, 0, outs[0].data_ptr(), outs[1].data_ptr(),
                              outs[2].data_ptr(), radii.data_ptr(), 0,
                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc != 0 and "image too large" in _lib.last_error(), (rc, _lib.last_error())
    assert asked == [], "scratch was requested for a refused call"
    for t in outs:
        assert bool((t == -7.0).all()), "a refused call wrote into an output image"
    assert bool((radii == -7).all()), "a refused call wrote radii"
