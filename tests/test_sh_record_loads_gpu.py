"""The deferred colour kernels after they fetch a whole SH record in one round trip (``sh_colour_listed_kernel`` and
``sh_colour_all_kernel``: twelve aligned 16-byte loads and the position issued together, the evaluation from registers) against
the in-line colours of a full call (``preprocess_kernel``: ``sh_to_rgb``, coefficient by coefficient) -- BIT FOR BIT.

What is compared, per scene (``check``): the ``rgb`` block of the geometry arena (found through ``_C.last_layout()``) of an
inference call, for every Gaussian the call coloured (two slabs: the ones a list names, ``listed != 0``; one slab: the ones
with a radius), against the same rows of a full call; and the colour image.  As integer views, so that a NaN has to be the
same NaN.  Every scene runs twice: ``slabs=1`` (``sh_colour_all_kernel``) and ``slabs=2`` with a first slab of 8 pairs per
tile on a 64 x 64 image (``sh_colour_listed_kernel``, tags 1 and 2).

The record path is taken by degree 3 with sixteen coefficients in one 16-byte aligned block; lower degrees, fewer coefficients,
a base that is only 4-byte aligned and the raw call's two tensors keep the coefficient-by-coefficient path -- both are here.
"""
import dataclasses

import numpy as np
import pytest
import torch

from autovfx_amd import scenes
from autovfx_amd.scenes import GaussianCloud

from helpers import hip_forward_raw, settings_for

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BG = (0.1, 0.2, 0.3)
MODES = {"one_slab": 1, "two_slabs": 2}


def camera():
    return scenes.c1_camera(64, 64)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def with_options(slabs, fn):
    """``fn()`` with the slab options of these tests set; every option back to its default afterwards."""
    from autovfx_amd import _lib
    from diff_gaussian_rasterization import _C
    _C.set_geometry_cache(False)
    _lib.set_option(_lib.OPT_SLABS, slabs)
    _lib.set_option(_lib.OPT_SLAB_FIRST, 8)
    _lib.set_option(_lib.OPT_DEFER_COLOUR, 1)
    _lib.set_option(_lib.OPT_SLAB_MIN_REST, 0)
    try:
        return fn()
    finally:
        _lib.set_option(_lib.OPT_SLABS, 2)
        _lib.set_option(_lib.OPT_SLAB_FIRST, 400)
        _lib.set_option(_lib.OPT_DEFER_COLOUR, 1)
        _lib.set_option(_lib.OPT_SLAB_MIN_REST, 3000000)
        _C.set_geometry_cache(None)


def decode(out, P):
    """Image, radii, the arena's rgb block, the marks and the slab sizes of the call that returned ``out`` just now."""
    from diff_gaussian_rasterization import _C
    torch.cuda.synchronize()
    lay = _C.last_layout()
    geom = out[5]
    g = lay["geom"]
    rgb = geom[g["rgb"]:g["rgb"] + 12 * P].view(torch.float32).reshape(P, 3).cpu().numpy()
    slabs = len(lay["slab_pairs"])
    radii = out[4].cpu().numpy()
    listed = geom[g["listed"]:g["listed"] + P].cpu().numpy()
    bins = geom[g["splat_bins"]:g["splat_bins"] + 16 * P].view(torch.int32).reshape(P, 4).cpu().numpy()
    return {"color": out[1].cpu().numpy(), "radii": radii, "rgb": rgb, "listed": listed, "slabs": slabs, "emits": bins[:, 1] != 0,
            "coloured": (listed != 0) if slabs > 1 else (radii > 0)}


def inference_call(cloud, cam, slabs):
    """An inference call from activated inputs; the cloud's tensors are handed over as they are (device tensors stay views)."""
    from diff_gaussian_rasterization import _C
    c = cloud.to(DEV)
    st = settings_for(cam, DEV, BG, 1.0, cloud.sh_degree)
    e = torch.Tensor([])

    def call():
        with torch.no_grad():
            out = _C.rasterize_gaussians(st.bg, c.means3D, e, c.opacities, c.scales, c.rotations, 1.0, e, st.viewmatrix, st.projmatrix,
                                         st.tanfovx, st.tanfovy, st.image_height, st.image_width, c.shs, st.sh_degree, st.campos,
                                         False, False, inference=True)
        return decode(out, cloud.P)
    return with_options(slabs, call)


def raw_call(cloud, cam, slabs, inference):
    """``gsr_forward_raw`` (the render() boundary): separate ``features_dc`` / ``features_rest`` rows."""
    from diff_gaussian_rasterization import _C
    c, camd = cloud.to(DEV), cam.to(DEV)
    ls, rot = torch.log(c.scales), (c.rotations * 1.5).contiguous()
    op = torch.logit(c.opacities.reshape(-1, 1).clamp(1e-6, 1 - 1e-6))
    bg = torch.tensor(BG, device=DEV)

    def call():
        with torch.no_grad():
            out = _C.rasterize_gaussians_raw(bg, c.means3D, ls, rot, op, c.shs[:, :1].contiguous(), c.shs[:, 1:].contiguous(), 1.0,
                                             camd.world_view_transform, camd.full_proj_transform, camd.tanfovx, camd.tanfovy,
                                             cam.image_height, cam.image_width, cloud.sh_degree, camd.camera_center, False, True,
                                             want_normal=False, inference=inference)
        return decode(out, cloud.P)
    return with_options(slabs, call)


def full_call(cloud, cam):
    """A full call (in-line colours) and which Gaussians it coloured: the ones that emit pairs."""
    full = hip_forward_raw(cloud, cam, bg=BG, cull=True)
    full["emits"] = (full["tight_rect"][:, 2].astype(np.int64) * full["tight_rect"][:, 3]) != 0
    return full


def compare(name, got, full):
    """The deferred colours of ``got`` against the in-line colours of ``full``, and the images."""
    np.testing.assert_array_equal(got["radii"], full["radii"], err_msg=f"{name}: radii")
    # (a full call colours the Gaussians that emit pairs; sh_colour_all_kernel also the few with a radius whose every tile is dead)
    rows = got["coloured"] & full["emits"]
    assert not (got["coloured"] & ~(full["radii"] > 0)).any(), f"{name}: a Gaussian without a radius was coloured"
    if got["slabs"] > 1:
        assert not (got["coloured"] & ~full["emits"]).any(), f"{name}: a list names a Gaussian that emits nothing"
    np.testing.assert_array_equal(bits(got["rgb"][rows]), bits(full["rgb"][rows]), err_msg=f"{name}: rgb of {int(rows.sum())} coloured Gaussians")
    np.testing.assert_array_equal(bits(got["color"]), bits(full["color"]), err_msg=f"{name}: colour image")


def check(name, cloud, cam, two_slabs=None):
    """One scene: a full call once, then one inference call per mode against it.  ``two_slabs``: whether the two-slab mode has to
    end up with two slabs (None: whatever the scene's pair count gives)."""
    full = full_call(cloud, cam)
    got = {}
    for mode, slabs in MODES.items():
        got[mode] = inference_call(cloud, cam, slabs)
        compare(f"{name} {mode}", got[mode], full)
    assert got["one_slab"]["slabs"] == 1
    if two_slabs is not None:
        assert (got["two_slabs"]["slabs"] == 2) == two_slabs, f"{name}: {got['two_slabs']['slabs']} slabs"
    return full, got


def c1(P, seed, M=16, deg=3):
    base = scenes.config_c1(P=P, seed=seed)
    return GaussianCloud(base.means3D, base.opacities, base.scales, base.rotations, base.shs[:, :M].contiguous(), None, deg)


@pytest.mark.parametrize("P", [1, 255, 257, 1023, 1025, 4099])
def test_tails(P):
    """Clouds that end inside a wave's first lane, one short of and one past a wave's 256 Gaussians and a workgroup's 1024."""
    full, got = check(f"tail{P}", c1(P, 100 + P), camera(), two_slabs=True if P >= 1023 else None)
    if P >= 1023:
        marks = got["two_slabs"]["listed"]
        assert (marks == 1).any() and (marks == 2).any(), "both launches of sh_colour_listed_kernel were meant to colour something"
        assert (full["radii"] > 0).sum() > P // 2


@pytest.mark.parametrize("M", [1, 4, 9, 16])
@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_every_degree_and_width(deg, M):
    """Degree 0..3 declared over 1, 4, 9 and 16 coefficients: (3, 16) is the record path, every other pair the fallback --
    among them the degrees that M cannot hold and the kernels clamp (3 over 9: evaluated as 2)."""
    check(f"deg{deg} M{M}", c1(1500, 7 * deg + M, M=M, deg=deg), camera(), two_slabs=True)


def test_base_aligned_to_four_bytes_only():
    """``shs`` as a view one float into a larger allocation: 4-byte but not 16-byte aligned, so the fallback -- same bits as the
    aligned copy gives on the record path."""
    cloud = c1(1500, 31)
    cam = camera()
    aligned = cloud.to(DEV)
    store = torch.empty(cloud.P * 48 + 1, dtype=torch.float32, device=DEV)
    view = store[1:].view(cloud.P, 16, 3)
    view.copy_(aligned.shs)
    assert aligned.shs.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 and view.is_contiguous()
    shifted = GaussianCloud(aligned.means3D, aligned.opacities, aligned.scales, aligned.rotations, view, None, 3)
    full = full_call(cloud, cam)
    for mode, slabs in MODES.items():
        a = inference_call(aligned, cam, slabs)
        b = inference_call(shifted, cam, slabs)
        assert shifted.shs.data_ptr() == view.data_ptr()
        compare(f"aligned {mode}", a, full)
        compare(f"unaligned {mode}", b, full)
        np.testing.assert_array_equal(a["coloured"], b["coloured"])
        np.testing.assert_array_equal(bits(a["rgb"][a["coloured"]]), bits(b["rgb"][b["coloured"]]))
    assert a["slabs"] == 2


def test_raw_parameters():
    """The raw call with sixteen coefficients in two tensors (``shr = rest - 3``): deferred against in-line, both raw."""
    cloud = c1(1500, 41)
    cam = camera()
    full = raw_call(cloud, cam, 2, inference=False)
    assert (full["radii"] > 0).sum() > 700
    for mode, slabs in MODES.items():
        got = raw_call(cloud, cam, slabs, inference=True)
        compare(f"raw {mode}", got, full)
        assert got["slabs"] == slabs


def test_a_wave_with_all_256_listed_and_a_wave_with_one():
    """Wave 0's 256 Gaussians all reach the later slab's list (four passes of the evaluation loop), wave 2 holds exactly one
    listed Gaussian, wave 1 (faint, nearest: the first slab's cut falls among them) holds both tags."""
    base = c1(768, 51)
    g = np.random.default_rng(51)
    means = base.means3D.numpy().copy()
    opac = base.opacities.numpy().copy()
    means[:, :2] = g.uniform(-0.8, 0.8, (768, 2))
    means[0:256, 2] = g.uniform(0.5, 1.0, 256)       # far
    means[256:512, 2] = g.uniform(-1.0, -0.5, 256)   # near (the camera sits at z = -4 looking down +z)
    means[512:768, 2] = -6.0                         # behind the camera
    means[600, 2] = 0.75
    opac[0:256] = 0.5
    opac[256:512] = 0.02
    opac[600] = 0.5
    cloud = GaussianCloud(torch.from_numpy(means), torch.from_numpy(opac), base.scales, base.rotations, base.shs, None, 3)
    _, got = check("full wave", cloud, camera(), two_slabs=True)
    marks = got["two_slabs"]["listed"]
    assert (marks[0:256] == 2).all(), f"{int((marks[0:256] == 2).sum())} of wave 0 listed by the later slab"
    assert np.count_nonzero(marks[512:768]) == 1 and marks[600] != 0
    assert (marks[256:512] == 1).any() and (marks[256:512] == 2).any()


def test_non_finite_coefficients_and_a_gaussian_at_the_camera_position():
    """NaN and +-inf in single coefficients of every band, and ``campos`` on a visible Gaussian's mean (``len == 0``: the
    direction is 0 / 0): the non-finite colours are the in-line path's, bit for bit."""
    cloud = c1(1500, 61)
    cam = camera()
    shs = cloud.shs.numpy().copy()
    # which Gaussians both slabs' lists name depends on geometry and opacity alone: edit those, so that every mode colours them
    vis = np.flatnonzero(inference_call(cloud, cam, 2)["listed"] != 0)
    assert vis.size > 200
    values = (np.nan, np.inf, -np.inf)
    for k in range(16):                          # Gaussian vis[3 k + v]: value v in coefficient k, channel k % 3
        for v, value in enumerate(values):
            shs[vis[3 * k + v], k, k % 3] = value
    shs[vis[60], 5, :] = np.nan
    shs[vis[61], 0, 0] = np.inf; shs[vis[61], 9, 0] = -np.inf    # inf - inf
    at = int(vis[-1])
    bad = GaussianCloud(cloud.means3D, cloud.opacities, cloud.scales, cloud.rotations, torch.from_numpy(shs), None, 3)
    cam_at = dataclasses.replace(cam, camera_center=cloud.means3D[at].clone())
    full, got = check("non-finite", bad, cam_at, two_slabs=True)
    assert np.isnan(full["rgb"][at]).all(), "0 / 0 was meant to give a NaN direction"
    assert np.isnan(full["rgb"][vis[0]]).any() and np.isnan(full["rgb"][vis[61]]).any()
    for mode in MODES:
        rows = got[mode]["coloured"] & full["emits"]
        assert rows[at] and rows[vis[:62]].all(), f"{mode}: the edited Gaussians were meant to be coloured"
