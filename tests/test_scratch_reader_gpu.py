"""What gsr_backward and gsr_blend read out of a forward call's three scratch arenas, and what they refuse (gsr_api.hip: the
reader of the arena headers).  The headers of a call are remembered on the host under the arenas' addresses; a CLONE of the three
byte tensors is at addresses nobody remembers, so the same bytes take the other path -- three header copies from the device and a
wait -- and ``debug`` forces that path on the original buffers.  All of them must hand the kernels the same pointers: the results
are compared bit for bit (precomputed colours, and the deterministic backward, whose sums have a fixed order).

The refusals are decided on the host from the header's checked fields -- magic, kind, sizes, counts -- before anything is queued.
Only those fields are ever corrupted here: a header with a valid magic and a wrong OFFSET is not a refusal but a wild pointer, and
no test may build one.

One scene: 300 Gaussians of the C1 cube with doubled scales, precomputed colours, on 64 x 48 (4 x 3 whole tiles) and 70 x 50 (ragged
in both axes).
"""
import pytest
import torch

from autovfx_amd import _lib, scenes
from autovfx_amd.scenes import GaussianCloud

from helpers import settings_for

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = 300
BG = (0.1, 0.2, 0.3)
SIZES = [(64, 48), (70, 50)]
E = torch.Tensor([])


def scene(W, H):
    c = scenes.config_c1(P=P, seed=71)
    g = torch.Generator().manual_seed(72)
    cloud = GaussianCloud(c.means3D, c.opacities, c.scales * 2.0, c.rotations, None, torch.rand(P, 3, generator=g), 0).to(DEV)
    return cloud, settings_for(scenes.c1_camera(W, H), DEV, BG, 1.0, 0)


def forward(cloud, st, inference=False, deterministic=False):
    """One ``rasterize_gaussians`` call over the scene: its 8-tuple and the pairs of each depth slab.  An inference call is forced
    into slabs of a few pairs per tile, as helpers.hip_forward_inference does."""
    from diff_gaussian_rasterization import _C
    _C.set_geometry_cache(False)
    _lib.set_option(_lib.OPT_BACKWARD_DETERMINISTIC, 1 if deterministic else 0)
    if inference:
        _lib.set_option(_lib.OPT_SLABS, 0)
        _lib.set_option(_lib.OPT_SLAB_FIRST, 4)
        _lib.set_option(_lib.OPT_SLAB_MIN_REST, 0)
    try:
        out = _C.rasterize_gaussians(st.bg, cloud.means3D, cloud.colors_precomp, cloud.opacities, cloud.scales, cloud.rotations, 1.0, E,
                                     st.viewmatrix, st.projmatrix, st.tanfovx, st.tanfovy, st.image_height, st.image_width, E, 0,
                                     st.campos, False, False, inference=inference)
        torch.cuda.synchronize()
        return out, _C.last_layout()["slab_pairs"]
    finally:
        _lib.set_option(_lib.OPT_BACKWARD_DETERMINISTIC, 0)
        _lib.set_option(_lib.OPT_SLABS, 2)
        _lib.set_option(_lib.OPT_SLAB_FIRST, 400)
        _lib.set_option(_lib.OPT_SLAB_MIN_REST, 3000000)
        _C.set_geometry_cache(None)


def relocated(*arenas):
    """Clones of a call's byte tensors: the same bytes at addresses no forward call wrote.  The header is the first 256 bytes at the
    256-byte-aligned base, which for these tensors is their first byte."""
    clones = tuple(a.clone() for a in arenas)
    for a, c in zip(arenas, clones):
        assert a.data_ptr() % 256 == 0 and c.data_ptr() % 256 == 0 and c.data_ptr() != a.data_ptr()
    return clones


def blend(arenas, cloud, st, W, H):
    """gsr_blend over three arenas with the scene's colours: (colour, depth, alpha)."""
    geom, binning, image = arenas
    out = tuple(torch.empty((c, H, W), device=DEV) for c in (3, 1, 1))
    with torch.cuda.device(DEV):
        _lib.call("gsr_blend", geom.data_ptr(), binning.data_ptr(), image.data_ptr(), W, H, cloud.colors_precomp.data_ptr(),
                  st.bg.data_ptr(), *(t.data_ptr() for t in out), device=torch.device(DEV))
    torch.cuda.synchronize()
    return out


def backward(cloud, st, fwd, arenas, debug=False, R=None, W=None, H=None, rows=P):
    """rasterize_gaussians_backward over ``arenas`` with all-ones image gradients; ``R`` / ``W`` / ``H`` / ``rows``: what the call
    CLAIMS about the forward call (every tensor it hands over is sized for the claim)."""
    from diff_gaussian_rasterization import _C
    n, color, depth, alpha, radii = fwd[:5]
    H, W = depth.shape[1] if H is None else H, depth.shape[2] if W is None else W
    grow = lambda t: t if rows == t.shape[0] else torch.cat((t, t[:rows - t.shape[0]]))
    ones = lambda c: torch.ones((c, H, W), device=DEV)
    out = _C.rasterize_gaussians_backward(
        st.bg, grow(cloud.means3D), grow(radii), grow(cloud.colors_precomp), grow(cloud.scales), grow(cloud.rotations), 1.0, E,
        st.viewmatrix, st.projmatrix, st.tanfovx, st.tanfovy, ones(3), ones(1), ones(1), E, 0, st.campos, arenas[0],
        n if R is None else R, arenas[1], arenas[2], torch.zeros((1, H, W), device=DEV) if (H, W) != tuple(alpha.shape[1:]) else alpha,
        debug)
    torch.cuda.synchronize()
    return out


def assert_same_tuple(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), f"{what}: entry {i} differs"


@pytest.mark.parametrize("W,H", SIZES, ids=lambda v: str(v))
def test_a_second_blend_over_relocated_scratch_gives_the_same_images(W, H):
    cloud, st = scene(W, H)
    for inference in (False, True):
        fwd, slab_pairs = forward(cloud, st, inference=inference)
        if inference:
            assert sum(1 for n in slab_pairs if n > 0) >= 2, f"the scene should give two non-empty depth slabs: {slab_pairs}"
        else:
            assert len(slab_pairs) == 1 and slab_pairs[0] > 0, slab_pairs
        arenas = fwd[5:8]
        there = blend(arenas, cloud, st, W, H)                 # remembered headers
        moved = blend(relocated(*arenas), cloud, st, W, H)     # headers read from the device
        assert_same_tuple(moved, there, f"blend, inference={inference}: clones against the original buffers")
        assert_same_tuple(moved, fwd[1:4], f"blend, inference={inference}: clones against the forward call's own images")


@pytest.mark.parametrize("W,H", SIZES, ids=lambda v: str(v))
def test_the_deterministic_backward_over_relocated_scratch_gives_the_same_bits(W, H):
    cloud, st = scene(W, H)
    try:
        fwd, slab_pairs = forward(cloud, st, deterministic=True)
        assert len(slab_pairs) == 1
        _lib.set_option(_lib.OPT_BACKWARD_DETERMINISTIC, 1)
        arenas = fwd[5:8]
        remembered = backward(cloud, st, fwd, arenas, debug=False)
        moved = backward(cloud, st, fwd, relocated(*arenas))
        forced = backward(cloud, st, fwd, arenas, debug=True)
    finally:
        _lib.set_option(_lib.OPT_BACKWARD_DETERMINISTIC, 0)
    assert float(remembered[3].abs().sum()) > 0   # dL_dmeans3D
    assert_same_tuple(moved, remembered, "backward: clones against remembered headers")
    assert_same_tuple(forced, remembered, "backward: debug (forced device read) against remembered headers")


@pytest.fixture(scope="module")
def full_call():
    """One full forward call at 64 x 48 and its backward, shared by the refusals (nothing here is modified by them)."""
    cloud, st = scene(*SIZES[0])
    fwd, _ = forward(cloud, st)
    return cloud, st, fwd, backward(cloud, st, fwd, fwd[5:8])


def assert_still_works(cloud, st, fwd, want):
    """A valid call right after a refusal: the refusal queued nothing and left nothing behind."""
    W, H = SIZES[0]
    got = backward(cloud, st, fwd, fwd[5:8])
    for a, b in zip(got, want):   # float atomics: the same sums in another order
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()) + 1e-9 if a.numel() else True
    assert_same_tuple(blend(fwd[5:8], cloud, st, W, H), fwd[1:4], "blend after a refusal")


def refused_blend(arenas, cloud, st, W, H, words):
    """gsr_blend refuses with ``words`` and leaves the output images as they were."""
    geom, binning, image = arenas
    out = [torch.full(s, -7.0, device=DEV) for s in ((3, H, W), (1, H, W), (1, H, W))]
    with pytest.raises(RuntimeError, match=words), torch.cuda.device(DEV):
        _lib.call("gsr_blend", geom.data_ptr(), binning.data_ptr(), image.data_ptr(), W, H, cloud.colors_precomp.data_ptr(),
                  st.bg.data_ptr(), *(t.data_ptr() for t in out), device=torch.device(DEV))
    torch.cuda.synchronize()
    assert all(bool((t == -7.0).all()) for t in out), "a refused blend wrote into its outputs"


def test_swapped_arenas_are_refused(full_call):
    cloud, st, fwd, want = full_call
    W, H = SIZES[0]
    geom, binning, image = fwd[5:8]
    for swapped in ((binning, geom, image), (geom, image, binning)):
        refused_blend(swapped, cloud, st, W, H, "was not produced by gsr_forward")
        for debug in (False, True):
            with pytest.raises(RuntimeError, match="was not produced by gsr_forward"):
                backward(cloud, st, fwd, swapped, debug=debug)
    assert_still_works(cloud, st, fwd, want)


@pytest.mark.parametrize("which", range(3), ids=("geometry", "binning", "image"))
def test_a_scratch_without_its_magic_is_refused(full_call, which):
    cloud, st, fwd, want = full_call
    W, H = SIZES[0]
    clones = relocated(*fwd[5:8])
    clones[which][:4] = 0   # the header's magic word, nothing else
    refused_blend(clones, cloud, st, W, H, f"scratch buffer {which} was not produced by gsr_forward")
    with pytest.raises(RuntimeError, match=f"scratch buffer {which} was not produced by gsr_forward"):
        backward(cloud, st, fwd, clones)
    assert_still_works(cloud, st, fwd, want)


def test_another_image_size_is_refused(full_call):
    cloud, st, fwd, want = full_call
    W, H = SIZES[0]
    for arenas in (fwd[5:8], relocated(*fwd[5:8])):
        refused_blend(arenas, cloud, st, W + 16, H, "belong to")
        with pytest.raises(RuntimeError, match="belong to"):
            backward(cloud, st, fwd, arenas, W=W + 16)
    assert_still_works(cloud, st, fwd, want)


def test_another_gaussian_or_pair_count_is_refused(full_call):
    cloud, st, fwd, want = full_call
    for arenas in (fwd[5:8], relocated(*fwd[5:8])):
        with pytest.raises(RuntimeError, match="belong to a different call"):
            backward(cloud, st, fwd, arenas, rows=P + 1)
        with pytest.raises(RuntimeError, match="belong to a different call"):
            backward(cloud, st, fwd, arenas, R=fwd[0] + 1)
    assert_still_works(cloud, st, fwd, want)


def test_a_normal_gradient_over_a_scratch_without_normals_is_refused():
    from diff_gaussian_rasterization import _C
    from autovfx_amd.cameras import orbit_cameras
    from test_raw_gpu import call_raw, raw_model
    m, cam, bg = raw_model(P, 71, nasty=False), orbit_cameras(12, *SIZES[0])[7].to(DEV), torch.tensor(BG, device=DEV)
    H, W = int(cam.image_height), int(cam.image_width)
    n, color, depth, alpha, radii, geom, binning, image, normal = call_raw(m, cam, bg, inference=False, want_normal=False)
    torch.cuda.synchronize()
    assert normal is None

    def raw_backward(arenas, dL_dnormal):
        out = _C.rasterize_gaussians_raw_backward(
            bg, m._xyz, m._scaling, m._rotation, m._opacity, m._features_dc, m._features_rest, radii, 1.0, cam.world_view_transform,
            cam.full_proj_transform, cam.tanfovx, cam.tanfovy, torch.ones_like(color), None, None, dL_dnormal, m.active_sh_degree,
            cam.camera_center, arenas[0], n, arenas[1], arenas[2], alpha, False)
        torch.cuda.synchronize()
        return out

    for arenas in ((geom, binning, image), relocated(geom, binning, image)):
        with pytest.raises(RuntimeError, match="composited the normal image"):
            raw_backward(arenas, torch.ones_like(color))
    grads = raw_backward((geom, binning, image), None)   # the same scratch without the normal gradient is fine
    assert float(grads[1].abs().sum()) > 0
