"""Panoramas on the MI355X (autovfx_amd/panorama.py, csrc/gsr_panorama.hip): the cube-to-equirect kernel against the reference's
``c2e`` (the committed golden outputs: there is no reference tree on the GPU box) and against ``c2e_host`` (its numpy restatement,
held to the reference at <= 1e-12 by tests/test_panorama.py) at the reference's 1024^2 -> 1024 x 2048, the fused LDR bytes, the depth
option, the refusals, the faces in flight and the drop-in ``render_panorama`` end to end.

The parity bar ("Panoramas"): the face coordinates go through fp32 tan / cos in the reference, so device tanf / cosf against
numpy's move a coordinate by a few ulp; max-abs <= 5e-4 and mean-abs <= 2e-5 on noise faces (neighbouring texels differ by up to 1),
and a byte of pano_ldr.png may differ by one only where the reference's x * 255 lies within 255 * 5e-4 of an integer.
"""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from autovfx_amd import gaussian_model as gm
from autovfx_amd import panorama as pano
from autovfx_amd import renderer, scenes

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "pano", "c2e_*.npz")))
MAX_ABS, MEAN_ABS = 5e-4, 2e-5
DEV = "cuda:0"


def _planar(faces_hwc):
    """six [S, S, C] arrays -> six planar float32 [C, S, S] device tensors (what render()["render"] is)."""
    return [torch.from_numpy(np.ascontiguousarray(np.asarray(f, np.float32).transpose(2, 0, 1))).to(DEV) for f in faces_hwc]


def _hwc(faces_planar):
    return [f.permute(1, 2, 0).cpu().numpy() for f in faces_planar]


def _check_lsb_rule(ours: np.ndarray, ref: np.ndarray) -> int:
    """ours: uint8 bytes; ref: the reference's float64 panorama.  Every differing byte differs by one and lies where the reference's
    x * 255 is within 255 * MAX_ABS of an integer.  Returns the number of differing bytes."""
    ref_bytes = np.clip(ref * 255, 0, 255).astype(np.uint8)
    diff = ours.astype(np.int16) - ref_bytes.astype(np.int16)
    where = diff != 0
    assert np.abs(diff).max(initial=0) <= 1
    x = ref[where] * 255
    assert (np.abs(x - np.round(x)) <= 255 * MAX_ABS).all()
    return int(where.sum())


def _model(P=20_000, seed=3):
    c = scenes.config_c1(P=P, seed=seed)
    return gm.GaussianModel.from_activated(c.means3D, c.opacities, c.scales, c.rotations, c.shs, 3).to(DEV)


@pytest.mark.parametrize("path", GOLDEN, ids=os.path.basename)
def test_kernel_against_the_golden_files(path):
    g = np.load(path)
    h, w = int(g["h"]), int(g["w"])
    got = pano.cube_to_equirect(_planar(g["faces"]), h, w)
    torch.cuda.synchronize()
    err = np.abs(got.cpu().numpy().astype(np.float64) - g["c2e"])
    assert got.shape == (h, w, g["faces"].shape[-1]) and got.dtype == torch.float32
    assert err.max() <= MAX_ABS and err.mean() <= MEAN_ABS, (err.max(), err.mean())


def test_kernel_against_c2e_host_on_noise_at_full_size():
    rng = np.random.default_rng(7)
    faces = [rng.random((1024, 1024, 4), dtype=np.float32) for _ in range(6)]
    got = pano.cube_to_equirect(_planar(faces), 1024, 2048)
    u8 = pano.cube_to_equirect(_planar(faces), 1024, 2048, out_uint8=True)
    torch.cuda.synchronize()
    g = got.cpu().numpy()
    ref = pano.c2e_host(faces, 1024, 2048)
    err = np.abs(g.astype(np.float64) - ref)
    print(f"noise 1024^2 -> 1024x2048: max-abs {err.max():.3e}, mean-abs {err.mean():.3e}")
    assert err.max() <= MAX_ABS and err.mean() <= MEAN_ABS
    # the fused bytes are the float output's, truncated: uint8(clip(g * 255, 0, 255)) in fp32
    assert np.array_equal(u8.cpu().numpy(), np.clip(g * np.float32(255), 0, 255).astype(np.uint8))
    moved = _check_lsb_rule(u8.cpu().numpy(), ref)
    print(f"noise: {moved} of {ref.size} bytes differ from the reference's by one")


def test_kernel_against_c2e_host_on_rendered_faces():
    model, bg = _model(), torch.tensor([0.1, 0.2, 0.3], device=DEV)
    faces = pano.render_cube_faces(model, renderer.PipelineParams, bg, np.zeros(3), size=1024)
    planar = [faces[n]["render"] for n in pano.FACE_ORDER]
    got = pano.cube_to_equirect(planar, 1024, 2048)
    u8 = pano.cube_to_equirect(planar, 1024, 2048, out_uint8=True)
    torch.cuda.synchronize()
    ref = pano.c2e_host(_hwc(planar), 1024, 2048)
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
    print(f"rendered faces 1024^2 -> 1024x2048: max-abs {err.max():.3e}, mean-abs {err.mean():.3e}")
    assert err.max() <= MAX_ABS
    _check_lsb_rule(u8.cpu().numpy(), ref)


def test_depth_is_the_radial_distance_resampled():
    """The depth panorama is the resample of the radial-distance planes depth * |(2 cx, 2 cy, 1)| (cx, cy: the texel's pixel centre
    on the face plane): restated with torch ops and fed through the colour path as one-channel faces."""
    model, bg = _model(seed=5), torch.tensor([0.0, 0.0, 0.0], device=DEV)
    faces = pano.render_cube_faces(model, renderer.PipelineParams, bg, np.array([0.05, -0.1, 0.02]), size=256)
    planar = [faces[n]["render"] for n in pano.FACE_ORDER]
    depth = [faces[n]["depth"] for n in pano.FACE_ORDER]
    S = 256
    idx = torch.arange(S, device=DEV, dtype=torch.float32)
    x = (2 * idx + 1 - S) / S
    factor = torch.sqrt(1.0 + x[None, :] * x[None, :] + x[:, None] * x[:, None])     # [row, col]
    radial_planes = [(d * factor)[None] for d in depth]
    colour, radial = pano.cube_to_equirect(planar, 128, 256, depth=depth)
    expect = pano.cube_to_equirect(radial_planes, 128, 256)[..., 0]
    colour_only = pano.cube_to_equirect(planar, 128, 256)
    torch.cuda.synchronize()
    assert torch.equal(colour, colour_only)
    assert float(radial.abs().max()) > 0
    rel = ((radial - expect).abs() / expect.abs().clamp_min(1e-6)).max().item()
    assert rel <= 1e-5, rel
    # and against the numpy restatement of c2e over the same planes (float64 sums; coordinates a few ulp apart)
    ref = pano.c2e_host([p.permute(1, 2, 0).cpu().numpy() for p in radial_planes], 128, 256)[..., 0]
    assert np.abs(radial.cpu().numpy() - ref).max() <= MAX_ABS * float(np.abs(ref).max()) * 4


def test_refusals():
    faces = [torch.zeros(4, 8, 8, device=DEV) for _ in range(6)]
    with pytest.raises(ValueError):
        pano.cube_to_equirect(faces, 16, 36)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pano.cube_to_equirect([f.cpu() for f in faces], 16, 32)
    with pytest.raises(ValueError):
        pano.cube_to_equirect(faces[:5] + [torch.zeros(4, 9, 9, device=DEV)], 16, 32)
    from autovfx_amd import _lib
    out = torch.full((16, 36, 4), -1.0, device=DEV)
    u, v, c = (torch.zeros(n, device=DEV) for n in (36, 16, 9))
    ptrs = (ctypes.c_void_p * 6)(*[f.data_ptr() for f in faces])
    rc = _lib.lib.gsr_cube_to_equirect(ptrs, 8, 4, None, u.data_ptr(), v.data_ptr(), c.data_ptr(), 16, 36, out.data_ptr(), None, None,
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == -1 and "multiple of 8" in _lib.last_error()
    assert bool((out == -1.0).all())          # nothing was launched


def test_faces_in_flight_equal_blocking_renders():
    model, bg = _model(seed=9), torch.tensor([0.2, 0.1, 0.0], device=DEV)
    center = np.array([0.1, 0.05, -0.05])
    faces = pano.render_cube_faces(model, renderer.PipelineParams, bg, center, size=320)
    cams = pano.cube_map_cameras(center, 320)
    assert list(faces) == list(pano.VIEW_ORDER)
    for name in pano.VIEW_ORDER:
        with torch.no_grad():
            ref = renderer.render(cams[name].to(DEV), model, renderer.PipelineParams, bg)
        assert torch.equal(faces[name]["render"], ref["render"]), name
        assert torch.equal(faces[name]["depth"], ref["depth"]), name


def test_render_panorama_end_to_end(tmp_path):
    """The drop-in against the reference-shaped path built from this repository's render() + c2e_host + PIL: the same seven files,
    the same face pixels, the panorama within the one-LSB rule."""
    from PIL import Image
    model, bg = _model(seed=11), torch.tensor([0.0, 0.0, 0.0], device=DEV)
    center = np.array([0.02, -0.03, 0.01])
    S, h, w = 128, 128, 256
    ours_dir, ref_dir = tmp_path / "ours", tmp_path / "ref"
    path = pano.render_panorama(model, renderer.PipelineParams, bg, center, str(ours_dir), h, w, face_size=S)
    assert path == os.path.join(str(ours_dir), "pano_ldr.png")

    ref_dir.mkdir()
    cams, faces = pano.cube_map_cameras(center, S), {}
    with torch.no_grad():
        for name in pano.VIEW_ORDER:
            img = renderer.render(cams[name].to(DEV), model, renderer.PipelineParams, bg)["render"]
            arr = img.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8).numpy()   # save_image's bytes
            Image.fromarray(arr).save(ref_dir / f"{name}.png")
            faces[name] = img.permute(1, 2, 0).cpu().numpy()
    ref = pano.c2e_host(faces, h, w)
    Image.fromarray(np.clip(ref * 255, 0, 255).astype(np.uint8)).save(ref_dir / "pano_ldr.png")

    assert sorted(os.listdir(ours_dir)) == sorted(os.listdir(ref_dir)) == sorted([n + ".png" for n in pano.VIEW_ORDER] + ["pano_ldr.png"])
    for name in pano.VIEW_ORDER:
        a, b = Image.open(ours_dir / f"{name}.png"), Image.open(ref_dir / f"{name}.png")
        assert a.mode == b.mode == "RGBA" and np.array_equal(np.asarray(a), np.asarray(b)), name
    p = Image.open(path)
    assert p.mode == "RGBA" and p.size == (w, h)
    _check_lsb_rule(np.asarray(p), ref)

    path2, radial = pano.render_panorama(model, renderer.PipelineParams, bg, center, str(tmp_path / "again"), h, w, face_size=S,
                                         return_depth=True)
    assert radial.shape == (h, w) and radial.dtype == torch.float32 and radial.is_cuda
    assert np.array_equal(np.asarray(Image.open(path2)), np.asarray(p))
