"""The cube-to-equirect kernel (csrc/gsr_panorama.hip) held per pixel on the MI355X: at every seam of the padded map, on an odd face
size, on a partly filled workgroup, on the smallest call, on the depth path against a numpy restatement of its radial planes, with
all three outputs in one call between guards, and on a side stream.  tests/panorama_cases.py derives the bound from the reference's
own coordinate error; tests/test_panorama_seams.py shows on the CPU that the bound rejects every single wrong entry
of the padded map at the first case here.  All inputs are generated from seeds.
"""
import ctypes

import numpy as np
import pytest
import torch

import panorama_cases as cases
from autovfx_amd import panorama as pano

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S7 = cases.TAP_CASES[0]


def _planar(faces_hwc):
    """six [S, S, C] arrays -> six planar float32 [C, S, S] device tensors (what render()["render"] is)."""
    return [torch.from_numpy(np.ascontiguousarray(np.asarray(f, np.float32).transpose(2, 0, 1))).to(DEV) for f in faces_hwc]


def _depth_planes(S: int, seed: int) -> list:
    rng = np.random.default_rng(seed)
    return [rng.uniform(0.5, 20.0, (S, S)).astype(np.float32) for _ in range(6)]


def _guarded(count: int, dtype):
    """``count`` elements between two guards of 64, every byte 0xFF; returns ``(whole, inner)``."""
    if dtype == torch.uint8:
        whole = torch.full((count + 128,), 0xFF, dtype=torch.uint8, device=DEV)
    else:
        whole = torch.full((count + 128,), -1, dtype=torch.int32, device=DEV).view(dtype)
    return whole, whole[64:64 + count]


def _raw(t) -> torch.Tensor:
    return t if t.dtype == torch.uint8 else t.view(torch.int32)


def _guards_untouched(whole) -> bool:
    raw, fill = _raw(whole), (0xFF if whole.dtype == torch.uint8 else -1)
    return bool((raw[:64] == fill).all()) and bool((raw[-64:] == fill).all())


def test_coordinates_against_the_float64_truth():
    """Ramp faces away from the pads return the kernel's own (x, y): device tanf / cosf / sinf against the truth, within 4 E."""
    S, h, w = cases.COORDINATE_CASE
    got = pano.cube_to_equirect(_planar(cases.ramp_faces(S)), h, w)
    torch.cuda.synchronize()
    got = got.cpu().numpy().astype(np.float64)
    tp, u, v = cases.grid(h, w)
    rx, ry = pano._face_coordinates(tp, u, v, S)
    tx, ty = cases.truth_coordinates(tp, u, v, S)
    inside = (rx < S - 1 - 1e-3) & (ry < S - 1 - 1e-3)
    share = [float(inside[tp == k].mean()) for k in range(6)]
    assert min(share) >= 0.95, share
    e = cases.E(S, h, w)
    limit = 4 * e + 2.0 ** -25                           # 2^-25: the fp32 rounding of the output, in face-coordinate units
    err = np.maximum(np.abs(got[..., 0] / S - tx / S), np.abs(got[..., 1] / S - ty / S))[inside]
    ref_err = np.maximum(np.abs(rx - tx), np.abs(ry - ty))[inside].max() / S
    print(f"coordinates S {S} {h}x{w}: E {e / cases.ULP:.3f} x 2^-24 (inside {ref_err / cases.ULP:.3f}), kernel against the truth "
          f"{err.max() / cases.ULP:.3f} x 2^-24, limit {limit / cases.ULP:.3f} x 2^-24, ratio {err.max() / limit:.4f}; "
          f"inside share per face type {min(share):.3f} .. {max(share):.3f}")
    assert err.max() <= limit


@pytest.mark.parametrize("S,h,w,C", cases.TAP_CASES, ids=lambda n: str(n))
def test_noise_faces_within_the_bound_at_every_tap(S, h, w, C):
    faces = cases.noise_faces(S, C, seed=70 + S)
    got = pano.cube_to_equirect(_planar(faces), h, w)
    torch.cuda.synchronize()
    cases.check(got.cpu().numpy(), faces, h, w, what="kernel, noise")


def test_smallest_call_equals_the_reference_bit_for_bit():
    """S 2, 2 x 8: every pixel is up or down and tan is taken of an exact 0, so no device function can move a coordinate."""
    S, h, w = cases.SMALLEST_CASE
    for C in (1, 3, 4):
        faces = cases.noise_faces(S, C, seed=2 + C)
        got = pano.cube_to_equirect(_planar(faces), h, w)
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), pano.c2e_host(faces, h, w).astype(np.float32)), C


@pytest.mark.parametrize("S,h,w,C", cases.TAP_CASES[:2], ids=lambda n: str(n))
def test_depth_against_the_numpy_radial_planes(S, h, w, C):
    faces, depth = cases.noise_faces(S, C, seed=90 + S), _depth_planes(S, seed=91 + S)
    planar = _planar(faces)
    colour, radial = pano.cube_to_equirect(planar, h, w, depth=[torch.from_numpy(d).to(DEV) for d in depth])
    colour_only = pano.cube_to_equirect(planar, h, w)
    torch.cuda.synchronize()
    assert radial.shape == (h, w) and radial.dtype == torch.float32
    assert torch.equal(colour, colour_only)
    cases.check(radial.cpu().numpy()[..., None], cases.radial_planes(depth), h, w, what="kernel, depth")


@pytest.mark.parametrize("C", [1, 3, 4])
def test_three_outputs_in_one_call_between_guards(C):
    """The C entry point with out, out_u8 and out_depth all set (the Python wrapper passes floats or bytes, never both)."""
    from autovfx_amd import _lib
    S, h, w, _C = S7
    faces, depth = cases.noise_faces(S, C, seed=100 + C, lo=-0.5, hi=1.5), _depth_planes(S, seed=110 + C)
    F, D = _planar(faces), [torch.from_numpy(d).to(DEV) for d in depth]
    single, single_depth = pano.cube_to_equirect(F, h, w, depth=D)
    single_u8 = pano.cube_to_equirect(F, h, w, out_uint8=True)
    gu, gv, gc = pano._device_grid(h, w, torch.device(DEV))
    ptrs = (ctypes.c_void_p * 6)(*[f.data_ptr() for f in F])
    dptrs = (ctypes.c_void_p * 6)(*[d.data_ptr() for d in D])
    n = h * w
    for u8_fill in (0xFF, 0x00):               # a byte left unwritten shows against one of the two prefills
        (out_w, out), (u8_w, u8), (od_w, od) = _guarded(n * C, torch.float32), _guarded(n * C, torch.uint8), _guarded(n, torch.float32)
        u8.fill_(u8_fill)
        with torch.cuda.device(DEV):
            _lib.call("gsr_cube_to_equirect", ptrs, S, C, dptrs, gu.data_ptr(), gv.data_ptr(), gc.data_ptr(), h, w, out.data_ptr(),
                      u8.data_ptr(), od.data_ptr(), device=torch.device(DEV))
        torch.cuda.synchronize()
        assert _guards_untouched(out_w) and _guards_untouched(u8_w) and _guards_untouched(od_w)
        assert not bool((_raw(out) == -1).any()) and not bool((_raw(od) == -1).any())       # every float was written
        assert torch.equal(out.view(h, w, C), single) and torch.equal(od.view(h, w), single_depth)
        g = out.view(h, w, C).cpu().numpy()
        expect = np.clip(g * np.float32(255), 0, 255).astype(np.uint8)
        assert expect.min() == 0 and expect.max() == 255 and (g < 0).any() and (g > 1).any()   # both clips are exercised
        assert np.array_equal(u8.view(h, w, C).cpu().numpy(), expect)
        assert torch.equal(u8.view(h, w, C), single_u8)


def test_side_stream_equals_the_current_stream():
    S, h, w, C = S7
    faces, depth = cases.noise_faces(S, C, seed=120), _depth_planes(S, seed=121)
    F, D = _planar(faces), [torch.from_numpy(d).to(DEV) for d in depth]
    here, here_depth = pano.cube_to_equirect(F, h, w, depth=D)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        there, there_depth = pano.cube_to_equirect(F, h, w, depth=D)
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(here, there) and torch.equal(here_depth, there_depth)
