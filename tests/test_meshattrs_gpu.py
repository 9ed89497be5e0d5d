"""pytorch3d's face areas / normals and face-attribute interpolation on the GPU (gsr_meshattrs.hip through autovfx_amd.meshattrs): the two
forwards and ``grad_bary`` bit for bit the numpy restatement of the contract -- the same IEEE operations in the same order, contraction off --
and the two atomically summed outputs inside the bound that follows from the contract's fp32 terms added in a free order
(cases.atomic_sum_check).  Sizes: one lane, the edges of a wave and of a workgroup (256 faces, 256 slots), several workgroups.  Every GPU
result is read after ``torch.cuda.synchronize()``, which raises if a kernel faulted: a fault fails the test that caused it."""
from __future__ import annotations

import sys
import types

import numpy as np
import pytest
import torch

import meshattrs_cases as cases
import meshraster_cases
from autovfx_amd import hook, meshattrs
from autovfx_amd.meshattrs import (face_areas_normals_backward_host, face_areas_normals_host, interp_face_attrs_backward_host,
                                   interp_face_attrs_host)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32


def _t(a):
    return torch.tensor(np.ascontiguousarray(a), device=DEV)


def _n(*tensors):
    torch.cuda.synchronize()
    out = tuple(t.cpu().numpy() for t in tensors)
    return out if len(out) > 1 else out[0]


def _same_bits(got, want, label):
    assert got.shape == want.shape and got.dtype == want.dtype == F, (label, got.shape, want.shape, got.dtype)
    differ = got.view(np.int32) != want.view(np.int32)
    assert not differ.any(), f"{label}: differs in {int(differ.sum())} of {differ.size} elements, first at {tuple(np.argwhere(differ)[0])}"


def _faces_grads(n_faces, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, n_faces).astype(F), rng.uniform(-1, 1, (n_faces, 3)).astype(F)


def _check_faces(verts, faces, seed, label):
    """Forward bit for bit, backward inside the bound of its terms.  Returns the largest error over the bound."""
    verts, faces = np.asarray(verts, F), np.asarray(faces, np.int64)
    areas, normals = _n(*meshattrs.face_areas_normals_forward(_t(verts), _t(faces)))
    want_areas, want_normals = face_areas_normals_host(verts, faces)
    _same_bits(areas, want_areas, label + ": areas")
    _same_bits(normals, want_normals, label + ": normals")
    ga, gn = _faces_grads(len(faces), seed)
    grad = _n(meshattrs.face_areas_normals_backward(_t(ga), _t(gn), _t(verts), _t(faces)))
    _, parts = face_areas_normals_backward_host(ga, gn, verts, faces)
    valid = ((faces >= 0) & (faces < len(verts))).all(1)
    assert grad.shape == (len(verts), 3) and grad.dtype == F
    return cases.atomic_sum_check(grad, parts[valid].reshape(-1, 3), faces[valid].reshape(-1), len(verts), label + ": grad_verts")


def _check_interp(pix, bary, attrs, grad, label):
    """Forward and grad_bary bit for bit, grad_attrs inside the bound of its terms.  Returns the largest error over the bound."""
    out = _n(meshattrs.interpolate_face_attributes_forward(_t(pix), _t(bary), _t(attrs)))
    _same_bits(out, interp_face_attrs_host(pix, bary, attrs), label + ": pix_attrs")
    grad_bary, grad_attrs = _n(*meshattrs.interpolate_face_attributes_backward(_t(pix), _t(bary), _t(attrs), _t(grad)))
    want_bary, _ = interp_face_attrs_backward_host(pix, bary, attrs, grad)
    _same_bits(grad_bary, want_bary, label + ": grad_bary")
    flat = pix.reshape(-1)
    held = (flat >= 0) & (flat < len(attrs))
    terms = bary.reshape(-1, 3)[held][:, :, None] * grad.reshape(len(flat), -1)[held][:, None, :]        # fp32 products, as the contract's
    assert grad_attrs.shape == attrs.shape and grad_attrs.dtype == F
    return cases.atomic_sum_check(grad_attrs, terms, flat[held], len(attrs), label + ": grad_attrs")


# ---- bit equality with the restatement ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_faces", [1, 63, 64, 65, 256, 257, 1000])
def test_faces_equal_the_restatement(n_faces):
    verts, faces = cases.random_mesh(max(3, n_faces // 2 + 3), n_faces, seed=n_faces)
    _check_faces(verts, faces, n_faces, f"F = {n_faces}")


# flat [P], as pytorch3d's interpolate_face_attributes hands the fragments over, and [N, H, W, K]
SLOT_SHAPES = [(1,), (63,), (64,), (65,), (256,), (257,), (1000,), (1, 25, 40, 1), (1, 25, 40, 10), (10000,)]
FACE_COUNTS = [1, 63, 64, 65, 256, 257, 1000]


@pytest.mark.parametrize("shape", SLOT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_interpolation_equals_the_restatement(shape):
    """About a third of the slots empty; 256 slots are one workgroup, 257 two; D = 48 takes 48 rounds of a workgroup's loop."""
    for i, D in enumerate((1, 2, 3, 5, 48)):
        n_faces = FACE_COUNTS[(i + SLOT_SHAPES.index(shape)) % len(FACE_COUNTS)]
        pix, bary, attrs, grad = cases.fragments(shape, n_faces, D, seed=1000 * D + int(np.prod(shape)))
        if pix.size > 2:
            assert (pix < 0).any() and (pix >= 0).any()
        _check_interp(pix, bary, attrs, grad, f"P = {pix.size}, F = {n_faces}, D = {D}")


# ---- the atomically summed outputs where many lanes meet ------------------------------------------------------------------------------

def test_a_closed_mesh_of_valence_six():
    verts, faces = cases.torus(20, 15, seed=5)
    assert (np.bincount(faces.reshape(-1)) == 6).all()
    worst = _check_faces(verts, faces, 5, "torus")
    print(f"torus: grad_verts at most {worst:.3f} of the bound")


def test_one_vertex_in_a_thousand_faces():
    verts, faces = cases.fan(1000, seed=6)
    assert np.bincount(faces.reshape(-1))[0] == 1000
    worst = _check_faces(verts, faces, 6, "fan")
    print(f"fan: grad_verts at most {worst:.3f} of the bound")


def test_one_face_under_five_thousand_slots():
    pix, bary, attrs, grad = cases.fragments((1, 50, 100, 1), 7, 3, seed=7, empty=0.0)
    pix[...] = 2
    pix[0, ::7, ::5, 0] = 5                                           # a few elsewhere: one term (bit-equal), several terms
    pix[0, 0, 0, 0] = 0
    worst = _check_interp(pix, bary, attrs, grad, "one face, D = 3")
    pix, bary, attrs, grad = cases.fragments((1, 50, 100, 1), 3, 48, seed=8, empty=0.0)
    pix[...] = 1
    worst = max(worst, _check_interp(pix, bary, attrs, grad, "one face, D = 48"))
    print(f"one face under 5000 slots: grad_attrs at most {worst:.3f} of the bound")


def test_unreferenced_vertices_and_vertices_in_one_face():
    verts, faces = cases.random_mesh(60, 12, seed=9)
    count = np.bincount(faces.reshape(-1), minlength=60)
    assert (count == 0).any() and (count == 1).any() and (count >= 2).any()
    _check_faces(verts, faces, 9, "sparse mesh")
    verts, faces = cases.torus(8, 8, seed=10)
    _check_faces(np.concatenate((verts, np.full((300, 3), 3.0, F))), faces, 10, "torus and 300 vertices in no face")


# ---- edge cases -----------------------------------------------------------------------------------------------------------------------

def test_degenerate_faces_among_normal_ones():
    """Zero area (collinear and coincident vertices) and n on both sides of 1e-6: 0.9e-6 takes the linear branch, 1.1e-6 the projected."""
    verts, faces = cases.random_mesh(40, 70, seed=11)
    extra = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2], [1e-3, 0, 0], [0, 0.9e-3, 0], [0, 1.1e-3, 0], [0.5, 0.5, 0.5]], F)
    at = len(verts)
    odd = np.array([[at, at + 1, at + 2], [at + 6, at + 6, at + 6], [at, at + 3, at + 4], [at, at + 3, at + 5], [3, 3, 7]], np.int64)
    faces = np.concatenate((faces[:30], odd[:3], faces[30:], odd[3:]))
    verts = np.concatenate((verts, extra))
    areas, _ = face_areas_normals_host(verts, faces)
    n = 2 * areas[[30, 31, 32, 73, 74]]
    assert n[0] == 0 and n[1] == 0 and 0 < n[2] < 1e-6 < n[3] and n[4] == 0
    _check_faces(verts, faces, 11, "degenerate faces")


def test_out_of_range_indices_among_valid_ones():
    """The valid ones come out as if the others were absent, and nothing faults."""
    verts, faces = cases.random_mesh(50, 200, seed=12)
    bad = np.array([[0, 1, 50], [-1, 2, 3], [4, 5, 1 << 40], [-(1 << 62), 0, 0], [(1 << 31), 1, 2]], np.int64)
    at = np.array([0, 63, 64, 130, 204])
    mixed = np.insert(faces, at - np.arange(5), bad, axis=0)
    valid = np.ones(len(mixed), bool)
    valid[at] = False
    assert np.array_equal(mixed[valid], faces) and np.array_equal(mixed[~valid], bad)
    _check_faces(verts, mixed, 12, "out-of-range faces")
    areas, normals = _n(*meshattrs.face_areas_normals_forward(_t(verts), _t(mixed)))
    alone_areas, alone_normals = _n(*meshattrs.face_areas_normals_forward(_t(verts), _t(faces)))
    _same_bits(areas[valid], alone_areas, "areas of the valid faces")
    _same_bits(normals[valid], alone_normals, "normals of the valid faces")
    assert not areas[~valid].any() and not normals[~valid].any()

    pix, bary, attrs, grad = cases.fragments((1, 30, 20, 2), 40, 3, seed=13)
    wild = pix.copy()
    rng = np.random.default_rng(14)
    where = rng.uniform(size=pix.shape) < 0.2
    wild[where] = rng.choice(np.array([40, 41, 1 << 31, 1 << 40, -2, -(1 << 62)], np.int64), int(where.sum()))
    _check_interp(wild, bary, attrs, grad, "out-of-range slots")
    emptied = np.where(where, -1, pix)
    out = _n(meshattrs.interpolate_face_attributes_forward(_t(wild), _t(bary), _t(attrs)))
    _same_bits(out, _n(meshattrs.interpolate_face_attributes_forward(_t(emptied), _t(bary), _t(attrs))), "as if empty")
    got = _n(*meshattrs.interpolate_face_attributes_backward(_t(wild), _t(bary), _t(attrs), _t(grad)))
    want = _n(*meshattrs.interpolate_face_attributes_backward(_t(emptied), _t(bary), _t(attrs), _t(grad)))
    _same_bits(got[0], want[0], "grad_bary as if empty")
    assert np.abs(got[1] - want[1]).max() <= 1e-5                    # (two atomic sums of the same terms; the bound itself is checked above)


def test_nothing_to_do():
    verts = _t(np.ones((5, 3), F))
    none = torch.zeros((0, 3), dtype=torch.int64, device=DEV)
    areas, normals = meshattrs.face_areas_normals_forward(verts, none)
    assert areas.shape == (0,) and normals.shape == (0, 3)
    grad = _n(meshattrs.face_areas_normals_backward(torch.zeros(0, device=DEV), torch.zeros((0, 3), device=DEV), verts, none))
    assert grad.shape == (5, 3) and not grad.any()                   # V with no faces: zeros, written
    no_verts = torch.zeros((0, 3), device=DEV)
    areas, normals = _n(*meshattrs.face_areas_normals_forward(no_verts, _t(np.array([[0, 1, 2]], np.int64))))
    assert areas.tolist() == [0.0] and not normals.any()
    assert meshattrs.face_areas_normals_backward(_t(np.ones(1, F)), _t(np.ones((1, 3), F)), no_verts, _t(np.array([[0, 1, 2]], np.int64))).shape == (0, 3)

    attrs = _t(np.ones((4, 3, 2), F))
    pix, bary = torch.zeros((1, 0, 3, 2), dtype=torch.int64, device=DEV), torch.zeros((1, 0, 3, 2, 3), device=DEV)
    assert meshattrs.interpolate_face_attributes_forward(pix, bary, attrs).shape == (1, 0, 3, 2, 2)
    grad_bary, grad_attrs = meshattrs.interpolate_face_attributes_backward(pix, bary, attrs, torch.zeros((1, 0, 3, 2, 2), device=DEV))
    assert grad_bary.shape == (1, 0, 3, 2, 3) and grad_attrs.shape == (4, 3, 2) and not _n(grad_attrs).any()       # P == 0: zeros, written
    no_attrs = torch.zeros((0, 3, 2), device=DEV)
    pix, bary = torch.zeros((1, 2, 3, 1), dtype=torch.int64, device=DEV), torch.ones((1, 2, 3, 1, 3), device=DEV)
    assert not _n(meshattrs.interpolate_face_attributes_forward(pix, bary, no_attrs)).any()
    grad_bary, grad_attrs = meshattrs.interpolate_face_attributes_backward(pix, bary, no_attrs, torch.ones((1, 2, 3, 1, 2), device=DEV))
    assert not _n(grad_bary).any() and grad_attrs.shape == (0, 3, 2)


def test_non_contiguous_inputs_are_copied():
    verts, faces = cases.torus(9, 7, seed=15)
    ga, gn = _faces_grads(len(faces), 15)
    wide = torch.zeros((len(verts), 6), device=DEV)
    wide[:, ::2] = _t(verts)
    strided_verts, strided_faces = wide[:, ::2], _t(faces.T.copy()).t()
    strided_gn = _t(gn.T.copy()).t()
    assert not strided_verts.is_contiguous() and not strided_faces.is_contiguous() and not strided_gn.is_contiguous()
    got = _n(*meshattrs.face_areas_normals_forward(strided_verts, strided_faces))
    want = face_areas_normals_host(verts, faces)
    _same_bits(got[0], want[0], "areas")
    _same_bits(got[1], want[1], "normals")
    grad = _n(meshattrs.face_areas_normals_backward(_t(np.repeat(ga, 2))[::2], strided_gn, strided_verts, strided_faces))
    _, parts = face_areas_normals_backward_host(ga, gn, verts, faces)
    cases.atomic_sum_check(grad, parts.reshape(-1, 3), faces.reshape(-1), len(verts), "strided grad_verts")

    pix, bary, attrs, grad_out = cases.fragments((2, 6, 7, 3), 30, 5, seed=16)
    s_pix = _t(pix.transpose(0, 2, 1, 3).copy()).permute(0, 2, 1, 3)
    s_bary = _t(bary.transpose(0, 2, 1, 3, 4).copy()).permute(0, 2, 1, 3, 4)
    s_attrs = _t(attrs.transpose(2, 0, 1).copy()).permute(1, 2, 0)
    s_grad = _t(grad_out.transpose(4, 0, 1, 2, 3).copy()).permute(1, 2, 3, 4, 0)
    assert not any(t.is_contiguous() for t in (s_pix, s_bary, s_attrs, s_grad))
    _same_bits(_n(meshattrs.interpolate_face_attributes_forward(s_pix, s_bary, s_attrs)), interp_face_attrs_host(pix, bary, attrs), "pix_attrs")
    grad_bary, grad_attrs = _n(*meshattrs.interpolate_face_attributes_backward(s_pix, s_bary, s_attrs, s_grad))
    _same_bits(grad_bary, interp_face_attrs_backward_host(pix, bary, attrs, grad_out)[0], "grad_bary")
    held = pix.reshape(-1) >= 0
    terms = bary.reshape(-1, 3)[held][:, :, None] * grad_out.reshape(-1, 5)[held][:, None, :]
    cases.atomic_sum_check(grad_attrs, terms, pix.reshape(-1)[held], 30, "strided grad_attrs")


def test_on_a_stream_of_its_own():
    verts, faces = cases.torus(11, 9, seed=17)
    pix, bary, attrs, grad = cases.fragments((1, 30, 31, 2), 50, 3, seed=18)
    stream = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        assert torch.cuda.current_stream(DEV) == stream
        worst = _check_faces(verts, faces, 17, "stream")
        worst = max(worst, _check_interp(pix, bary, attrs, grad, "stream"))
    assert worst <= 1


def test_every_output_element_is_written():
    """The C entry points on outputs prefilled with 0xFF bytes (a NaN): no element keeps them, at sizes with part-filled workgroups."""
    from autovfx_amd import _lib

    def prefilled(*shape):
        return torch.full(shape, 255, dtype=torch.uint8, device=DEV).view(torch.float32).reshape(*shape[:-1], shape[-1] // 4)

    nan_bits = np.int32(-1)
    for n_faces in (1, 257, 1000):
        verts, faces = cases.random_mesh(80, n_faces, seed=19 + n_faces)
        faces[::9, 1] = 80                                            # invalid faces are written too
        ga, gn = _faces_grads(n_faces, 19)
        v, f, tga, tgn = _t(verts), _t(faces), _t(ga), _t(gn)
        areas, normals, grad = prefilled(n_faces * 4), prefilled(n_faces, 12), prefilled(80 + 20, 12)
        _lib.call("gsr_face_areas_normals", 80, n_faces, v.data_ptr(), f.data_ptr(), areas.data_ptr(), normals.data_ptr(), device=v.device)
        _lib.call("gsr_face_areas_normals_backward", 80, n_faces, v.data_ptr(), f.data_ptr(), tga.data_ptr(), tgn.data_ptr(), grad.data_ptr(),
                  device=v.device)
        areas, normals, grad = _n(areas, normals, grad)
        want = face_areas_normals_host(verts, faces)
        _same_bits(areas, want[0], "areas")
        _same_bits(normals, want[1], "normals")
        assert not (grad[:80].view(np.int32) == nan_bits).any() and (grad[80:].view(np.int32) == nan_bits).all()      # V rows, not one more
    for shape, D in (((1, 1, 1, 1), 1), ((1, 1, 257, 1), 3), ((1, 25, 40, 10), 2), ((1, 7, 11, 3), 48)):
        pix, bary, attrs, grad_out = cases.fragments(shape, 33, D, seed=20 + D)
        P = pix.size
        out, grad_bary, grad_attrs = prefilled(P + 1, 4 * D), prefilled(P + 1, 12), prefilled(33 + 1, 3, 4 * D)
        tensors = [_t(a) for a in (pix, bary, attrs, grad_out)]
        p, w, a, g = (t.data_ptr() for t in tensors)
        _lib.call("gsr_interp_face_attrs", P, 33, D, p, w, a, out.data_ptr(), device=out.device)
        _lib.call("gsr_interp_face_attrs_backward", P, 33, D, p, w, a, g, grad_bary.data_ptr(), grad_attrs.data_ptr(), device=out.device)
        out, grad_bary, grad_attrs = _n(out, grad_bary, grad_attrs)
        _same_bits(out[:P].reshape(shape + (D,)), interp_face_attrs_host(pix, bary, attrs), "pix_attrs")
        _same_bits(grad_bary[:P].reshape(shape + (3,)), interp_face_attrs_backward_host(pix, bary, attrs, grad_out)[0], "grad_bary")
        assert not (grad_attrs[:33].view(np.int32) == nan_bits).any()
        for tail in (out[P:], grad_bary[P:], grad_attrs[33:]):
            assert (tail.view(np.int32) == nan_bits).all()               # and nothing past the end


# ---- end to end -----------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def hooked_pytorch3d():
    """A stub ``pytorch3d._C`` whose six operators have no GPU code, under ``install()``."""
    names = ("pytorch3d", "pytorch3d._C")
    saved = {k: sys.modules.pop(k) for k in names if k in sys.modules}
    root, leaf = (types.ModuleType(n) for n in names)

    def no_gpu_code(*_args):
        raise RuntimeError("Not compiled with GPU support")

    for name in ("rasterize_meshes", "rasterize_meshes_backward", "face_areas_normals_forward", "face_areas_normals_backward",
                 "interpolate_face_attributes_forward", "interpolate_face_attributes_backward"):
        setattr(leaf, name, no_gpu_code)
    root._C = leaf
    sys.modules.update(zip(names, (root, leaf)))
    path = list(sys.path)
    try:
        hook.install(path=False)
        yield root
    finally:
        hook.uninstall()
        sys.path[:] = path
        for k in names:
            sys.modules.pop(k, None)
        sys.modules.update(saved)


def _autograd_classes(pytorch3d):
    """pytorch3d's ``_MeshFaceAreasNormals`` and ``_InterpFaceAttrs`` in outline: the operators are looked up on ``_C`` at call time."""
    class FaceAreasNormals(torch.autograd.Function):
        @staticmethod
        def forward(ctx, verts, faces):
            ctx.save_for_backward(verts, faces)
            return pytorch3d._C.face_areas_normals_forward(verts, faces)

        @staticmethod
        def backward(ctx, grad_areas, grad_normals):
            verts, faces = ctx.saved_tensors
            return pytorch3d._C.face_areas_normals_backward(grad_areas.contiguous(), grad_normals.contiguous(), verts, faces), None

    class InterpFaceAttrs(torch.autograd.Function):
        @staticmethod
        def forward(ctx, pix_to_face, bary, attrs):
            ctx.save_for_backward(pix_to_face, bary, attrs)
            return pytorch3d._C.interpolate_face_attributes_forward(pix_to_face, bary, attrs)

        @staticmethod
        def backward(ctx, grad_out):
            pix_to_face, bary, attrs = ctx.saved_tensors
            grad_bary, grad_attrs = pytorch3d._C.interpolate_face_attributes_backward(pix_to_face, bary, attrs, grad_out)
            return None, grad_bary, grad_attrs

    return FaceAreasNormals, InterpFaceAttrs


def test_gradients_through_the_hooked_operators(hooked_pytorch3d):
    FaceAreasNormals, InterpFaceAttrs = _autograd_classes(hooked_pytorch3d)
    verts, faces = cases.torus(14, 10, seed=21)
    weights = _t(np.random.default_rng(22).uniform(-1, 1, (len(faces), 3)).astype(F))
    v = _t(verts).requires_grad_(True)
    areas, normals = FaceAreasNormals.apply(v, _t(faces))
    normals.retain_grad()
    areas.retain_grad()
    loss = (torch.nn.functional.normalize(normals, dim=-1) * weights).sum() + (areas * areas).sum()
    loss.backward()
    want_areas, want_normals = face_areas_normals_host(verts, faces)
    _same_bits(_n(areas.detach()), want_areas, "areas")
    _same_bits(_n(normals.detach()), want_normals, "normals")
    _, parts = face_areas_normals_backward_host(_n(areas.grad), _n(normals.grad), verts, faces)
    cases.atomic_sum_check(_n(v.grad), parts.reshape(-1, 3), faces.reshape(-1), len(verts), "grad_verts through normalize")

    pix, bary, attrs, _ = cases.fragments((1, 20, 30, 4), 60, 3, seed=23)
    w, a = _t(bary).requires_grad_(True), _t(attrs).requires_grad_(True)
    out = InterpFaceAttrs.apply(_t(pix).view(-1), w.view(-1, 3), a).view(1, 20, 30, 4, 3)       # flattened, as pytorch3d's Python does
    out.retain_grad()
    (out * out).sum().backward()
    _same_bits(_n(out.detach()), interp_face_attrs_host(pix, bary, attrs), "pix_attrs")
    grad_out = _n(out.grad)
    _same_bits(_n(w.grad), interp_face_attrs_backward_host(pix, bary, attrs, grad_out)[0], "grad_bary")
    held = pix.reshape(-1) >= 0
    terms = bary.reshape(-1, 3)[held][:, :, None] * grad_out.reshape(-1, 3)[held][:, None, :]
    cases.atomic_sum_check(_n(a.grad), terms, pix.reshape(-1)[held], 60, "grad_attrs through the square")


def test_the_z_buffers_fragments_interpolate_back_to_zbuf(hooked_pytorch3d):
    """With ``perspective_correct`` and the clip off, ``zbuf`` is the interpolation of the three vertex depths by the barycentrics the
    rasterizer returns: the face vertices as attributes reproduce it in z (the same three products and two sums; 2 ulp allowed)."""
    H, W, n_faces, seed = meshraster_cases.SCENES[0]
    fv = meshraster_cases.scene(n_faces, seed)
    first, num, nbr = meshraster_cases.one_mesh(fv)
    C = hooked_pytorch3d._C
    pix, zbuf, bary, _ = C.rasterize_meshes(_t(fv), _t(first), _t(num), _t(nbr), (H, W), 0.0, 4, None, 50_000, False, False, False)
    out = C.interpolate_face_attributes_forward(pix, bary, _t(fv))
    pix, zbuf, out = _n(pix, zbuf, out)
    held = pix >= 0
    assert held.sum() > H * W and out.shape == (1, H, W, 4, 3) and not out[~held].any()
    z, want = out[..., 2][held], zbuf[held]
    assert np.all(np.abs(z.astype(np.float64) - want) <= 2 * np.spacing(np.abs(want)))
