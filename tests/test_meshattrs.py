"""autovfx_amd.meshattrs without a GPU: the numpy restatements of the contract against float64 truths and on exact cases, which calls the
kernels take, the hook's rows for ``pytorch3d._C``, and the C ABI's refusals."""
from __future__ import annotations

import importlib
import sys
import types

import numpy as np
import pytest
import torch

import meshattrs_cases as cases
from autovfx_amd import hook, meshattrs
from autovfx_amd.meshattrs import (face_areas_normals_backward_host, face_areas_normals_host, interp_face_attrs_backward_host,
                                   interp_face_attrs_host)
from helpers import OnOtherGpu as _OnOtherGpu, fake_gpu as _gpu

F = np.float32
OPERATORS = ("face_areas_normals_forward", "face_areas_normals_backward", "interpolate_face_attributes_forward",
             "interpolate_face_attributes_backward")


def _ulps(got, truth):
    """The largest ``|got - truth|`` in units of the fp32 spacing at ``|truth|``, element by element."""
    unit = np.spacing(np.abs(truth).astype(F)).astype(np.float64)
    return float((np.abs(got.astype(np.float64) - truth) / unit).max())


# ---- the restatements against the float64 truth -------------------------------------------------------------------------------------

# Vertices on a grid of 2^-12: the edge vectors a and b are then exact, and what is left is the rounding of the contract's own operations.
TRUTH_MESHES = [cases.torus(12, 9, seed=1, grid=2.0 ** -12), cases.torus(31, 17, seed=2, grid=2.0 ** -12)]


@pytest.mark.parametrize("index", range(len(TRUTH_MESHES)))
def test_face_forward_restatement_against_truth(index):
    """4 ulp per element, each element of the areas and of the normals held to the fp32 spacing at its own float64 value."""
    verts, faces = TRUTH_MESHES[index]
    rng = np.random.default_rng(index)
    areas64, normals64, _ = cases.faces_gradients_torch(verts, faces, rng.uniform(-1, 1, len(faces)).astype(F),
                                                        rng.uniform(-1, 1, (len(faces), 3)).astype(F), torch.float64)
    areas, normals = face_areas_normals_host(verts, faces)
    assert areas.dtype == F and normals.dtype == F and areas.shape == (len(faces),) and normals.shape == (len(faces), 3)
    ea, en = _ulps(areas, areas64), _ulps(normals, normals64)
    print(f"mesh {index}: areas {ea:.2f} ulp, normals {en:.2f} ulp")
    assert ea <= 4 and en <= 4


@pytest.mark.parametrize("index", range(len(TRUTH_MESHES)))
def test_face_backward_restatement_against_truth(index):
    """No bar fixed in advance: torch's own fp32 CPU autograd of the same forward, against the same float64 truth and in units of the sum
    of the absolute products (cases.faces_gradient_scale), is the measure; the restatement rounds in another order but does the same
    number of operations, and may be at most 4 x that.  Every face has n >= 1e-3, so the clamp is in no one's path."""
    verts, faces = TRUTH_MESHES[index]
    rng = np.random.default_rng(10 + index)
    ga, gn = rng.uniform(-1, 1, len(faces)).astype(F), rng.uniform(-1, 1, (len(faces), 3)).astype(F)
    areas64, _, truth = cases.faces_gradients_torch(verts, faces, ga, gn, torch.float64)
    assert (2 * areas64).min() >= 1e-3
    _, _, torch32 = cases.faces_gradients_torch(verts, faces, ga, gn, torch.float32)
    got, contributions = face_areas_normals_backward_host(ga, gn, verts, faces)
    assert got.dtype == F and contributions.shape == (len(faces), 3, 3)
    scale = cases.faces_gradient_scale(verts, faces, ga, gn)
    e_torch, e_ours = cases.relative_to(scale, torch32, truth), cases.relative_to(scale, got, truth)
    print(f"mesh {index}: grad_verts, torch fp32 autograd {e_torch:.3e}, restatement {e_ours:.3e} of the scale")
    assert 0 < e_torch and e_ours <= 4 * e_torch
    # the contributions are what the sum is made of
    again = np.zeros_like(got)
    np.add.at(again, faces.reshape(-1), contributions.reshape(-1, 3))
    assert np.array_equal(again, got)


@pytest.mark.parametrize("D", [1, 3, 48])
def test_interp_restatements_against_truth(D):
    """The forward within 4 ulp of each element on non-negative barycentrics and attributes (UVs, colours: no term cancels another, so an
    element's own spacing is the unit); the backward, on signed attributes, at most 4 x the error of torch's fp32 autograd in units of the
    sum of the absolute products."""
    shape = (1, 9, 11, 3)
    pix, bary, attrs, grad = cases.fragments(shape, 40, D, seed=D, signed=False)
    truth, _, _ = cases.interp_gradients_torch(pix, bary, attrs, grad, torch.float64)
    out = interp_face_attrs_host(pix, bary, attrs)
    assert out.dtype == F and out.shape == shape + (D,) and np.all(out[pix < 0] == 0) and (pix < 0).any() and (pix >= 0).any()
    e = _ulps(out, truth)
    print(f"D = {D}: forward {e:.2f} ulp")
    assert e <= 4

    pix, bary, attrs, grad = cases.fragments(shape, 40, D, seed=100 + D)
    _, bary64, attrs64 = cases.interp_gradients_torch(pix, bary, attrs, grad, torch.float64)
    _, bary32, attrs32 = cases.interp_gradients_torch(pix, bary, attrs, grad, torch.float32)
    got_bary, got_attrs = interp_face_attrs_backward_host(pix, bary, attrs, grad)
    assert got_bary.shape == shape + (3,) and got_attrs.shape == attrs.shape and got_bary.dtype == F and got_attrs.dtype == F
    scale_bary, scale_attrs = cases.interp_gradient_scales(pix, bary, attrs, grad)
    for name, scale, t32, ours, t64 in (("grad_bary", scale_bary, bary32, got_bary, bary64), ("grad_attrs", scale_attrs, attrs32, got_attrs, attrs64)):
        e_torch, e_ours = cases.relative_to(scale, t32, t64), cases.relative_to(scale, ours, t64)
        print(f"D = {D}: {name}, torch fp32 autograd {e_torch:.3e}, restatement {e_ours:.3e} of the scale")
        assert 0 < e_torch and e_ours <= 4 * e_torch


# ---- exact cases ----------------------------------------------------------------------------------------------------------------------

def test_a_right_triangle():
    areas, normals = face_areas_normals_host([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 2]])
    assert areas.tolist() == [0.5] and normals.tolist() == [[0.0, 0.0, 1.0]]
    areas, normals = face_areas_normals_host([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 2, 1]])
    assert areas.tolist() == [0.5] and normals.tolist() == [[0.0, 0.0, -1.0]]
    # d area / d v1 along x is half the height: the contributions, and their sum to zero over the face
    grad, parts = face_areas_normals_backward_host([1.0], [[0, 0, 0]], [[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 2]])
    assert grad.tolist() == [[-0.5, -0.5, 0.0], [0.5, 0.0, 0.0], [0.0, 0.5, 0.0]] and np.array_equal(parts[0], grad)


def test_a_zero_area_face():
    verts = [[0, 0, 0], [1, 1, 1], [2, 2, 2], [5, 5, 5]]
    areas, normals = face_areas_normals_host(verts, [[0, 1, 2], [3, 3, 3]])
    assert areas.tolist() == [0.0, 0.0] and not normals.any()
    grad, parts = face_areas_normals_backward_host([3.0, 3.0], np.zeros((2, 3), F), verts, [[0, 1, 2], [3, 3, 3]])
    assert not grad.any() and not parts.any()                        # nothing through the area at n == 0
    # through the normal the linear branch applies: c / 1e-6, so d normal / d c = 1 / 1e-6
    grad, parts = face_areas_normals_backward_host([0.0], [[0, 0, 1]], [[0, 0, 0], [1, 0, 0], [2, 0, 0]], [[0, 1, 2]])
    inv = F(1.0) / F(1e-6)
    # g_c = (0, 0, inv); g_a = b x g_c = (b.y inv, -b.x inv, 0) = (0, -2 inv, 0); g_b = g_c x a = (-inv a.y, inv a.x, 0) = (0, inv, 0)
    assert np.array_equal(parts[0], np.array([[0, F(2) * inv - inv, 0], [0, -F(2) * inv, 0], [0, inv, 0]], F))


def test_both_sides_of_the_clamp():
    """n just below 1e-6: normal = c / 1e-6 and the linear backward; just above: c / n and the projected backward."""
    def tri(h):
        return np.array([[0, 0, 0], [1e-3, 0, 0], [0, h, 0]], F)

    eps = F(1e-6)
    for h, below in ((F(0.9e-3), True), (F(1.1e-3), False)):
        verts = tri(h)
        n = verts[1, 0] * verts[2, 1]                                  # c = (0, 0, a.x b.y) exactly as the contract computes it
        assert (n < eps) == below
        areas, normals = face_areas_normals_host(verts, [[0, 1, 2]])
        assert areas[0] == n / F(2) and np.array_equal(normals[0], np.array([0, 0, n / (eps if below else n)], F))
        g = np.array([[0.25, -0.5, 2.0]], F)
        _, parts = face_areas_normals_backward_host([0.0], g, verts, [[0, 1, 2]])
        if below:
            gc = g[0] / eps
        else:                                                           # m = (0, 0, 1): the projection removes g.z
            gc = np.array([g[0, 0] / n, g[0, 1] / n, (g[0, 2] - F(1.0) * g[0, 2]) / n], F)
        a, b = verts[1] - verts[0], verts[2] - verts[0]
        g_a = np.array([b[1] * gc[2] - b[2] * gc[1], b[2] * gc[0] - b[0] * gc[2], b[0] * gc[1] - b[1] * gc[0]], F)
        g_b = np.array([gc[1] * a[2] - gc[2] * a[1], gc[2] * a[0] - gc[0] * a[2], gc[0] * a[1] - gc[1] * a[0]], F)
        assert np.array_equal(parts[0], np.stack((-(g_a + g_b), g_a, g_b)))
        assert (parts[0, 1, 0] != 0) == below                          # g_a.x = b.y g_c.z: only the linear branch lets g.z through


def test_out_of_range_faces_and_unreferenced_vertices():
    verts, faces = cases.random_mesh(9, 6, seed=3)
    verts = np.concatenate((verts, [[7, 7, 7], [np.nan, np.inf, 1]])).astype(F)     # vertices 9 and 10 are in no face
    bad = np.array([[0, 1, 11], [-1, 2, 3], [4, 5, 1 << 40]], np.int64)
    mixed = np.concatenate((faces[:3], bad[:2], faces[3:], bad[2:]))
    valid = np.array([True] * 3 + [False] * 2 + [True] * 3 + [False])
    areas, normals = face_areas_normals_host(verts, mixed)
    want_a, want_n = face_areas_normals_host(verts, faces)
    assert np.array_equal(areas[valid], want_a) and np.array_equal(normals[valid], want_n) and not areas[~valid].any() and not normals[~valid].any()
    rng = np.random.default_rng(4)
    ga, gn = rng.uniform(-1, 1, len(mixed)).astype(F), rng.uniform(-1, 1, (len(mixed), 3)).astype(F)
    grad, parts = face_areas_normals_backward_host(ga, gn, verts, mixed)
    want, _ = face_areas_normals_backward_host(ga[valid], gn[valid], verts, faces)
    assert np.array_equal(grad, want) and not parts[~valid].any()
    assert not grad[9:].any() and grad[np.unique(faces)].all()       # a vertex in no face gets exactly zero
    # no faces, no vertices
    assert [x.shape for x in face_areas_normals_host(verts, np.zeros((0, 3), np.int64))] == [(0,), (0, 3)]
    assert not face_areas_normals_backward_host(np.zeros(0, F), np.zeros((0, 3), F), verts, np.zeros((0, 3), np.int64))[0].any()
    areas, normals = face_areas_normals_host(np.zeros((0, 3), F), [[0, 0, 0]])
    assert areas.tolist() == [0.0] and not normals.any()


def test_empty_slots_and_faces_past_the_end():
    attrs = np.arange(2 * 3 * 2, dtype=F).reshape(2, 3, 2)
    pix = np.array([[[[0, -1, 1, 2, -7]]]], np.int64)                # face 2 does not exist: treated as empty
    bary = np.tile(np.array([0.5, 0.25, 0.25], F), (1, 1, 1, 5, 1))
    out = interp_face_attrs_host(pix, bary, attrs)
    assert out[0, 0, 0].tolist() == [[1.5, 2.5], [0, 0], [7.5, 8.5], [0, 0], [0, 0]]
    grad = np.ones((1, 1, 1, 5, 2), F)
    grad_bary, grad_attrs = interp_face_attrs_backward_host(pix, bary, attrs, grad)
    assert grad_bary[0, 0, 0].tolist() == [[1, 5, 9], [0, 0, 0], [13, 17, 21], [0, 0, 0], [0, 0, 0]]
    assert np.array_equal(grad_attrs, np.broadcast_to(np.array([0.5, 0.25, 0.25], F)[None, :, None], (2, 3, 2)))
    # no slots, no faces
    assert interp_face_attrs_host(np.zeros((1, 0, 4, 1), np.int64), np.zeros((1, 0, 4, 1, 3), F), attrs).shape == (1, 0, 4, 1, 2)
    out = interp_face_attrs_host(np.zeros((1, 1, 1, 1), np.int64), np.ones((1, 1, 1, 1, 3), F), np.zeros((0, 3, 4), F))
    assert out.shape == (1, 1, 1, 1, 4) and not out.any()


# ---- which calls the kernels take ---------------------------------------------------------------------------------------------------

def _faces_call(**over):
    args = dict(grad_areas=_gpu(5), grad_normals=_gpu(5, 3), verts=_gpu(7, 3), faces=_gpu(5, 3, dtype=torch.int64))
    assert set(over) <= set(args)
    args.update(over)
    return tuple(args.values())


def _interp_call(**over):
    args = dict(pix_to_face=_gpu(2, 4, 6, 3, dtype=torch.int64), bary=_gpu(2, 4, 6, 3, 3), attrs=_gpu(9, 3, 5), grad=_gpu(2, 4, 6, 3, 5))
    assert set(over) <= set(args)
    args.update(over)
    return tuple(args.values())


def test_which_calls_the_kernels_take():
    assert meshattrs.face_areas_normals_takes(*_faces_call()[2:]) and meshattrs.face_areas_normals_backward_takes(*_faces_call())
    assert meshattrs.face_areas_normals_takes(_gpu(0, 3), _gpu(0, 3, dtype=torch.int64))
    assert meshattrs.face_areas_normals_takes(_gpu(3, 7).t(), _gpu(3, 5, dtype=torch.int64).t())          # non-contiguous: copied, not refused
    refused = dict(
        verts=[torch.zeros(7, 3), _gpu(7, 3, dtype=torch.float64), _gpu(7, 3, dtype=torch.float16), _gpu(7), _gpu(7, 2), _gpu(7, 3, 1), np.zeros((7, 3), F)],
        faces=[torch.zeros(5, 3, dtype=torch.int64), _gpu(5, 3, dtype=torch.int32), _gpu(5, 3), _gpu(5, 4, dtype=torch.int64), _gpu(15, dtype=torch.int64),
               _gpu(5, 3, dtype=torch.int64, cls=_OnOtherGpu)],
        grad_areas=[torch.zeros(5), _gpu(4), _gpu(5, 1), _gpu(5, dtype=torch.float64), _gpu(5, cls=_OnOtherGpu)],
        grad_normals=[torch.zeros(5, 3), _gpu(5), _gpu(4, 3), _gpu(5, 3, dtype=torch.float64), None],
    )
    for name, values in refused.items():
        for value in values:
            call = _faces_call(**{name: value})
            assert not meshattrs.face_areas_normals_backward_takes(*call), (name, value)
            if name in ("verts", "faces"):
                assert not meshattrs.face_areas_normals_takes(*call[2:]), (name, value)
    for over, word in ((dict(verts=torch.zeros(7, 3)), "GPU"), (dict(verts=_gpu(7, 3, dtype=torch.float64)), "float32"),
                       (dict(faces=_gpu(5, 3, dtype=torch.int32)), "int64"), (dict(faces=_gpu(5, 2, dtype=torch.int64)), r"\[F, 3\]"),
                       (dict(faces=_gpu(5, 3, dtype=torch.int64, cls=_OnOtherGpu)), "cuda:0")):
        with pytest.raises(ValueError, match=word):
            meshattrs.face_areas_normals_forward(*_faces_call(**over)[2:])
        with pytest.raises(ValueError, match=word):
            meshattrs.face_areas_normals_backward(*_faces_call(**over))
    with pytest.raises(ValueError, match="grad_areas"):
        meshattrs.face_areas_normals_backward(*_faces_call(grad_areas=_gpu(4)))

    assert meshattrs.interpolate_face_attributes_takes(*_interp_call()[:3]) and meshattrs.interpolate_face_attributes_backward_takes(*_interp_call())
    assert meshattrs.interpolate_face_attributes_takes(_gpu(1, 0, 4, 1, dtype=torch.int64), _gpu(1, 0, 4, 1, 3), _gpu(0, 3, 1))
    flat = (_gpu(144, dtype=torch.int64), _gpu(144, 3), _gpu(9, 3, 5), _gpu(144, 5))             # as pytorch3d's Python flattens the fragments
    assert meshattrs.interpolate_face_attributes_takes(*flat[:3]) and meshattrs.interpolate_face_attributes_backward_takes(*flat)
    assert not meshattrs.interpolate_face_attributes_takes(_gpu((), dtype=torch.int64), _gpu(3), _gpu(9, 3, 5))
    refused = dict(
        pix_to_face=[torch.zeros(2, 4, 6, 3, dtype=torch.int64), _gpu(2, 4, 6, 3, dtype=torch.int32), _gpu(2, 4, 6, 3), _gpu(2, 4, 18, dtype=torch.int64),
                     _gpu(2, 4, 6, 2, dtype=torch.int64), _gpu(2, 4, 6, 3, dtype=torch.int64, cls=_OnOtherGpu)],
        bary=[torch.zeros(2, 4, 6, 3, 3), _gpu(2, 4, 6, 3, 3, dtype=torch.float64), _gpu(2, 4, 6, 3), _gpu(2, 4, 6, 3, 2), _gpu(2, 4, 6, 3, 3, cls=_OnOtherGpu)],
        attrs=[torch.zeros(9, 3, 5), _gpu(9, 3, 5, dtype=torch.float16), _gpu(9, 3), _gpu(9, 2, 5), _gpu(9, 3, 0), _gpu(1, 3, meshattrs.MAX_D + 1)],
        grad=[torch.zeros(2, 4, 6, 3, 5), _gpu(2, 4, 6, 3, 4), _gpu(2, 4, 6, 3, 5, dtype=torch.float64), _gpu(2, 4, 6, 15), "grad"],
    )
    for name, values in refused.items():
        for value in values:
            call = _interp_call(**{name: value})
            assert not meshattrs.interpolate_face_attributes_backward_takes(*call), (name, value)
            if name != "grad":
                assert not meshattrs.interpolate_face_attributes_takes(*call[:3]), (name, value)
    for over, word in ((dict(attrs=torch.zeros(9, 3, 5)), "GPU"), (dict(attrs=_gpu(9, 3, 0)), "D >= 1"), (dict(pix_to_face=_gpu(2, 4, 6, 3)), "int64"),
                       (dict(bary=_gpu(2, 4, 6, 3, 2)), "barycentric_coords"), (dict(attrs=_gpu(1, 3, meshattrs.MAX_D + 1)), "65536")):
        with pytest.raises(ValueError, match=word):
            meshattrs.interpolate_face_attributes_forward(*_interp_call(**over)[:3])
        with pytest.raises(ValueError, match=word):
            meshattrs.interpolate_face_attributes_backward(*_interp_call(**over))
    with pytest.raises(ValueError, match="grad_pix_attrs"):
        meshattrs.interpolate_face_attributes_backward(*_interp_call(grad=_gpu(2, 4, 6, 3, 4)))


def _drop_ins(calls):
    def original(name):
        return lambda *args: calls.append((name, args)) or "the original's result"

    return {name: getattr(meshattrs, "drop_in_" + name)(original(name)) for name in OPERATORS}


def _taken_calls():
    return {OPERATORS[0]: _faces_call()[2:], OPERATORS[1]: _faces_call(), OPERATORS[2]: _interp_call()[:3], OPERATORS[3]: _interp_call()}


def test_a_capturing_stream_is_not_taken(monkeypatch):
    from autovfx_amd import _lib
    calls = []
    ours = _drop_ins(calls)
    takes = {OPERATORS[0]: meshattrs.face_areas_normals_takes, OPERATORS[1]: meshattrs.face_areas_normals_backward_takes,
             OPERATORS[2]: meshattrs.interpolate_face_attributes_takes, OPERATORS[3]: meshattrs.interpolate_face_attributes_backward_takes}
    assert all(takes[name](*args) for name, args in _taken_calls().items())
    monkeypatch.setattr(_lib, "capturing", lambda: True)
    for name, args in _taken_calls().items():
        assert not takes[name](*args)
        with pytest.raises(ValueError, match="capturing"):
            getattr(meshattrs, name)(*args)
        assert ours[name](*args) == "the original's result"
        assert calls[-1][0] == name and all(x is y for x, y in zip(calls[-1][1], args))
    assert len(calls) == 4


def test_the_drop_ins_hand_every_other_call_to_the_original():
    calls = []
    ours = _drop_ins(calls)
    cpu_faces = (torch.zeros(5), torch.zeros(5, 3), torch.zeros(7, 3), torch.zeros(5, 3, dtype=torch.int64))
    cpu_interp = (torch.zeros(1, 2, 2, 1, dtype=torch.int64), torch.zeros(1, 2, 2, 1, 3), torch.zeros(4, 3, 2), torch.zeros(1, 2, 2, 1, 2))
    others = ((OPERATORS[0], cpu_faces[2:]), (OPERATORS[0], _faces_call(verts=_gpu(7, 3, dtype=torch.float64))[2:]), (OPERATORS[0], ()),
              (OPERATORS[1], cpu_faces), (OPERATORS[1], _faces_call(grad_areas=_gpu(4))), (OPERATORS[1], cpu_faces[:3]),
              (OPERATORS[2], cpu_interp[:3]), (OPERATORS[2], _interp_call(attrs=_gpu(9, 3, 0))[:3]),
              (OPERATORS[3], cpu_interp), (OPERATORS[3], _interp_call(grad=_gpu(2, 4, 6, 3, 4))))
    for name, args in others:
        assert ours[name](*args) == "the original's result"
        assert calls[-1][0] == name and len(calls[-1][1]) == len(args) and all(x is y for x, y in zip(calls[-1][1], args))
    assert len(calls) == len(others)
    for name in OPERATORS:
        assert ours[name].__name__ == name and callable(ours[name].fallback)
    # a call by keyword, which the compiled originals accept, reaches the original with its keywords even where the tensors would be taken
    seen = []
    by_keyword = meshattrs.drop_in_face_areas_normals_forward(lambda *args, **kwargs: seen.append((args, kwargs)) or "the original's result")
    verts, faces = _faces_call()[2:]
    assert by_keyword(verts, faces=faces) == "the original's result" and by_keyword(verts=verts, faces=faces) == "the original's result"
    assert len(seen[0][0]) == 1 and seen[0][0][0] is verts and seen[0][1]["faces"] is faces
    assert seen[1][0] == () and seen[1][1]["verts"] is verts and seen[1][1]["faces"] is faces


# ---- the hook -------------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def stub_pytorch3d():
    """pytorch3d and a pytorch3d._C with the six operators the hook looks for."""
    names = ("pytorch3d", "pytorch3d._C")
    saved = {k: sys.modules.pop(k) for k in names if k in sys.modules}
    calls = []
    root, leaf = (types.ModuleType(n) for n in names)
    originals = {}
    for name in ("rasterize_meshes", "rasterize_meshes_backward") + OPERATORS:
        def operator(*args, _name=name):
            calls.append((_name, args))
            return "the original's result"

        operator.__name__ = name
        originals[name] = operator
        setattr(leaf, name, operator)
    root._C = leaf
    sys.modules.update(zip(names, (root, leaf)))
    path = list(sys.path)
    try:
        yield leaf, originals, calls
    finally:
        hook.uninstall()
        sys.path[:] = path
        for k in names:
            sys.modules.pop(k, None)
        sys.modules.update(saved)


def test_hook_patches_the_three_operators_and_uninstall_restores_them(stub_pytorch3d):
    leaf, originals, calls = stub_pytorch3d
    hook.install(path=False)
    patched = ("rasterize_meshes",) + OPERATORS
    ours = {name: getattr(leaf, name) for name in patched}
    for name in patched:
        assert ours[name] is not originals[name] and ours[name].fallback is originals[name] and ours[name].__name__ == name
        assert getattr(leaf, "reference_" + name) is originals[name]
    assert leaf.rasterize_meshes_backward is originals["rasterize_meshes_backward"] and not hasattr(leaf, "reference_rasterize_meshes_backward")
    assert hook.patched_modules.count("pytorch3d._C") == 1
    hook.install(path=False)                                                          # a second install changes nothing
    assert all(getattr(leaf, name) is ours[name] and getattr(leaf, "reference_" + name) is originals[name] for name in patched)
    # looked up by attribute at call time, as pytorch3d's autograd classes do: a CPU call reaches the original with its arguments untouched
    sent = (torch.zeros(7, 3), torch.zeros(5, 3, dtype=torch.int64))
    assert sys.modules["pytorch3d"]._C.face_areas_normals_forward(*sent) == "the original's result"
    assert calls[-1][0] == "face_areas_normals_forward" and all(x is y for x, y in zip(calls[-1][1], sent))
    sent = (torch.zeros(1, 2, 2, 1, dtype=torch.int64), torch.zeros(1, 2, 2, 1, 3), torch.zeros(4, 3, 2), torch.zeros(1, 2, 2, 1, 2))
    assert sys.modules["pytorch3d"]._C.interpolate_face_attributes_backward(*sent) == "the original's result"
    assert calls[-1][0] == "interpolate_face_attributes_backward" and all(x is y for x, y in zip(calls[-1][1], sent))
    hook.uninstall()
    for name in patched:
        assert getattr(leaf, name) is originals[name] and not hasattr(leaf, "reference_" + name)
    assert hook.patched_modules == []


@pytest.mark.parametrize("missing", OPERATORS)
def test_a_c_module_with_one_of_a_pair_keeps_that_pair(stub_pytorch3d, missing):
    leaf, originals, _calls = stub_pytorch3d
    delattr(leaf, missing)
    hook.install(path=False)
    pair = OPERATORS[:2] if missing in OPERATORS[:2] else OPERATORS[2:]
    other = OPERATORS[2:] if missing in OPERATORS[:2] else OPERATORS[:2]
    for name in pair:
        assert getattr(leaf, name, None) is originals[name] or name == missing
        assert not hasattr(leaf, "reference_" + name)
    assert not hasattr(leaf, missing)
    for name in other + ("rasterize_meshes",):
        assert getattr(leaf, name).fallback is originals[name]


def test_the_other_c_modules_still_load_under_the_hook():
    """``diff_gaussian_rasterization._C`` and ``simple_knn._C`` share the leaf name and define none of the four operators."""
    names = ("diff_gaussian_rasterization._C", "simple_knn._C")
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k.split(".")[0] in ("diff_gaussian_rasterization", "simple_knn")}
    path = list(sys.path)
    try:
        hook.install()
        for mod in (importlib.import_module(n) for n in names):
            assert not any(hasattr(mod, name) or hasattr(mod, "reference_" + name) for name in OPERATORS)
            assert mod.__name__ not in hook.patched_modules and mod.__file__.startswith(hook._REPO_ROOT)
        assert not any(hasattr(torch._C, "reference_" + name) for name in OPERATORS)
    finally:
        hook.uninstall()
        sys.path[:] = path
        for k in list(sys.modules):
            if k.split(".")[0] in ("diff_gaussian_rasterization", "simple_knn"):
                sys.modules.pop(k)
        sys.modules.update(saved)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------

def test_cabi_version_and_refusals_need_no_device():
    from autovfx_amd import _lib
    L = _lib.lib
    assert L.gsr_abi_version() == 20 == _lib.ABI_VERSION
    a, b, c, d, e, f, g = (1 << 20) * 1, (1 << 20) * 2, (1 << 20) * 3, (1 << 20) * 4, (1 << 20) * 5, (1 << 20) * 6, (1 << 20) * 7   # never read: every call is refused
    big = 1 << 31

    def refused(name, args, word):
        return getattr(L, name)(*args, None) != 0 and word in _lib.last_error() and name in _lib.last_error()

    table = {
        # V F verts faces areas normals
        "gsr_face_areas_normals": ([100, 50, a, b, c, d], [(0, -1, "negative"), (1, -1, "negative"), (0, big, "2^31"), (1, big, "2^31"),
                                                          (2, None, "null"), (3, None, "null"), (4, None, "null"), (5, None, "null"),
                                                          (2, a + 2, "aligned"), (3, b + 4, "aligned"), (4, c + 1, "aligned"), (5, d + 3, "aligned")]),
        # V F verts faces grad_areas grad_normals grad_verts
        "gsr_face_areas_normals_backward": ([100, 50, a, b, c, d, e], [(0, -1, "negative"), (1, -1, "negative"), (0, big, "2^31"), (1, big, "2^31"),
                                                                      (2, None, "null"), (3, None, "null"), (4, None, "null"), (5, None, "null"),
                                                                      (6, None, "null"), (2, a + 1, "aligned"), (3, b + 4, "aligned"),
                                                                      (4, c + 2, "aligned"), (5, d + 2, "aligned"), (6, e + 3, "aligned")]),
        # P F D pix_to_face bary attrs out
        "gsr_interp_face_attrs": ([100, 50, 3, a, b, c, d], [(0, -1, "negative"), (1, -1, "negative"), (0, big, "2^31"), (1, big, "2^31"),
                                                            (2, 0, "D = 0"), (2, -3, "D = -3"), (2, 65537, "D = 65537"),
                                                            (3, None, "null"), (4, None, "null"), (5, None, "null"), (6, None, "null"),
                                                            (3, a + 4, "aligned"), (4, b + 2, "aligned"), (5, c + 1, "aligned"), (6, d + 2, "aligned")]),
        # P F D pix_to_face bary attrs grad_out grad_bary grad_attrs
        "gsr_interp_face_attrs_backward": ([100, 50, 3, a, b, c, d, e, f], [(0, -1, "negative"), (1, -1, "negative"), (0, big, "2^31"), (1, big, "2^31"),
                                                                           (2, 0, "D = 0"), (2, 65537, "D = 65537"),
                                                                           (3, None, "null"), (4, None, "null"), (5, None, "null"), (6, None, "null"),
                                                                           (7, None, "null"), (8, None, "null"), (3, a + 4, "aligned"),
                                                                           (4, b + 2, "aligned"), (5, c + 1, "aligned"), (6, d + 2, "aligned"),
                                                                           (7, e + 1, "aligned"), (8, f + 3, "aligned")]),
    }
    for name, (ok, cases_) in table.items():
        for at, value, word in cases_:
            args = list(ok)
            args[at] = value
            assert refused(name, args, word), (name, at, value, _lib.last_error())
    # nothing to do: no launch, nothing read, arrays of no elements may be NULL
    assert L.gsr_face_areas_normals(100, 0, a, None, None, None, None) == 0 and L.gsr_face_areas_normals(0, 0, None, None, None, None, None) == 0
    assert L.gsr_face_areas_normals_backward(0, 50, None, b, c, d, None, None) == 0
    assert L.gsr_interp_face_attrs(0, 50, 3, None, None, c, None, None) == 0 and L.gsr_interp_face_attrs(0, 0, 1, None, None, None, None, None) == 0
    assert L.gsr_interp_face_attrs_backward(0, 0, 3, None, None, None, None, None, None, None) == 0
    assert g
