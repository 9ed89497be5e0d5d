"""pytorch3d's rasterize_meshes without a GPU: the numpy restatement of the contract (autovfx_amd/meshraster.py:
rasterize_face_verts_host) against the float64 truth of tests/meshraster_cases.py and against hand-built rows, which calls the kernels
take, the hook's patch of a stub pytorch3d._C, and the C ABI's refusals."""
from __future__ import annotations

import ctypes
import importlib
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import meshraster_cases as cases
from autovfx_amd import hook, meshraster
from autovfx_amd.meshraster import rasterize_face_verts_host, rasterize_takes
from meshraster_cases import one_mesh, tri_around
from helpers import fake_gpu as _gpu

F = np.float32


def _host(fv, size, K=1, first=None, num=None, nbr=None, **flags):
    fv = np.asarray(fv, F).reshape(-1, 3, 3)
    a, b, c = one_mesh(fv)
    return rasterize_face_verts_host(fv, a if first is None else first, b if num is None else num, c if nbr is None else nbr, size, 0.0, K,
                                     **flags)


@pytest.mark.parametrize("perspective", [True, False])
@pytest.mark.parametrize("index", range(len(cases.SCENES)))
def test_host_restatement_against_truth(index, perspective):
    H, W, _n, _seed = cases.SCENES[index]
    fv, want = cases.scene_truth(index, 10, perspective)
    got = rasterize_face_verts_host(fv, *one_mesh(fv), (H, W), 0.0, 10, perspective_correct=perspective)
    ez, eb, ed = cases.against_truth(got, want, f"scene {index}, perspective_correct={perspective}")
    assert ez <= cases.BAR_Z and eb <= cases.BAR_BARY and ed <= cases.BAR_DIST
    listed = (want[0] >= 0).sum(-1)
    assert listed.mean() > 3 and listed.max() >= 9                  # the scenes are deep enough to exercise the K slots


@pytest.mark.parametrize("index", range(len(cases.NEAR_PLANE)))
def test_near_plane_restatement_against_truth(index):
    """Depths at and behind the camera plane, with the flags off and with ``perspective_correct`` and ``clip_barycentric_coords``: the
    truth's faces on every decided pixel and 4 x the restatement's own measured error, as on the scenes.  With ``perspective_correct`` and
    no clip only ``pix_to_face`` is compared: the corrected barycentrics are a quotient by a denominator that passes through zero inside
    such a face, and where it is tiny the fp32 quotient is far from the float64 one (z differs by up to 87, the barycentrics by 1061, on
    these two scenes) -- no bar would say anything there; the clip bounds the barycentrics again."""
    H, W, _n, _seed = cases.NEAR_PLANE[index]
    for flags in ((False, False), (True, True)):
        fv, want = cases.near_plane_truth(index, *flags)
        got = rasterize_face_verts_host(fv, *one_mesh(fv), (H, W), 0.0, 10, perspective_correct=flags[0], clip_barycentric_coords=flags[1])
        ez, eb, ed = cases.against_truth(got, want, f"near plane {index}, perspective and clip {flags}")
        assert ez <= cases.NEAR_BAR_Z and eb <= cases.NEAR_BAR_BARY and ed <= cases.NEAR_BAR_DIST
        assert (got[1][got[0] >= 0] < 0.05).any()
    plain = rasterize_face_verts_host(fv, *one_mesh(fv), (H, W), 0.0, 10)
    fv, want = cases.near_plane_truth(index, True, False)
    got = rasterize_face_verts_host(fv, *one_mesh(fv), (H, W), 0.0, 10, perspective_correct=True)
    decided = ~want[4]
    assert want[4].mean() <= cases.MAX_UNDECIDED and np.array_equal(got[0][decided], want[0][decided])
    assert (got[0] >= 0).sum() < (plain[0] >= 0).sum()               # depths that only the correction turns negative


def test_huge_depths_are_pinned():
    """Finite depths times 1e19 overflow ``(w0 * z1) * z2``: the sum of the three is ``inf`` or NaN, ``max(NaN, eps)`` must be ``eps`` and
    ``max(0, min(1, NaN))`` must be 1, as C's ``fmaxf`` / ``fminf`` give them (with numpy's ``maximum`` / ``minimum`` the NaN spreads and all
    four outputs differ).  The fixture is what the kernels give on an MI355X."""
    golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "meshraster", "huge_z_37x53.npz"))
    H, W, n_faces, seed = cases.SCENES[0]
    fv = cases.scaled_scene(n_faces, seed, z_scale=1e19)
    assert np.array_equal(fv, golden["face_verts"]) and np.isfinite(fv).all()
    got = rasterize_face_verts_host(fv, *one_mesh(fv), (H, W), 0.0, 10, perspective_correct=True, clip_barycentric_coords=True)
    assert (got[0] >= 0).sum() > 5000 and not np.isnan(got[1]).any()
    for name, g in zip(("pix_to_face", "zbuf", "bary_coords", "dists"), got):
        w = golden[name].astype(g.dtype)
        assert g.shape == w.shape and np.array_equal(g.view(np.int32) if g.dtype == F else g, w.view(np.int32) if w.dtype == F else w), name


def test_nan_loses_every_min_and_max_and_orders_before_nothing():
    """By hand, on one pixel (4 x 4, pixel (1, 1) at (0.25, 0.25)): three faces around it whose perspective products overflow."""
    big = np.float32(3e38)
    t = tri_around(0.25, 0.25, r=0.3)
    over, near = t.copy(), t.copy()
    over[:, 2] = big                                                  # (w * z) * z = inf for every w: inf / inf = NaN in all three
    near[:, 2] = 1.0
    # perspective_correct alone: b is NaN, pz is NaN, which is not < 0 and not less than anything: never listed
    face, z, _b, _d = _host([over, near], (4, 4), K=2, perspective_correct=True)
    assert list(face[0, 1, 1]) == [1, -1] and list(z[0, 1, 1]) == [1.0, -1.0]
    # with the clip: max(0, min(1, NaN)) = 1 three times, b = 1 / 3 each, pz = 3e38 or its neighbour
    face, z, b, _d = _host([over, near], (4, 4), K=2, perspective_correct=True, clip_barycentric_coords=True)
    third = np.float32(1.0) / np.float32(3.0)
    assert list(face[0, 1, 1]) == [1, 0] and np.array_equal(b[0, 1, 1, 1], [third] * 3)
    assert z[0, 1, 1, 1] == (third * big + third * big) + third * big


def test_an_infinite_depth_is_listed_last():
    """Depths at the largest finite float32: ``(b0 * z0 + b1 * z1) + b2 * z2`` rounds to ``inf`` on some pixels.  Such a face is kept: it comes
    behind every finite depth, the lower index first, and before the empty slots."""
    H, W, n_faces, seed = cases.SCENES[0]
    fv = cases.scaled_scene(n_faces, seed, z_scale=1e38)
    assert np.isfinite(fv).all() and (fv[:, :, 2] == np.finfo(F).max).any()
    face, z, _b, _d = rasterize_face_verts_host(fv, *one_mesh(fv), (H, W), 0.0, 10)
    listed = face >= 0
    assert np.isinf(z[listed]).sum() > 100 and (~np.isinf(z[listed])).sum() > 100 and not np.isnan(z).any()
    assert (listed[..., :-1] >= listed[..., 1:]).all()                                    # no empty slot before a filled one
    pair = listed[..., 1:]
    assert (z[..., :-1][pair] <= z[..., 1:][pair]).all()
    assert (face[..., :-1][pair] < face[..., 1:][pair])[z[..., :-1][pair] == z[..., 1:][pair]].all()
    assert (np.isinf(z[..., :-1]) & pair & ~np.isinf(z[..., 1:])).sum() == 0


@pytest.mark.parametrize("K", [4, 16])
def test_non_finite_vertices_leave_the_finite_faces_alone(K):
    """Outside the contract (what such a face receives is unspecified), but the finite faces of a pixel keep their order and their values."""
    H, W, n_faces, seed = cases.SCENES[0]
    broken, finite_only, is_broken = cases.non_finite_scene(n_faces, seed)
    assert 40 <= is_broken.sum() and all(np.isnan(broken[..., i]).any() and np.isinf(broken[..., i]).any() for i in range(3))
    held = 0
    for flags in ((False, False, False), (True, False, False), (True, True, False)):
        got = rasterize_face_verts_host(broken, *one_mesh(broken), (H, W), 0.0, K, None, None, *flags)
        want = rasterize_face_verts_host(finite_only, *one_mesh(finite_only), (H, W), 0.0, K, None, None, *flags)
        held += cases.finite_faces_are_a_prefix(got, want, is_broken, f"K={K}, flags={flags}")
    assert held > 0                                                  # an infinite depth is listed last, where slots are to spare


def test_host_restatement_is_chunk_independent():
    fv, _ = cases.scene_truth(0)
    ref = rasterize_face_verts_host(fv, *one_mesh(fv), (37, 53), 0.0, 4)
    for chunk in (1, 300 * 7 + 1):
        got = rasterize_face_verts_host(fv, *one_mesh(fv), (37, 53), 0.0, 4, chunk_elems=chunk)
        assert all(np.array_equal(g, r) for g, r in zip(got, ref))


def test_one_triangle_in_a_4x4_image():
    # pixel centres at +-0.25, +-0.75, column 0 at x = +0.75 and row 0 at y = +0.75; the triangle holds x <= 1, y <= 1, x + y >= 0.9
    face, z, bary, dists = _host([[(1.0, 1.0, 2.0), (-0.1, 1.0, 2.0), (1.0, -0.1, 2.0)]], (4, 4), K=2)
    assert face.shape == z.shape == dists.shape == (1, 4, 4, 2) and bary.shape == (1, 4, 4, 2, 3)
    assert face.dtype == np.int64 and z.dtype == bary.dtype == dists.dtype == F
    covered = np.zeros((4, 4), bool)
    covered[0, 0] = covered[0, 1] = covered[1, 0] = True
    assert np.array_equal(face[0, :, :, 0] == 0, covered)
    assert np.all(face[0, :, :, 0][~covered] == -1) and np.all(face[..., 1] == -1)
    for out in (z, dists):
        assert np.all(out[0, :, :, 0][~covered] == -1) and np.all(out[..., 1] == -1)
    assert np.all(bary[0, :, :, 0][~covered] == -1) and np.all(bary[..., 1, :] == -1)
    assert np.allclose(z[0, :, :, 0][covered], 2.0, atol=1e-6)
    assert np.allclose(bary[0, :, :, 0][covered].sum(-1), 1.0, atol=1e-6) and np.all(bary[0, :, :, 0][covered] > 0)
    # dists is minus the squared distance to the nearest edge: pixel (0, 0) at (0.75, 0.75) is 0.25 from x = 1 and from y = 1
    assert np.all(dists[0, :, :, 0][covered] < 0)
    assert dists[0, 0, 0, 0] == pytest.approx(-0.0625, abs=1e-6)
    assert dists[0, 0, 1, 0] == pytest.approx(-((0.25 + 0.75 - 0.9) ** 2) / 2, abs=1e-6)    # (0.25, 0.75): nearest is x + y = 0.9


def test_x_points_left_and_y_points_up():
    face = _host([tri_around(0.75, 0.75), tri_around(-0.75, 0.25)], (4, 4))[0][0, :, :, 0]
    want = np.full((4, 4), -1)
    want[0, 0], want[1, 3] = 0, 1
    assert np.array_equal(face, want)


def test_non_square_images_stretch_the_longer_side():
    # H = 2, W = 4: x centres at -+0.5, -+1.5, y centres at -+0.5
    face = _host([tri_around(1.5, 0.5), tri_around(-0.5, -0.5)], (2, 4))[0][0, :, :, 0]
    want = np.full((2, 4), -1)
    want[0, 0], want[1, 2] = 0, 1
    assert np.array_equal(face, want)
    # H = 4, W = 2: the other way round
    face = _host([tri_around(0.5, 1.5), tri_around(-0.5, -1.5)], (4, 2))[0][0, :, :, 0]
    want = np.full((4, 2), -1)
    want[0, 0], want[3, 1] = 0, 1
    assert np.array_equal(face, want)


def test_equal_depths_go_by_the_lower_face_index():
    t = tri_around(0.25, 0.25, r=0.3)
    far = tri_around(0.25, 0.25, z=3.0, r=0.3)
    face, z, _b, _d = _host([far, t, t], (4, 4), K=3)
    assert list(face[0, 1, 1]) == [1, 2, 0] and list(z[0, 1, 1]) == [1.0, 1.0, 3.0]


def test_faces_that_are_skipped():
    t = tri_around(0.25, 0.25, r=0.3)
    flat = np.array([(0.0, 0.0, 1.0), (0.25, 0.25, 1.0), (0.5, 0.5, 1.0)], F)          # zero area
    behind = tri_around(0.25, 0.25, z=-1.0, r=0.3)                                      # every z below 0
    face = _host([flat, behind, t], (4, 4), K=3)[0]
    assert list(face[0, 1, 1]) == [2, -1, -1]
    assert set(np.unique(face)) == {-1, 2}
    # mixed signs: kept only where the interpolated depth is not negative
    wide = np.array([(-3.0, -3.0, -1.3), (3.0, -3.0, 1.0), (0.0, 4.0, 1.0)], F)   # (-1.3: the zero line passes no pixel centre)
    face, z, bary, _d = _host([wide], (16, 16))
    in_front = wide.copy()
    in_front[:, 2] = 1.0
    full = _host([in_front], (16, 16))[0]
    listed = face[0, :, :, 0] == 0
    assert np.all(full == 0) and 0 < listed.sum() < 256
    assert np.all(z[0, :, :, 0][listed] >= 0)
    w64 = bary[0, :, :, 0].astype(np.float64)
    interpolated = -1.3 * w64[..., 0] + w64[..., 1] + w64[..., 2]
    assert np.all(interpolated[listed] >= 0)
    _f, tz, _tb, _td, undecided = cases.truth(wide[None], *one_mesh(wide[None]), (16, 16), 1)
    assert np.array_equal(listed[~undecided[0]], (tz[0, :, :, 0] >= 0)[~undecided[0]])


def test_cull_backfaces():
    t = tri_around(0.25, 0.25, r=0.3)
    pair = [t, t[::-1].copy()]
    both = _host(pair, (4, 4), K=2)[0]
    assert list(both[0, 1, 1]) == [0, 1]
    culled = _host(pair, (4, 4), K=2, cull_backfaces=True)[0]
    area = [(p[0, 0] - p[1, 0]) * (p[2, 1] - p[1, 1]) - (p[0, 1] - p[1, 1]) * (p[2, 0] - p[1, 0]) for p in (np.asarray(q, np.float64) for q in pair)]
    front = int(np.argmax(area))
    assert area[front] > 0 > area[1 - front]
    assert list(culled[0, 1, 1]) == [front, -1]


def test_clip_barycentric_coords():
    # perspective correction with two vertices behind the camera leaves [0, 1] (b0, b1 < 0, b2 > 1 wherever the depth is positive); the clip
    # brings the coordinates back and renormalises
    wide = np.array([[(-3.0, -3.0, -4.0), (3.0, -3.0, -4.0), (0.0, 4.0, 1.0)]], F)
    _f, _z, loose, _d = _host(wide, (16, 16), perspective_correct=True)
    face, _z, clipped, _d = _host(wide, (16, 16), perspective_correct=True, clip_barycentric_coords=True)
    listed = face[0, :, :, 0] == 0
    assert listed.sum() > 20
    inside = clipped[0, :, :, 0][listed]
    assert np.all(inside >= 0) and np.all(inside <= 1) and np.allclose(inside.sum(-1), 1.0, atol=1e-6)
    raw = loose[0, :, :, 0][loose[0, :, :, 0, 0] != -1]
    assert len(raw) == listed.sum() and np.all(raw[:, :2] < 0) and np.all(raw[:, 2] > 1)


def test_perspective_correct_on_and_off():
    t = tri_around(0.25, 0.25, z=(1.0, 4.0, 4.0), r=0.6)
    _f, z_off, b_off, _d = _host([t], (4, 4))
    _f, z_on, b_on, _d = _host([t], (4, 4), perspective_correct=True)
    w = b_off[0, 1, 1, 0].astype(np.float64)
    zs = np.array([1.0, 4.0, 4.0])
    assert z_off[0, 1, 1, 0] == pytest.approx(float(w @ zs), abs=1e-5)
    assert z_on[0, 1, 1, 0] == pytest.approx(1.0 / float((w / zs).sum()), abs=1e-5)       # 1 / z is what is linear on the screen
    assert np.allclose(b_on[0, 1, 1, 0], (w / zs) / (w / zs).sum(), atol=1e-5)
    assert z_on[0, 1, 1, 0] < z_off[0, 1, 1, 0] - 0.1


def test_neighbour_rule_keeps_the_face_nearer_to_its_own_edges():
    big = tri_around(0.0, 0.0, z=1.0, r=0.95)
    small = tri_around(0.25, 0.25, z=2.0, r=0.6)
    fv = np.stack([big, small])
    alone = [_host([f], (8, 8))[3][0, :, :, 0] for f in (big, small)]                    # each face's dists without the other
    free = _host(fv, (8, 8), K=2)[0][0]
    both = (free[..., 0] == 0) & (free[..., 1] == 1)
    assert both.sum() > 4
    face, z, _b, dists = _host(fv, (8, 8), K=2, nbr=np.array([1, 0], np.int64))
    assert np.all(face[0, :, :, 1][both] == -1)                                          # one slot where both cover the pixel
    small_wins = np.abs(alone[1]) < np.abs(alone[0])
    assert (both & small_wins).any() and (both & ~small_wins).any()
    assert np.array_equal(face[0, :, :, 0][both], np.where(small_wins, 1, 0)[both])
    assert np.array_equal(dists[0, :, :, 0][both], np.where(small_wins, alone[1], alone[0])[both])
    assert np.array_equal(face[0, :, :, 0][~both], free[..., 0][~both])                  # elsewhere nothing changed
    # a neighbour that is not kept at the pixel, or a face naming itself, changes nothing
    assert np.array_equal(_host(fv, (8, 8), K=2, nbr=np.array([0, 1], np.int64))[0][0], free)


def test_two_meshes_with_unequal_face_counts():
    fv = np.stack([tri_around(0.75, 0.75), tri_around(0.25, 0.25, r=0.3), tri_around(-0.25, 0.25), tri_around(0.25, 0.25, z=2.0, r=0.3)])
    first, num = np.array([0, 3], np.int64), np.array([3, 1], np.int64)
    out = _host(fv, (4, 4), K=2, first=first, num=num, nbr=np.full(4, -1, np.int64))
    assert out[0].shape == (2, 4, 4, 2)
    a = _host(fv[:3], (4, 4), K=2)
    b = _host(fv[3:], (4, 4), K=2)
    for got, wa, wb in zip(out, a, b):
        assert np.array_equal(got[0], wa[0])
    assert np.array_equal(out[0][1], np.where(b[0][0] >= 0, b[0][0] + 3, -1))            # packed indices
    for got, wb in zip(out[1:], b[1:]):
        assert np.array_equal(got[1], wb[0])
    assert out[0][1, 1, 1, 0] == 3 and out[0][0, 1, 1, 0] == 1


def test_no_faces():
    out = rasterize_face_verts_host(np.zeros((0, 3, 3), F), [0], [0], np.zeros(0, np.int64), (3, 5), 0.0, 2)
    assert [o.shape for o in out] == [(1, 3, 5, 2), (1, 3, 5, 2), (1, 3, 5, 2, 3), (1, 3, 5, 2)]
    assert all(np.all(o == -1) for o in out)
    with pytest.raises(ValueError, match="blur_radius"):
        rasterize_face_verts_host(np.zeros((0, 3, 3), F), [0], [0], np.zeros(0, np.int64), (3, 5), 1e-4, 2)


def _call(F_=7, N=1, **over):
    """pytorch3d's positional arguments for a call the kernels take, with overrides by name."""
    args = dict(face_verts=_gpu(F_, 3, 3), first=_gpu(N, dtype=torch.int64), num=_gpu(N, dtype=torch.int64), nbr=_gpu(F_, dtype=torch.int64),
                image_size=(32, 48), blur_radius=0.0, faces_per_pixel=10, bin_size=None, max_faces_per_bin=50_000, perspective_correct=True,
                clip_barycentric_coords=False, cull_backfaces=False)
    assert set(over) <= set(args)
    args.update(over)
    return tuple(args.values())


def test_which_calls_the_kernels_take():
    assert rasterize_takes(*_call())
    assert rasterize_takes(*_call(faces_per_pixel=1)) and rasterize_takes(*_call(faces_per_pixel=16))
    assert rasterize_takes(*_call(F_=0)) and rasterize_takes(*_call(N=3))
    assert rasterize_takes(*_call(blur_radius=0)) and rasterize_takes(*_call(image_size=[16384, 1]))
    assert rasterize_takes(*_call(bin_size=0, max_faces_per_bin=1, cull_backfaces=True, clip_barycentric_coords=True))   # ignored / flags
    refused = dict(
        face_verts=[torch.zeros(7, 3, 3), _gpu(7, 3, 3, dtype=torch.float64), _gpu(7, 3), _gpu(7, 3, 2), _gpu(3, 3, 7).permute(2, 0, 1),
                    _gpu(7, 3, 3, requires_grad=True), np.zeros((7, 3, 3), F)],
        first=[torch.zeros(1, dtype=torch.int64), _gpu(1, dtype=torch.int32), _gpu(2, dtype=torch.int64), _gpu(1, 1, dtype=torch.int64)],
        num=[torch.zeros(1, dtype=torch.int64), _gpu(1, dtype=torch.int32)],
        nbr=[torch.zeros(7, dtype=torch.int64), _gpu(7, dtype=torch.float32), _gpu(6, dtype=torch.int64)],
        image_size=[32, (32,), (0, 48), (32, 16385), (32.0, 48.0)],
        blur_radius=[1e-6, -1.0, None],
        faces_per_pixel=[0, 17, 10.0],
    )
    for name, values in refused.items():
        for value in values:
            assert not rasterize_takes(*_call(**{name: value})), (name, value)
    for over, word in ((dict(face_verts=torch.zeros(7, 3, 3)), "GPU"), (dict(blur_radius=1e-4), "blur_radius"), (dict(faces_per_pixel=17), "1..16"),
                       (dict(face_verts=_gpu(7, 3, 3, requires_grad=True)), "gradient"), (dict(image_size=(32, 16385)), "16384")):
        with pytest.raises(ValueError, match=word):
            meshraster.rasterize_face_verts(*_call(**over))


def test_a_capturing_stream_is_not_taken(monkeypatch):
    """The call reads the pair total back and allocates its scratch, which would break a capture: such a call is the original's."""
    from autovfx_amd import _lib
    calls = []
    ours = meshraster.drop_in(lambda *args: calls.append(args) or "the original's result")
    assert rasterize_takes(*_call())
    monkeypatch.setattr(_lib, "capturing", lambda: True)
    assert not rasterize_takes(*_call())
    with pytest.raises(ValueError, match="capturing"):
        meshraster.rasterize_face_verts(*_call())
    args = _call()
    assert ours(*args) == "the original's result"
    assert len(calls) == 1 and all(x is y for x, y in zip(calls[0], args))


def test_too_many_pairs_go_to_the_original(monkeypatch):
    """The one refusal that is only known after the count step: the drop-in hands the call on, the direct call raises."""
    calls = []
    ours = meshraster.drop_in(lambda *args: calls.append(args) or "the original's result")

    def too_many(*_args):
        raise meshraster.TooManyPairs("rasterize_meshes: 4294967296 (tile, face) pairs, at most 2^31 - 1")

    monkeypatch.setattr(meshraster, "_taken", too_many)
    args = _call()
    assert ours(*args) == "the original's result"
    assert len(calls) == 1 and all(x is y for x, y in zip(calls[0], args))
    with pytest.raises(ValueError, match="pairs"):
        meshraster.rasterize_face_verts(*args)


@pytest.fixture
def stub_pytorch3d():
    """pytorch3d and pytorch3d._C as far as the hook looks at them."""
    names = ("pytorch3d", "pytorch3d._C")
    saved = {k: sys.modules.pop(k) for k in names if k in sys.modules}
    calls = []

    def rasterize_meshes(*args):
        calls.append(args)
        return "the original's result"

    def rasterize_meshes_backward(*args):
        raise AssertionError("not called")

    root, leaf = (types.ModuleType(n) for n in names)
    leaf.rasterize_meshes, leaf.rasterize_meshes_backward = rasterize_meshes, rasterize_meshes_backward
    root._C = leaf
    sys.modules.update(zip(names, (root, leaf)))
    try:
        yield leaf, rasterize_meshes, calls
    finally:
        hook.uninstall()
        for k in names:
            sys.modules.pop(k, None)
        sys.modules.update(saved)


def test_hook_patches_the_operator_and_uninstall_restores_it(stub_pytorch3d):
    leaf, original, calls = stub_pytorch3d
    backward = leaf.rasterize_meshes_backward
    path = list(sys.path)
    try:
        hook.install(path=False)
        ours = leaf.rasterize_meshes
        assert ours is not original and ours.fallback is original and ours.__name__ == "rasterize_meshes"
        assert leaf.reference_rasterize_meshes is original
        assert leaf.rasterize_meshes_backward is backward                                 # nothing else moved
        assert "pytorch3d._C" in hook.patched_modules
        hook.install(path=False)                                                          # a second install changes nothing
        assert leaf.rasterize_meshes is ours and leaf.reference_rasterize_meshes is original
        # what the kernels do not take reaches the original with its arguments untouched: a CPU call, blur, K = 17, a gradient
        cpu = _call(face_verts=torch.zeros(7, 3, 3), first=torch.zeros(1, dtype=torch.int64), num=torch.zeros(1, dtype=torch.int64),
                    nbr=torch.zeros(7, dtype=torch.int64))
        others = (cpu, _call(blur_radius=1e-4), _call(faces_per_pixel=17), _call(face_verts=_gpu(7, 3, 3, requires_grad=True)))
        for args in others:
            assert sys.modules["pytorch3d"]._C.rasterize_meshes(*args) == "the original's result"      # looked up by attribute, as pytorch3d does
        assert len(calls) == 4 and all(all(x is y for x, y in zip(got, sent)) for got, sent in zip(calls, others))
        hook.uninstall()
        assert leaf.rasterize_meshes is original and not hasattr(leaf, "reference_rasterize_meshes")
        assert hook.patched_modules == []
    finally:
        sys.path[:] = path


def test_a_c_module_without_both_operators_is_left_alone(stub_pytorch3d):
    leaf, original, _calls = stub_pytorch3d
    del leaf.rasterize_meshes_backward                                                    # some other package's _C
    path = list(sys.path)
    try:
        hook.install(path=False)
        assert leaf.rasterize_meshes is original and "pytorch3d._C" not in hook.patched_modules
    finally:
        sys.path[:] = path


def test_the_other_c_modules_are_unpatched_and_working_under_the_hook():
    """``diff_gaussian_rasterization._C`` and ``simple_knn._C`` share the leaf name: imported afresh through the hook's loader they stay as
    they are and keep their surface."""
    names = ("diff_gaussian_rasterization._C", "simple_knn._C")
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k.split(".")[0] in ("diff_gaussian_rasterization", "simple_knn")}
    path = list(sys.path)
    try:
        hook.install()
        dgr, knn = (importlib.import_module(n) for n in names)
        for mod in (dgr, knn):
            assert not hasattr(mod, "reference_rasterize_meshes") and not hasattr(mod, "rasterize_meshes")
            assert mod.__name__ not in hook.patched_modules
            assert mod.__file__.startswith(hook._REPO_ROOT)
        assert callable(dgr.rasterize_gaussians) and callable(dgr.rasterize_gaussians_backward) and callable(dgr.mark_visible)
        assert callable(knn.distCUDA2)
        with pytest.raises(ValueError, match="GPU"):                                      # it runs: the call reaches autovfx_amd.knn's checks
            knn.distCUDA2(torch.zeros(4, 3))
    finally:
        hook.uninstall()
        sys.path[:] = path
        for k in list(sys.modules):
            if k.split(".")[0] in ("diff_gaussian_rasterization", "simple_knn"):
                sys.modules.pop(k)
        sys.modules.update(saved)


def test_a_real_extension_module_named_C_loads_through_the_hook():
    """Leaf ``_C`` makes the hook wrap the loader of every ``*._C`` imported after ``install()``; ``torch._C`` is a compiled extension of
    that name.  In a fresh interpreter: it is loaded through the wrapper, stays unpatched and torch works."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from autovfx_amd import hook\n"
            "hook.install()\n"
            "assert 'torch' not in sys.modules\n"
            "import torch, torch._C\n"
            "assert type(torch._C.__spec__.loader).__name__ == '_PatchingLoader', type(torch._C.__spec__.loader)\n"
            "assert torch._C.__file__.endswith('.so') and not hasattr(torch._C, 'reference_rasterize_meshes')\n"
            "assert hook.patched_modules == []\n"
            "assert float(torch.arange(4.0).sum()) == 6.0\n"
            "print('ok')\n") % hook._REPO_ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]


def test_cabi_version_and_refusals_need_no_device():
    from autovfx_amd import _lib
    L = _lib.lib
    assert L.gsr_abi_version() == 20 == _lib.ABI_VERSION
    plan = L.gsr_mesh_raster_plan_bytes(1000, 1, 1080, 1920)
    assert 256 + 12 * 1000 + 8 * 68 * 120 <= plan <= 256 + 12 * 1000 + 8 * 68 * 120 + 4 * 256
    assert L.gsr_mesh_raster_plan_bytes(1000, 2, 1080, 1920) > plan
    for bad in ((-1, 1, 8, 8), (5, -1, 8, 8), ((1 << 31) - 1, 1, 8, 8), (5, 1, 0, 8), (5, 1, 8, 16385), (5, 1 << 12, 16384, 16384)):
        assert L.gsr_mesh_raster_plan_bytes(*bad) == 0, bad
    assert L.gsr_mesh_raster_pair_bytes(0) == 256 and L.gsr_mesh_raster_pair_bytes(1000) == 4096
    assert L.gsr_mesh_raster_pair_bytes(-1) == 0 and L.gsr_mesh_raster_pair_bytes(1 << 31) == 0
    assert L.gsr_mesh_raster_pair_bytes((1 << 31) - 1) == 1 << 33

    fv, first, num, nbr, scratch, pairs = 4096, 8192, 8192 + 64, 1 << 14, 1 << 20, 1 << 21   # addresses that are never read: every call is refused
    face, z, bary, dists = 1 << 22, 1 << 23, 1 << 24, 1 << 25
    total = ctypes.c_int64(-5)

    def count_refused(F_, N, verts, a, b, H, W, where, nbytes, out, word):
        return L.gsr_mesh_raster_count(F_, N, verts, a, b, H, W, 0, where, nbytes, out, None) != 0 and word in _lib.last_error()

    assert L.gsr_mesh_raster_count(0, 1, None, None, None, 8, 8, 0, None, 0, ctypes.byref(total), None) == 0 and total.value == 0
    total.value = -5
    assert L.gsr_mesh_raster_count(1000, 0, None, None, None, 8, 8, 0, None, 0, ctypes.byref(total), None) == 0 and total.value == 0
    ok = (1000, 1, fv, first, num, 1080, 1920, scratch, plan, ctypes.byref(total))
    for at, value, word in ((0, -1, "negative"), (1, -1, "negative"), (0, (1 << 31) - 1, "2^31"), (5, 0, "16384"), (5, 16385, "16384"),
                            (6, 0, "16384"), (6, 16385, "16384"), (2, None, "null"), (3, None, "null"), (4, None, "null"), (7, None, "null"),
                            (9, None, "null"), (2, fv + 2, "aligned"), (3, first + 4, "aligned"), (4, num + 4, "aligned"),
                            (7, scratch + 128, "aligned"), (8, plan - 1, "scratch too small")):
        args = list(ok)
        args[at] = value
        assert count_refused(*args, word=word), (at, value)

    def refused(*args, word):
        return L.gsr_mesh_raster(*args, None) != 0 and word in _lib.last_error()

    pair_bytes = L.gsr_mesh_raster_pair_bytes(5000)
    ok = [1000, 1, fv, first, num, nbr, 1080, 1920, 0.0, 10, 1, 0, 0, scratch, plan, 5000, pairs, pair_bytes, face, z, bary, dists]
    for at, value, word in ((9, 0, "K = 0"), (9, 17, "K = 17"), (8, 1e-4, "blur_radius"), (8, float("nan"), "blur_radius"), (6, 0, "16384"),
                            (6, 16385, "16384"), (7, 0, "16384"), (7, 16385, "16384"), (0, -1, "negative"), (1, -1, "negative"),
                            (0, (1 << 31) - 1, "2^31"), (15, -1, "negative"), (15, 1 << 31, "2^31"),
                            (2, None, "null"), (3, None, "null"), (4, None, "null"), (5, None, "null"), (13, None, "null"), (16, None, "null"),
                            (18, None, "null"), (19, None, "null"), (20, None, "null"), (21, None, "null"),
                            (2, fv + 1, "aligned"), (3, first + 4, "aligned"), (4, num + 2, "aligned"), (5, nbr + 4, "aligned"),
                            (13, scratch + 64, "aligned"), (16, pairs + 128, "aligned"), (18, face + 4, "aligned"), (19, z + 2, "aligned"),
                            (20, bary + 1, "aligned"), (21, dists + 3, "aligned"),
                            (14, plan - 1, "plan scratch too small"), (17, pair_bytes - 1, "pair scratch too small")):
        args = list(ok)
        args[at] = value
        assert refused(*args, word=word), (at, value)
    # N == 0: nothing to do, nothing read
    assert L.gsr_mesh_raster(0, 0, None, None, None, None, 8, 8, 0.0, 1, 0, 0, 0, None, 0, 0, None, 0, None, None, None, None, None) == 0
    # F == 0 still needs somewhere to write the -1s
    assert refused(0, 1, None, None, None, None, 8, 8, 0.0, 1, 0, 0, 0, None, 0, 0, None, 0, None, z, bary, dists, word="null")
