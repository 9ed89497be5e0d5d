"""pytorch3d's rasterize_meshes on the GPU (gsr_meshraster.hip through autovfx_amd.meshraster.rasterize_face_verts): bit for bit the
numpy restatement of the contract -- the same IEEE operations in the same order, contraction off, no transcendental -- on the scenes of
tests/meshraster_cases.py at every slot bucket and flag, at the sizes where the kernels change path (a second round of the scan, the
64-tile bound of a wave-walked rectangle, the edges of the slot buckets, ties and neighbour pairs across LDS chunks), at and behind the
camera plane, on finite coordinates that overflow the intermediates, and through the hook.  Every GPU
result is read after ``torch.cuda.synchronize()``, which raises if a kernel faulted: a fault fails the test that caused it."""
from __future__ import annotations

import ctypes
import functools
import sys
import types

import numpy as np
import pytest
import torch

import meshraster_cases as cases
from autovfx_amd import hook, meshraster
from autovfx_amd.meshraster import rasterize_face_verts, rasterize_face_verts_host
from meshraster_cases import one_mesh, tri_around

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
CHUNK = cases.CHUNK         # faces per LDS chunk of the raster kernel (gsr_meshraster.hip: kMeshChunk)
FLAGS = [(False, False, False), (True, False, False), (False, True, False), (True, True, False), (True, False, True)]   # perspective, clip, cull


def _device(fv, first, num, nbr):
    return (torch.tensor(np.asarray(fv, F), device=DEV), *(torch.tensor(np.asarray(a, np.int64), device=DEV) for a in (first, num, nbr)))


def _run(fv, first, num, nbr, size, K, flags=(False, False, False)):
    out = rasterize_face_verts(*_device(fv, first, num, nbr), size, 0.0, K, None, 50_000, *flags)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


def _want(fv, first, num, nbr, size, K, flags=(False, False, False)):
    return rasterize_face_verts_host(fv, first, num, nbr, size, 0.0, K, None, None, *flags)


def _bits(a):
    return a.view(np.int32) if a.dtype == F else a


def _assert_bit_equal(got, want, label=""):
    for name, g, w in zip(("pix_to_face", "zbuf", "bary_coords", "dists"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (label, name, g.shape, w.shape, g.dtype)
        differ = _bits(g) != _bits(w)
        assert not differ.any(), f"{label}: {name} differs in {int(differ.sum())} of {differ.size} elements, first at {tuple(np.argwhere(differ)[0])}"


def _check(fv, first, num, nbr, size, K, flags=(False, False, False), label=""):
    want = _want(fv, first, num, nbr, size, K, flags)
    _assert_bit_equal(_run(fv, first, num, nbr, size, K, flags), want, label)
    return want


@functools.lru_cache(maxsize=None)
def _scene_want(index, K, flags):
    H, W, n_faces, seed = cases.SCENES[index]
    fv = cases.scene(n_faces, seed)
    return fv, _want(fv, *one_mesh(fv), (H, W), K, flags)


@pytest.mark.parametrize("K", [1, 4, 10, 16])
@pytest.mark.parametrize("index", range(len(cases.SCENES)))
def test_bit_equal_to_the_restatement_on_the_scenes(index, K):
    """H and W are no multiples of the tile on three of the four scenes; 10 sits in the 16-slot bucket with six slots to spare."""
    H, W, _n, _seed = cases.SCENES[index]
    for flags in FLAGS:
        fv, want = _scene_want(index, K, flags)
        _assert_bit_equal(_run(fv, *one_mesh(fv), (H, W), K, flags), want, f"scene {index}, K={K}, flags={flags}")


@pytest.mark.parametrize("index", range(len(cases.SCENES)))
def test_scenes_against_the_float64_truth(index):
    """What holds the kernels to the contract and not only to its restatement: SuGaR's setting (K = 10, perspective_correct) against the
    brute-force float64 evaluation, identical faces on every decided pixel and the bars of meshraster_cases."""
    H, W, _n, _seed = cases.SCENES[index]
    fv, want = cases.scene_truth(index, 10, True)
    ez, eb, ed = cases.against_truth(_run(fv, *one_mesh(fv), (H, W), 10, (True, False, False)), want, f"scene {index}")
    assert ez <= cases.BAR_Z and eb <= cases.BAR_BARY and ed <= cases.BAR_DIST


@pytest.mark.parametrize("size", [(1, 1), (16, 16), (17, 1), (1, 33)])
def test_tiny_and_exact_tile_images(size):
    fv = cases.scene(300, 9)
    want = _check(fv, *one_mesh(fv), size, 10, (True, False, False), f"{size}")
    if size[0] == size[1]:
        assert (want[0][..., 1] >= 0).all()                  # the two screen-filling faces reach every pixel of a square image


def test_a_tile_list_of_three_chunks():
    g = np.random.default_rng(5)
    n = 3 * CHUNK + 5
    fv = np.stack([tri_around(x, y, z, r=0.03) for x, y, z in zip(g.uniform(0.55, 0.95, n), g.uniform(0.55, 0.95, n), g.uniform(1, 2, n))])
    want = _check(fv, *one_mesh(fv), (64, 64), 10, label="three chunks")
    in_tile = want[0][0, :16, :16]
    assert len(np.unique(in_tile[in_tile >= 0])) > 2 * CHUNK  # faces of all three chunks are in somebody's ten nearest
    assert (in_tile >= 0).all(-1).any() and (want[0][0, 17:, 17:] == -1).all()


@pytest.mark.parametrize("K", [5, 8, 10, 16])
def test_more_layers_than_slots_come_out_nearest_first(K):
    g = np.random.default_rng(6)
    depth = g.permutation(24) + 1.0
    fv = np.stack([np.array([(-3, -3, z), (3, -3, z), (0, 4, z)], F) for z in depth])
    face, z, _b, _d = _run(fv, *one_mesh(fv), (20, 20), K)
    assert np.allclose(z, np.arange(1, K + 1, dtype=F), rtol=0, atol=1e-5)
    assert np.array_equal(face, np.broadcast_to(np.argsort(depth)[:K], face.shape))
    _check(fv, *one_mesh(fv), (20, 20), K, (True, True, False), "layers")


def test_exact_ties_go_by_the_lower_index():
    fv = np.stack([np.array([(-3, -3, 2), (3, -3, 2), (0, 4, 2)], F)] * 20)
    face = _check(fv, *one_mesh(fv), (20, 20), 16, label="ties")[0]
    assert np.array_equal(face, np.broadcast_to(np.arange(16), face.shape))


def test_rectangles_walked_by_the_wave():
    """150 x 140 pixels are 10 x 9 tiles: the screen-filling faces' rectangles are above the 64 tiles a lane walks alone."""
    fv = cases.scene(40, 11)
    fv[5], fv[39] = fv[0], fv[1]
    fv[5, :, 2] = 0.1                                        # in front of everything
    want = _check(fv, *one_mesh(fv), (150, 140), 4, (True, False, False), "wave-walked rectangles")
    assert (want[0][..., 0] == 5).all() and (want[0][..., 3] >= 0).all()


def test_neighbour_rule():
    fv = np.stack([tri_around(0, 0, 1, r=0.95), tri_around(0.25, 0.25, 2, r=0.6), tri_around(0, 0, 3, r=0.9)])
    first, num = np.array([0], np.int64), np.array([3], np.int64)
    free = _check(fv, first, num, np.full(3, -1, np.int64), (40, 40), 4, label="no neighbours")[0]
    paired = _check(fv, first, num, np.array([1, 0, -1], np.int64), (40, 40), 4, label="neighbours")[0]
    both = (free[0, :, :, 0] == 0) & (free[0, :, :, 1] == 1)
    assert both.sum() > 100 and ((paired[0] == 0).any(-1) & (paired[0] == 1).any(-1)).sum() == 0
    assert set(np.unique(paired[0, :, :, 0][both])) == {0, 1}                            # each of the two wins somewhere


def test_two_meshes():
    fv = cases.scene(200, 3)
    first, num, nbr = np.array([0, 150], np.int64), np.array([150, 50], np.int64), np.full(200, -1, np.int64)
    want = _check(fv, first, num, nbr, (33, 20), 4, (True, False, False), "N=2")
    assert want[0][0].max() < 150 <= want[0][1][want[0][1] >= 0].min()


# ---- where the kernels change path ----------------------------------------------------------------------------------------------------

def _pair_total(fv, first, num, size):
    """The count step alone: the number of (tile, face) pairs of the plan."""
    from autovfx_amd import _lib
    t_fv, t_first, t_num, _nbr = _device(fv, first, num, np.zeros(len(fv), np.int64))
    plan, plan_bytes = _lib.scratch("gsr_mesh_raster_plan_bytes", len(fv), len(first), *size, device=torch.device(DEV))
    total = ctypes.c_int64(-1)
    _lib.call("gsr_mesh_raster_count", len(fv), len(first), t_fv.data_ptr(), t_first.data_ptr(), t_num.data_ptr(), *size, 0, plan.data_ptr(), plan_bytes,
              ctypes.byref(total), device=torch.device(DEV))
    torch.cuda.synchronize()
    return total.value


@pytest.mark.parametrize("n_meshes", [1024, 1025])
def test_many_small_meshes_fill_one_scan_round_and_start_another(n_meshes):
    """17 x 17 images are 4 tiles each: 1024 meshes are the 4096 tiles of one round of the scan, 1025 carry its running sum into a second."""
    fv, first, num, nbr = cases.many_small_meshes(n_meshes)
    assert (n_meshes * 4 > cases.SCAN_ROUND) == (n_meshes == 1025)
    face = _check(fv, first, num, nbr, (17, 17), 4, label=f"{n_meshes} meshes")[0]
    for n in (1023, n_meshes - 1):
        assert (face[n] >= 3 * n).any() and face[n].max() < 3 * n + 3


def test_one_image_of_two_scan_rounds():
    """1041 x 1041 is 66 x 66 = 4356 tiles with a last tile row and column one pixel wide: the screen-filling faces are one wave-walked
    rectangle over the tiles of both rounds, the small faces sit in the last pixel row and column."""
    fv = cases.large_image_faces(1041)
    assert 66 * 66 > cases.SCAN_ROUND
    face = _check(fv, *one_mesh(fv), (1041, 1041), 4, (True, False, False), "1041 x 1041")[0][0]
    assert (face[..., 1] >= 0).all()
    assert set(range(2, 8)) <= set(np.unique(face[1040])) and set(range(8, 14)) <= set(np.unique(face[:, 1040]))


def test_waves_that_mix_every_kind_of_face_in_the_second_mesh():
    """150 x 140 is 10 x 9 tiles; 700 faces are three workgroups of the count and the fill, the last one ragged.  The wave-walked rectangles
    of mesh 1 carry ``base != 0`` from lanes of every position, next to lane-walked, culled and off-image lanes."""
    fv, first, num, nbr = cases.mixed_waves_two_meshes()
    face = _check(fv, first, num, nbr, (150, 140), 4, (True, False, False), "mixed waves")[0]
    assert face[0].max() < first[1] and (face[1] >= first[1]).all()           # mesh 1: four screen-filling faces over every pixel
    assert (face[0][..., :3] >= 0).all() and (face[0] == 130).any()           # mesh 0: its three
    kinds = cases.mixed_wave_kind(np.unique(face[1]))
    assert (kinds == 0).any() and (kinds >= 4).any() and not np.isin(kinds, (1, 2, 3)).any()


def test_rectangles_of_64_tiles_and_of_72():
    """The bound between a rectangle its lane walks (64 tiles) and one the wave walks (more); the spans are worked out in meshraster_cases."""
    three = cases.rect_bound_faces()
    assert [_pair_total(three[i:i + 1], *one_mesh(three[:1])[:2], (160, 160)) for i in range(3)] == [64, 72, 72]
    assert 64 == cases.WAVE_RECT
    fv = cases.rect_bound_scene()
    face = _check(fv, *one_mesh(fv), (160, 160), 4, label="the 64-tile bound")[0]
    assert all((face == f).any() for f in (7, 8, 100))


@pytest.mark.parametrize("K", [2, 3, 5, 8, 9, 15])
def test_slot_counts_inside_and_at_the_edges_of_the_buckets(K):
    """Buckets of 1, 4, 8 and 16 slots: 2 and 3 leave slots of bucket 4 unused, 5 and 8 are the two ends of bucket 8, 9 and 15 sit in 16."""
    H, W, _n, _seed = cases.SCENES[3]
    for flags in FLAGS:
        fv, want = _scene_want(3, K, flags)
        _assert_bit_equal(_run(fv, *one_mesh(fv), (H, W), K, flags), want, f"K={K}, flags={flags}")
    assert (_scene_want(3, K, FLAGS[0])[1][0][..., K - 1] >= 0).any()            # the last slot is in use


@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("K", [16, 1])
def test_a_tie_longer_than_two_chunks(K, interleaved):
    """The order of a tile's list comes from the fill's atomics; (depth, index) ordering must make it immaterial, run after run."""
    fv, expected = cases.long_tie(interleaved)
    want = _want(fv, *one_mesh(fv), (64, 64), K)
    covered = want[0][0, :, :, 0] >= 0
    assert covered.sum() > 20 and np.array_equal(want[0][0][covered], np.broadcast_to(expected[:K], (covered.sum(), K)))
    for run in range(2):
        _assert_bit_equal(_run(fv, *one_mesh(fv), (64, 64), K), want, f"run {run}")


def test_a_tie_between_lane_walked_and_wave_walked_faces():
    """A tie whose list order is known not to be the index order: see meshraster_cases.tie_of_two_walks."""
    fv, size, both, wide_only = cases.tie_of_two_walks()
    want = _want(fv, *one_mesh(fv), size, 16)
    assert (want[1][want[0] >= 0] == 2.0).all()                                   # the tie is exact
    assert np.array_equal(want[0][0][:, both], np.broadcast_to(np.arange(16), (size[0], both.sum(), 16)))
    assert np.array_equal(want[0][0][:, wide_only], np.broadcast_to(2 * np.arange(16), (size[0], wide_only.sum(), 16)))
    for run in range(2):
        _assert_bit_equal(_run(fv, *one_mesh(fv), size, 16), want, f"run {run}")


NEAR_PLANE_SIZES = ((37, 53, 300, 101), (64, 48, 600, 102))


@pytest.mark.parametrize("H, W, n_faces, seed", NEAR_PLANE_SIZES)
def test_near_plane_scene_bit_equal_under_every_flag(H, W, n_faces, seed):
    """Depths at and behind the camera plane: the eps clamp of the perspective denominator, a clip that changes the barycentrics and the
    ``pz < 0`` skip all decide something here."""
    fv = cases.near_plane_scene(n_faces, seed)
    want = {flags: _check(fv, *one_mesh(fv), (H, W), 10, flags, f"near plane {H}x{W}, flags={flags}") for flags in FLAGS}
    plain, perspective = want[FLAGS[0]], want[FLAGS[1]]
    assert (plain[1][plain[0] >= 0] < 0.05).any() and (perspective[1][perspective[0] >= 0] < 0.05).any()
    assert (perspective[0] >= 0).sum() < (plain[0] >= 0).sum()                    # negative depths that only the correction produces
    assert not all(np.array_equal(a, b) for a, b in zip(want[FLAGS[1]], want[FLAGS[3]]))   # the clip changes something


@pytest.mark.parametrize("index", range(len(cases.NEAR_PLANE)))
def test_near_plane_scene_against_the_float64_truth(index):
    """As tests/test_meshraster.py::test_near_plane_restatement_against_truth, on the kernels.  Perspective without the clip: only the faces,
    for the reason given there."""
    H, W, _n, _seed = cases.NEAR_PLANE[index]
    for flags in ((False, False), (True, True)):
        fv, want = cases.near_plane_truth(index, *flags)
        ez, eb, ed = cases.against_truth(_run(fv, *one_mesh(fv), (H, W), 10, (*flags, False)), want, f"near plane {index}, {flags}")
        assert ez <= cases.NEAR_BAR_Z and eb <= cases.NEAR_BAR_BARY and ed <= cases.NEAR_BAR_DIST
    fv, want = cases.near_plane_truth(index, True, False)
    got = _run(fv, *one_mesh(fv), (H, W), 10, (True, False, False))
    decided = ~want[4]
    assert want[4].mean() <= cases.MAX_UNDECIDED and np.array_equal(got[0][decided], want[0][decided])


def test_a_face_that_names_itself():
    case = cases.neighbour_names_itself()
    want = _check(*case, (40, 40), 4, label="nbr[f] == f")
    _assert_bit_equal(want, _want(*case[:3], np.full(3, -1, np.int64), (40, 40), 4), "as without neighbours")


def test_a_culled_neighbour():
    case = cases.neighbour_is_culled()
    flags = (False, False, True)
    want = _check(*case, (40, 40), 4, flags, "culled neighbours")
    _assert_bit_equal(want, _want(*case[:3], np.full(4, -1, np.int64), (40, 40), 4, flags), "as without neighbours")
    assert set(np.unique(want[0])) == {-1, 0, 1}
    assert set(np.unique(_want(*case, (40, 40), 4)[0])) == {-1, 0, 1, 2}         # without the cull the back face is there


def test_a_neighbour_in_the_other_mesh():
    fv, first, num, nbr = cases.neighbour_in_the_other_mesh()
    face = _check(fv, first, num, nbr, (40, 40), 4, label="N=2 neighbours")[0]
    free = _want(fv, first, num, np.full(5, -1, np.int64), (40, 40), 4)[0]
    assert np.array_equal(face[0], free[0])                                       # mesh 0: naming face 3 of mesh 1 changes nothing
    assert np.array_equal((face[1] == 4).any(-1), (free[1] == 4).any(-1))         # mesh 1: nor does face 4's naming face 1 of mesh 0
    both = (free[1] == 2).any(-1) & (free[1] == 3).any(-1)
    assert both.sum() > 100 and not ((face[1] == 2).any(-1) & (face[1] == 3).any(-1)).any()
    assert set(np.unique(face[1, :, :, 0][both])) == {2, 3}                       # the pair inside mesh 1: each wins somewhere


def test_neighbours_that_are_no_face():
    case = cases.neighbour_out_of_range()
    want = _check(*case, (40, 40), 4, label="nbr out of range")
    _assert_bit_equal(want, _want(*case[:3], np.full(4, -1, np.int64), (40, 40), 4), "as without neighbours")


def test_twins_that_name_each_other():
    case = cases.neighbour_is_a_twin()
    face = _check(*case, (40, 40), 4, label="twins")[0]
    free = _want(*case[:3], np.full(3, -1, np.int64), (40, 40), 4)[0]
    both = (free == 0).any(-1)
    assert both.sum() > 100 and np.array_equal(both, (free == 1).any(-1))
    assert np.array_equal((face == 0).any(-1), both) and not (face == 1).any()   # equal distances: exactly the lower index stays


def test_a_pair_in_different_chunks_of_a_list():
    fv, first, num, nbr = cases.neighbour_across_chunks()
    last = len(fv) - 1
    face = _check(fv, first, num, nbr, (64, 64), 4, label="a pair across chunks")[0]
    free = _want(fv, first, num, np.full(len(fv), -1, np.int64), (64, 64), 4)[0]
    both = (free == 0).any(-1) & (free == last).any(-1)
    assert both.sum() > 20 and not ((face == 0).any(-1) & (face == last).any(-1)).any()
    assert set(np.unique(face[..., 0][both])) == {0, last}


HUGE = ((1e19, 1.0), (1e25, 1.0), (1e38, 1.0), (1.0, 1e18), (1.0, 1e20))        # z times, xy times


@pytest.mark.parametrize("z_scale, xy_scale", HUGE)
def test_huge_finite_coordinates(z_scale, xy_scale):
    """Finite inputs whose intermediates overflow to infinities and NaN: the contract's ``min`` and ``max`` are ``fminf`` and ``fmaxf``, a NaN
    depth is never listed and an infinite one comes last."""
    H, W, n_faces, seed = cases.SCENES[0]
    fv = cases.scaled_scene(n_faces, seed, z_scale, xy_scale)
    assert np.isfinite(fv).all()
    for flags in FLAGS:
        _check(fv, *one_mesh(fv), (H, W), 10, flags, f"z x {z_scale:g}, xy x {xy_scale:g}, flags={flags}")


@pytest.mark.parametrize("K", [4, 16])
def test_non_finite_vertices_leave_the_finite_faces_alone(K):
    """Outside the contract, but the kernels must finish (the sync raises otherwise) and the finite faces keep their order and values."""
    H, W, n_faces, seed = cases.SCENES[0]
    broken, finite_only, is_broken = cases.non_finite_scene(n_faces, seed)
    for flags in FLAGS:
        want = _want(finite_only, *one_mesh(finite_only), (H, W), K, flags)
        held = cases.finite_faces_are_a_prefix(_run(broken, *one_mesh(broken), (H, W), K, flags), want, is_broken, f"K={K}, flags={flags}")
        print(f"K={K}, flags={flags}: {held} slots hold a non-finite face")


def test_no_faces_and_no_meshes():
    out = _run(np.zeros((0, 3, 3), F), [0], [0], np.zeros(0, np.int64), (5, 7), 2)
    assert [o.shape for o in out] == [(1, 5, 7, 2), (1, 5, 7, 2), (1, 5, 7, 2, 3), (1, 5, 7, 2)] and all((o == -1).all() for o in out)
    out = _run(np.zeros((0, 3, 3), F), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64), (5, 7), 2)
    assert [o.shape for o in out] == [(0, 5, 7, 2), (0, 5, 7, 2), (0, 5, 7, 2, 3), (0, 5, 7, 2)]
    culled = np.stack([tri_around(0, 0, -1.0, r=0.5)] * 3)                               # faces, but none that survives: empty lists
    out = _run(culled, *one_mesh(culled), (20, 20), 3)
    assert all((o == -1).all() for o in out)


def test_a_non_default_stream():
    fv, want = _scene_want(3, 10, (True, False, False))
    args = _device(fv, *one_mesh(fv))
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):
        out = rasterize_face_verts(*args, (64, 48), 0.0, 10, None, None, True, False, False)
    stream.synchronize()
    _assert_bit_equal(tuple(o.cpu().numpy() for o in out), want, "side stream")
    torch.cuda.synchronize()


@pytest.mark.parametrize("n_faces", [0, 1000])
def test_every_output_element_is_written(n_faces):
    """The C ABI on outputs pre-filled with garbage, and on scratch full of it."""
    from autovfx_amd import _lib
    H, W, K = 64, 48, 10
    fv = cases.scene(1000, 4)[:n_faces]
    want = _want(fv, *one_mesh(fv), (H, W), K, (True, False, False))
    t_fv, first, num, nbr = _device(fv, *one_mesh(fv))
    outs = [torch.full((1, H, W, K), 0x7A7A7A7A7A7A7A7A, dtype=torch.int64, device=DEV), torch.full((1, H, W, K), float("nan"), device=DEV),
            torch.full((1, H, W, K, 3), float("nan"), device=DEV), torch.full((1, H, W, K), float("nan"), device=DEV)]
    ptrs = [o.data_ptr() for o in outs]
    if n_faces == 0:
        _lib.call("gsr_mesh_raster", 0, 1, None, None, None, None, H, W, 0.0, K, 1, 0, 0, None, 0, 0, None, 0, *ptrs, device=torch.device(DEV))
    else:
        plan_bytes = _lib.lib.gsr_mesh_raster_plan_bytes(n_faces, 1, H, W)
        plan = torch.full((plan_bytes,), 0xAB, dtype=torch.uint8, device=DEV)
        total = ctypes.c_int64(-1)
        _lib.call("gsr_mesh_raster_count", n_faces, 1, t_fv.data_ptr(), first.data_ptr(), num.data_ptr(), H, W, 0, plan.data_ptr(), plan_bytes,
                  ctypes.byref(total), device=torch.device(DEV))
        assert n_faces <= total.value <= 12 * n_faces                                    # 4 x 3 tiles
        pair_bytes = _lib.lib.gsr_mesh_raster_pair_bytes(total.value)
        pairs = torch.full((pair_bytes,), 0xCD, dtype=torch.uint8, device=DEV)
        _lib.call("gsr_mesh_raster", n_faces, 1, t_fv.data_ptr(), first.data_ptr(), num.data_ptr(), nbr.data_ptr(), H, W, 0.0, K, 1, 0, 0,
                  plan.data_ptr(), plan_bytes, total.value, pairs.data_ptr(), pair_bytes, *ptrs, device=torch.device(DEV))
        # the same plan again, with one slot and the other flags: a count serves any number of raster calls
        again = [torch.full((1, H, W, 1), -7, dtype=torch.int64, device=DEV), torch.full((1, H, W, 1), float("nan"), device=DEV),
                 torch.full((1, H, W, 1, 3), float("nan"), device=DEV), torch.full((1, H, W, 1), float("nan"), device=DEV)]
        _lib.call("gsr_mesh_raster", n_faces, 1, t_fv.data_ptr(), first.data_ptr(), num.data_ptr(), nbr.data_ptr(), H, W, 0.0, 1, 0, 1, 0,
                  plan.data_ptr(), plan_bytes, total.value, pairs.data_ptr(), pair_bytes, *(o.data_ptr() for o in again), device=torch.device(DEV))
        torch.cuda.synchronize()
        _assert_bit_equal(tuple(o.cpu().numpy() for o in again), _want(fv, *one_mesh(fv), (H, W), 1, (False, True, False)), "the plan's second use")
    torch.cuda.synchronize()
    _assert_bit_equal(tuple(o.cpu().numpy() for o in outs), want, f"{n_faces} faces over garbage")


def test_through_the_hook():
    """A stub ``pytorch3d._C``: a taken call never reaches the original, a CPU call and a blurred call do."""
    names = ("pytorch3d", "pytorch3d._C")
    saved = {k: sys.modules.pop(k) for k in names if k in sys.modules}
    calls = []

    def rasterize_meshes(*args):
        calls.append(args)
        return "the original's result"

    root, leaf = (types.ModuleType(n) for n in names)
    leaf.rasterize_meshes, leaf.rasterize_meshes_backward = rasterize_meshes, (lambda *a: None)
    root._C = leaf
    sys.modules.update(zip(names, (root, leaf)))
    path = list(sys.path)
    try:
        hook.install(path=False)
        fv, want = _scene_want(0, 10, (True, False, False))
        args = _device(fv, *one_mesh(fv))
        out = root._C.rasterize_meshes(*args, (37, 53), 0.0, 10, None, 50_000, True, False, False)
        torch.cuda.synchronize()
        assert calls == []
        _assert_bit_equal(tuple(o.cpu().numpy() for o in out), want, "through the hook")
        assert root._C.rasterize_meshes(*args, (37, 53), 1e-4, 10, None, 50_000, True, False, False) == "the original's result"
        cpu = tuple(a.cpu() for a in args)
        assert root._C.rasterize_meshes(*cpu, (37, 53), 0.0, 10, None, 50_000, True, False, False) == "the original's result"
        assert len(calls) == 2 and calls[0][5] == 1e-4 and calls[1][0] is cpu[0]
        with pytest.raises(ValueError, match="blur_radius"):
            meshraster.rasterize_face_verts(*args, (37, 53), 1e-4, 10)
    finally:
        hook.uninstall()
        sys.path[:] = path
        for k in names:
            sys.modules.pop(k, None)
        sys.modules.update(saved)
