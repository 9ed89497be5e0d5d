"""pytorch3d's rasterize_meshes on the GPU (gsr_meshraster.hip through autovfx_amd.meshraster.rasterize_face_verts): bit for bit the
numpy restatement of the contract -- the same IEEE operations in the same order, contraction off, no transcendental -- on the scenes of
tests/meshraster_cases.py at every slot bucket and flag, at the sizes where the kernels change path, and through the hook.  Every GPU
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
CHUNK = 256                 # faces per LDS chunk of the raster kernel (gsr_meshraster.hip: kMeshChunk)
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


@pytest.mark.parametrize("K", [10, 16])
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
