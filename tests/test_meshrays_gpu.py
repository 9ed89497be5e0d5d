"""The first-hit kernel (gsr_meshquery.hip: ray_hit_kernel) against the numpy restatement of its contract (meshquery.first_hits_host),
bit for bit: the face index, the bits of t and of the barycentrics -- at every face count where the tree changes shape, at the wave's
edges in the ray count, from inside and outside a mesh, and through the layers above the kernel."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from autovfx_amd import extract, meshquery
from autovfx_amd.meshquery import first_hits_host

import meshquery_cases as cases
import meshrays_cases as rays

pytestmark = pytest.mark.gpu
F32 = np.float32
DEV = "cuda:0"


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _points_host(o, d, face, t):
    """``o + t d`` as a multiplication and an addition in fp32, zeros on a miss."""
    hit = face >= 0
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(hit[:, None], o + np.where(hit, t, F32(0))[:, None] * d, F32(0)).astype(F32)


def assert_same_bits(got, want, what=""):
    got = [t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in got]
    assert got[0].dtype == np.int64 and all(g.dtype == F32 for g in got[1:])
    bad = np.nonzero(got[0] != want[0])[0]
    assert bad.size == 0, (what, "face_idx", bad[:5], got[0][bad[:5]], want[0][bad[:5]], got[1][bad[:5]], want[1][bad[:5]])
    bad = np.nonzero(_bits(got[1]) != _bits(want[1]))[0]
    assert bad.size == 0, (what, "t", bad[:5], got[1][bad[:5]], want[1][bad[:5]])
    for name, g, w in zip(("bary", "points"), got[2:], want[2:]):
        bad = np.nonzero((_bits(g) != _bits(w)).any(axis=1))[0]
        assert bad.size == 0, (what, name, bad[:5], g[bad[:5]], w[bad[:5]])


def _on_gpu(*arrays):
    return tuple(torch.tensor(a, device=DEV) for a in arrays)


def check(o, d, verts, faces, what="", pruned=False):
    face, t, bary = first_hits_host(o, d, verts, faces, pruned=pruned)
    want = (face, t, bary, _points_host(o, d, face, t))
    to, td, tv, tf = _on_gpu(o, d, verts, faces)
    got = meshquery.first_hits(to, td, tv, tf, return_bary=True, return_points=True)
    assert_same_bits(got, want, what)
    # (above: asked in a coherent order and put back; here: in the caller's order -- an answer is a function of its own ray alone)
    assert_same_bits(meshquery._cast(to, td, meshquery.plan(tv, tf), True, order=None), want[:3], what + ", caller's order")
    short = meshquery.first_hits(to, td, tv, tf)                    # bary = NULL: the same ids and t
    assert len(short) == 2 and torch.equal(short[0], got[0]) and torch.equal(short[1].view(torch.int32), got[1].view(torch.int32))
    return want


def _rays_for(verts, faces, n, seed):
    """Inside, outside with hits, outside with misses (rays.mixed_rays), then the rays that answer nothing by themselves."""
    ok = np.isfinite(verts).all(1)
    o, d = rays.mixed_rays(verts[ok], n, seed)
    bad_o, bad_d = o[:6].copy(), d[:6].copy()
    bad_o[0, 1], bad_o[1, 0], bad_d[2, 2], bad_d[3, 0], bad_d[4], bad_d[5] = np.nan, np.inf, np.nan, -np.inf, 0.0, (0.0, -0.0, 0.0)
    return np.concatenate((o, bad_o)), np.concatenate((d, bad_d))


# ---- the tree's shape changes, the wave's edges ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 63, 64, 65, 1025, 16385])
def test_every_tree_shape(F):
    """One leaf, the leaf seam, trees of two and three levels; a rippled sphere (a ray from inside crosses several folds)."""
    verts, faces = rays.rippled_sphere(F, seed=F)
    o, d = _rays_for(verts, faces, 270, seed=F + 1)
    want = check(o, d, verts, faces, f"F = {F}", pruned=F > 2000)
    hits = int((want[0] >= 0).sum())
    assert (want[0][-6:] == -1).all() and hits < 270 and (hits >= 100 if F >= 1025 else hits >= (1 if F > 1 else 0))


@functools.lru_cache(maxsize=None)
def _wave_case():
    verts, faces = rays.icosphere(3)                                 # closed: every finite ray from inside hits
    verts = (verts + np.asarray((0.3, -0.2, 0.5), F32)).astype(F32)
    g = np.random.default_rng(12)
    away = g.normal(size=(64, 3))
    away = (4.0 * away / np.linalg.norm(away, axis=1, keepdims=True)).astype(F32)
    inside_d = g.normal(size=(193, 3)).astype(F32)
    inside_o = (np.asarray((0.3, -0.2, 0.5)) + 0.4 * g.uniform(-1, 1, (193, 3))).astype(F32)
    # a whole wave of misses (from outside, pointing away) first, then rays from inside
    o = np.concatenate((away + np.asarray((0.3, -0.2, 0.5), F32), inside_o)).astype(F32)
    d = np.concatenate((away, inside_d))
    return o, d, verts, faces, first_hits_host(o, d, verts, faces)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_every_wave_edge(n):
    """A partial wave, a full one, a second one of one lane, a workgroup whose fourth wave is partial and one more; the first 64 rays
    all miss (a wave with nothing to walk for), the others all hit."""
    o, d, verts, faces, want = _wave_case()
    assert (want[0][:64] == -1).all() and (want[0][64:] >= 0).all()
    for start in (0, 64):                                           # from the missing wave, and past it
        if start + n > len(o):
            continue
        sl = slice(start, start + n)
        to, td, tv, tf = _on_gpu(o[sl], d[sl], verts, faces)
        expect = tuple(w[sl] for w in want)
        assert_same_bits(meshquery._cast(to, td, meshquery.plan(tv, tf), True, order=None), expect, f"n = {n} from {start}")
        assert_same_bits(meshquery.first_hits(to, td, tv, tf, return_bary=True), expect, f"n = {n} from {start}, sorted")


def test_sorted_and_unsorted_answers_are_identical():
    o, d, verts, faces, want = _wave_case()
    to, td, tv, tf = _on_gpu(o, d, verts, faces)
    plan = meshquery.plan(tv, tf)
    order = meshquery.ray_order(to, td, tv)
    assert order.shape == (len(o),) and torch.equal(torch.sort(order).values, torch.arange(len(o), device=DEV))
    a = meshquery._cast(to, td, plan, True, order=order)
    b = meshquery._cast(to, td, plan, True, order=None)
    c = meshquery._cast(to, td, plan, True, order=torch.randperm(len(o), device=DEV, generator=torch.Generator(DEV).manual_seed(1)))
    for x, y, z in zip(a, b, c):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)) and torch.equal(x.view(torch.int32), z.view(torch.int32))
    assert_same_bits(a, want, "sorted")
    assert_same_bits(meshquery.first_hits(to, td, tv, tf, plan=plan, return_bary=True, sort=False), want, "first_hits(sort=False)")


def test_exact_ties_on_the_gpu():
    verts, faces = cases.plane_in_random_order(30, 20, seed=6)       # 1200 faces, integer coordinates: every tie is exact
    at = [(float(i), float(j)) for i in range(31) for j in range(21)] + [(i + 0.5, j + 0.5) for i in range(30) for j in range(20)]
    o = np.array([(x, y, 2.0) for x, y in at], F32)
    d = np.broadcast_to(np.array([0, 0, -4.0], F32), o.shape).copy()
    check(o, d, verts, faces, "plane")
    check(o, d, verts, np.concatenate((faces, faces[::-1])), "every face duplicated")


def test_invalid_faces_are_never_hit():
    verts, faces, bad = cases.sphere_with_invalid(1800, 300, seed=14)
    o, d = _rays_for(verts, faces, 300, seed=15)
    want = check(o, d, verts, faces, "invalid faces mixed in")
    assert (want[0] >= 0).sum() >= 100 and not np.isin(want[0], bad).any()
    none = faces.copy()
    none[:, 0] = -1
    want = check(o, d, verts, none, "no valid face")
    assert (want[0] == -1).all() and np.isposinf(want[1]).all()
    check(o, d, verts, faces[:0], "no face")


# ---- the C entry point ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [0xFF, 0x55])
def test_every_output_element_is_written(fill):
    from autovfx_amd import _lib
    o, d, verts, faces, want = _wave_case()
    to, td, tv, tf = _on_gpu(o, d, verts, faces)
    plan = meshquery.plan(tv, tf)
    n = len(o)
    raw = [torch.full((k * n,), fill, dtype=torch.uint8, device=DEV) for k in (8, 4, 12)]
    _lib.call("gsr_ray_first_hit", n, to.data_ptr(), td.data_ptr(), plan.buffer.data_ptr(), plan.buffer.numel(), raw[0].data_ptr(),
              raw[1].data_ptr(), raw[2].data_ptr(), device=to.device)
    assert_same_bits((raw[0].view(torch.int64), raw[1].view(torch.float32), raw[2].view(torch.float32).reshape(n, 3)), want, f"fill {fill:#x}")


def test_a_header_that_does_not_match_answers_nothing():
    from autovfx_amd import _lib
    o, d, verts, faces, _ = _wave_case()
    to, td, tv, tf = _on_gpu(o[64:], d[64:], verts, faces)            # rays that all hit
    plan = meshquery.plan(tv, tf)
    cleared = plan.buffer.clone()
    cleared[:256] = 0
    other = plan.buffer.clone()
    other[:256] = meshquery.plan(tv, tf[:100]).buffer[:256]
    for name, buffer in (("cleared", cleared), ("of another mesh", other)):
        idx, t, bary = meshquery.first_hits(to, td, tv, tf, plan=meshquery.Plan(buffer, plan.F, plan.V), return_bary=True)
        assert bool((idx == -1).all()) and bool(torch.isposinf(t).all()) and bool((bary == 0).all()), name
    cut = plan.buffer[:plan.buffer.numel() // 512 * 256]
    with pytest.raises(ValueError, match="a plan of 1280 faces is"):
        meshquery.first_hits(to, td, tv, tf, plan=meshquery.Plan(cut, plan.F, plan.V))
    n = to.shape[0]
    idx = torch.full((n,), 7, dtype=torch.int64, device=DEV)
    t, bary = torch.zeros(n, device=DEV), torch.ones((n, 3), device=DEV)
    _lib.call("gsr_ray_first_hit", n, to.data_ptr(), td.data_ptr(), cut.data_ptr(), cut.numel(), idx.data_ptr(), t.data_ptr(), bary.data_ptr(),
              device=to.device)
    assert bool((idx == -1).all()) and bool(torch.isposinf(t).all()) and bool((bary == 0).all())


def test_every_refusal_of_the_entry_point_and_n_zero():
    """Addresses that are never read: every call is refused before a launch, and n == 0 looks at nothing."""
    from autovfx_amd import _lib
    L = _lib.lib
    n, origins, dirs, plan, ids, t, bary, pb = 300, 4096, 8192, 1 << 20, 1 << 16, 1 << 17, 1 << 18, 1 << 12

    def refused(*args, word):
        return L.gsr_ray_first_hit(*args, None) != 0 and word in _lib.last_error()

    assert L.gsr_ray_first_hit(0, None, None, None, 0, None, None, None, None) == 0
    assert L.gsr_ray_first_hit(0, origins + 1, dirs + 1, plan + 1, 7, ids + 1, t + 1, bary + 1, None) == 0
    assert refused(-1, origins, dirs, plan, pb, ids, t, bary, word="negative")
    assert refused(1 << 31, origins, dirs, plan, pb, ids, t, bary, word="2^31")
    for hole in range(5):
        ptrs = [origins, dirs, plan, ids, t]
        ptrs[hole] = None
        assert refused(n, ptrs[0], ptrs[1], ptrs[2], pb, ptrs[3], ptrs[4], bary, word="null"), hole
    for k in range(6):
        ptrs = [origins, dirs, plan, ids, t, bary]
        ptrs[k] += (2, 2, 16, 4, 2, 2)[k]
        assert refused(n, ptrs[0], ptrs[1], ptrs[2], pb, ptrs[3], ptrs[4], ptrs[5], word="aligned"), k
    for size in (0, 255, 257, pb + 1):
        assert refused(n, origins, dirs, plan, size, ids, t, bary, word="not the size of a plan"), size
    # ... and through Python: empty rays give empty answers, whatever the mesh
    verts, faces = rays.icosphere(1)
    tv, tf = _on_gpu(verts, faces)
    empty = torch.zeros((0, 3), device=DEV)
    got = meshquery.first_hits(empty, empty, tv, tf, return_bary=True, return_points=True)
    assert [tuple(x.shape) for x in got] == [(0,), (0,), (0, 3), (0, 3)] and got[0].dtype == torch.int64
    for bad, word in (((empty.cpu(), empty, tv, tf), "GPU"), ((empty.double(), empty, tv, tf), "float32"),
                      ((torch.zeros((2, 3), device=DEV), empty, tv, tf), "2 origins and 0 dirs"), ((empty, empty, tv, tf.int()), "int64")):
        with pytest.raises(ValueError, match=word):
            meshquery.first_hits(*bad)


def test_one_plan_serves_both_queries_and_closest_triangles_is_unchanged():
    o, d, verts, faces, want = _wave_case()
    to, td, tv, tf = _on_gpu(o, d, verts, faces)
    plan = meshquery.plan(tv, tf)
    snapshot = plan.buffer.clone()
    q = torch.tensor(cases.queries_near(verts, faces, 500, 0.3, seed=3), device=DEV)
    before = meshquery.closest_triangles(q, tv, tf, plan=plan, return_points=True)
    assert_same_bits(meshquery.first_hits(to, td, tv, tf, plan=plan, return_bary=True), want, "on the shared plan")
    after = meshquery.closest_triangles(q, tv, tf, plan=plan, return_points=True)
    assert torch.equal(plan.buffer, snapshot)
    for x, y in zip(before, after):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    host = meshquery.closest_triangles_host(q.cpu().numpy(), verts, faces)
    assert np.array_equal(before[0].cpu().numpy(), host[0]) and np.array_equal(_bits(before[1].cpu().numpy()), _bits(host[1]))


# ---- the layers above -----------------------------------------------------------------------------------------------------------------
def test_scene_cast_rays_and_ray_intersector():
    o, d, verts, faces, want = _wave_case()
    face, t, bary = want
    scene = meshquery.Scene(verts.astype(np.float64), faces.astype(np.int32), device=DEV)
    for r in (np.concatenate((o, d), 1), np.concatenate((o, d), 1).astype(np.float64), torch.tensor(np.concatenate((o, d), 1))):
        ans = scene.cast_rays(r)
        assert set(ans) == {"t_hit", "primitive_ids", "primitive_uvs"} and all(x.is_cuda for x in ans.values())
        assert ans["primitive_ids"].dtype == torch.int64 and tuple(ans["primitive_uvs"].shape) == (len(o), 2)
        assert_same_bits((ans["primitive_ids"], ans["t_hit"]), (face, t), "Scene.cast_rays")
        assert np.array_equal(_bits(ans["primitive_uvs"].cpu().numpy()), _bits(bary[:, 1:]))
    # Open3D's convention: the point is (1 - u - v) a + u b + v c
    uv = bary[64:, 1:].astype(np.float64)
    corners = verts[faces[face[64:]]].astype(np.float64)
    point = (1 - uv.sum(1))[:, None] * corners[:, 0] + uv[:, :1] * corners[:, 1] + uv[:, 1:] * corners[:, 2]
    assert np.abs(point - (o[64:] + t[64:, None] * d[64:])).max() <= 1e-5
    ray = meshquery.RayIntersector(verts, faces, device=DEV)
    first = ray.intersects_first(ray_origins=o, ray_directions=d)
    assert isinstance(first, np.ndarray) and first.dtype == np.int64 and np.array_equal(first, face)
    assert np.array_equal(ray.intersects_any(o.astype(np.float64), d), face >= 0)
    locations, index_ray, index_tri = ray.intersects_location(ray_origins=o, ray_directions=d, multiple_hits=False)
    hit = np.nonzero(face >= 0)[0]
    assert np.array_equal(index_ray, hit) and np.array_equal(index_tri, face[hit])
    assert np.array_equal(_bits(locations), _bits(_points_host(o, d, face, t)[hit]))
    with pytest.raises(NotImplementedError):
        ray.intersects_location(o, d, multiple_hits=True)


def _votes_host(verts, faces, masks, c2ws, K, h, w):
    """extract.triangle_votes in numpy on meshquery.first_hits_host.  The poses of the test are signed permutations with small
    integer translations and K has powers of two, so every product and sum of the ray set-up is exact whatever its order; the
    centres are projected in float64 and must stay clear of a pixel's edge (asserted)."""
    counter, naive = np.zeros(len(faces), np.int32), np.zeros(len(faces), np.int32)
    v, u = np.meshgrid(np.arange(h, dtype=F32), np.arange(w, dtype=F32), indexing="ij")
    directions = np.stack([(u - K[0, 2] + F32(0.5)) / K[0, 0], (v - K[1, 2] + F32(0.5)) / K[1, 1], np.ones_like(u)], -1)
    centres = verts.astype(np.float64)[faces].mean(1)
    for mask, c2w in zip(masks, c2ws):
        rays_d = (directions.astype(np.float64) @ c2w[:3, :3].astype(np.float64).T).astype(F32)
        assert np.array_equal(rays_d.astype(np.float64), directions.astype(np.float64) @ c2w[:3, :3].astype(np.float64).T)   # exact
        rays_o = np.broadcast_to(c2w[:3, 3], rays_d.shape)
        index_tri = first_hits_host(rays_o[mask], rays_d[mask], verts, faces)[0]
        assert (index_tri < 0).any() and (index_tri >= 0).any()             # masked pixels that miss, and that hit
        index_tri = np.unique(index_tri[index_tri >= 0])
        naive[index_tri] += 1
        cam = (np.concatenate([centres[index_tri], np.ones((len(index_tri), 1))], 1) @ np.linalg.inv(c2w.astype(np.float64)).T)[:, :3]
        uv = ((cam / cam[:, 2:3]) @ K.astype(np.float64).T)[:, :2]
        assert np.abs(uv - np.floor(uv) - 0.5).min() > 1e-3                 # no centre within fp32 rounding of a pixel's edge
        uv = np.round(uv).astype(np.int64)
        ok = (uv[:, 0] >= 0) & (uv[:, 0] < w) & (uv[:, 1] >= 0) & (uv[:, 1] < h)
        ok[ok] = mask[uv[ok, 1], uv[ok, 0]]
        counter[index_tri[ok]] += 1
    return counter, naive


def test_triangle_votes_against_a_numpy_restatement():
    """Three 24 x 32 views of a 1280-face sphere from outside: the corners of every view miss it."""
    verts, faces = rays.icosphere(3)
    h, w = 24, 32
    K = np.array([[32, 0, 16], [0, 32, 12], [0, 0, 1]], F32)
    pose = lambda cols, at: np.concatenate((np.concatenate((np.array(cols, F32).T, np.array(at, F32)[:, None]), 1), [[0, 0, 0, 1]])).astype(F32)
    c2ws = [pose(((1, 0, 0), (0, 1, 0), (0, 0, 1)), (0, 0, -3)),           # looking along +z
            pose(((0, 0, -1), (0, 1, 0), (1, 0, 0)), (-3, 0, 0)),          # along +x
            pose(((1, 0, 0), (0, 0, 1), (0, -1, 0)), (0, 3, 0))]           # along -y
    g = np.random.default_rng(5)
    yy, xx = np.mgrid[:h, :w]
    masks = [np.ones((h, w), bool), (xx + yy) % 3 != 0, g.uniform(size=(h, w)) < 0.6]
    masks[1][:4], masks[2][:, :5] = True, True                               # (corner pixels, which miss, stay in)
    want, want_naive = _votes_host(verts, faces, masks, c2ws, K, h, w)
    assert want_naive.max() >= 2 and 0 < want.sum() <= want_naive.sum() and (want <= want_naive).all() and (want != want_naive).any()
    scene = meshquery.Scene(verts, faces, device=DEV)
    counter, naive = extract.triangle_votes(scene, [torch.tensor(m, device=DEV) for m in masks], [torch.tensor(c) for c in c2ws], K, h, w)
    assert counter.dtype == torch.int32 and naive.dtype == torch.int32 and counter.is_cuda and naive.is_cuda
    assert np.array_equal(naive.cpu().numpy(), want_naive)
    assert np.array_equal(counter.cpu().numpy(), want)
    # masks as 0 / 255 images, poses and K as numpy: the same votes
    again = extract.triangle_votes(scene, [(m * 255).astype(np.uint8) for m in masks], c2ws, K, h, w)
    assert torch.equal(again[0], counter) and torch.equal(again[1], naive)


# ---- the branches of the contract, family by family (meshrays_cases; tests/test_meshrays.py holds the restatement to the same rays) ---
def _check_case(case, what, pruned=False):
    """``check`` on a family: the kernel against the restatement in every bit, three ways; returns the restatement's answers."""
    with np.errstate(all="ignore"):
        return check(case.o, case.d, case.verts, case.faces, what, pruned=pruned)[:3]


def _kernel(case):
    return tuple(x.cpu().numpy() for x in meshquery.first_hits(*_on_gpu(case.o, case.d, case.verts, case.faces), return_bary=True))


@pytest.mark.parametrize("mesh", ["cube", "icosphere"])
def test_every_shear_and_the_ties_between_them(mesh):
    """kz at exact ties of |d| (to the lowest axis), the kx / ky swap on each axis, -0.0 components, Sz != +-1."""
    case = rays.shears(mesh)
    rays.expect_shears(case, *_check_case(case, f"shears, {mesh}"))


def test_axis_parallel_rays_and_flat_boxes():
    """d_k == 0 (and -0.0) on two axes with lo_k == o_k == hi_k on flat boxes: the exact t, the near side."""
    case = rays.axis_parallel()
    rays.expect_axis_parallel(case, *_check_case(case, "axis-parallel"))
    rays.expect_axis_parallel(case, *_kernel(case))


@pytest.mark.parametrize("distance", [3.0, 1e2, 1e4])
def test_the_clamp_at_work_on_flat_boxes(distance):
    """Oblique rays onto the cube: one hit in six has t != t_tri (asserted by the family: one in twenty at least), so the bits of t
    are those of the clamp."""
    case = rays.oblique_onto_cube(distance)
    rays.expect_oblique_onto_cube(case, *_check_case(case, f"oblique from {distance}"))


def test_origins_on_the_surface_and_faces_without_area():
    """t == +0.0 (never -0.0) from an origin on a face, det == 0 in a face's plane and on faces of zero area."""
    case = rays.surface_origins()
    rays.expect_surface_origins(case, *_check_case(case, "origins on the surface"))
    face, t, _ = _kernel(case)
    assert not np.signbit(t).any() and (t[case.normal] == 0).all() and not np.isin(face, case.degenerate).any()


def test_denormal_components_and_overflow():
    """Denormal components of d are kept (1 / d_k finite or +-inf by the value, 0 * inf dropped by fmax / fmin); overflowing
    determinants are a miss."""
    case = rays.denormal_rays()
    rays.expect_denormal_rays(case, *_check_case(case, "denormal components"))
    rays.expect_all_miss(case.huge, *_check_case(case.huge, "coordinates of 1e38"))


@pytest.mark.parametrize("F", [1025, 16385])
def test_comb_rays_that_prune_nothing_and_exact_hits(F):
    """Whole waves that enter every leaf and hit nothing, waves that hit the first, the last and a middle plane, and all of them
    mixed: the exact t and the plane."""
    case = rays.comb(F)
    rays.expect_comb(case, *_check_case(case, f"a comb of {F}"))
    rays.expect_comb(case, *_kernel(case))


def test_ties_between_leaves():
    """An equal t with a lower face index in a leaf that is popped later: 301 copies of one face over five leaves, and diagonal rays
    through the vertices of the integer plane, where up to six faces of several leaves tie."""
    case = rays.copies()
    rays.expect_copies(case, *_check_case(case, "301 copies of one face"))
    assert (_kernel(case)[0] == case.same.min()).all()
    case = rays.plane_vertex_rays(30, 20, 6)                          # the plane of test_exact_ties_on_the_gpu
    rays.expect_plane_vertex_rays(case, *_check_case(case, "diagonal rays through the vertices of a plane"))
    rays.expect_plane_vertex_rays(case, *_kernel(case))


def test_four_levels():
    """F = 262145: 4097 leaves under 257, 17 and 2 boxes, the level of a stack entry one higher than any other ray test has it."""
    case = rays.four_levels()
    rays.expect_four_levels(case, *_check_case(case, "four levels", pruned=True))
