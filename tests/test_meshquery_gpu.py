"""The closest-triangle kernels (gsr_meshquery.hip) against the numpy restatement of their contract (meshquery.closest_triangles_host),
bit for bit: the face index, the bits of the squared distance and the bits of the closest point -- at every face count where the tree
changes shape, at the wave's edges in the query count, and on the meshes where an inexact search or a loose tie rule would show."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from autovfx_amd import meshquery
from autovfx_amd.meshquery import closest_triangles_host

import meshquery_cases as cases

pytestmark = pytest.mark.gpu
F32 = np.float32
DEV = "cuda:0"


def _special_queries(verts, faces, seed=0):
    """On the surface (corners, and fp32 points inside faces), far outside the bounds, non-finite."""
    g = np.random.default_rng(seed)
    out = []
    if faces.shape[0] and verts.shape[0]:
        ok = meshquery.valid_faces_host(verts, faces)
        f = faces[ok][g.integers(0, max(1, ok.sum()), 12)] if ok.any() else faces[:0]
        if f.shape[0]:
            out.append(verts[f[:, 0]])
            out.append(((verts[f[:, 0]] + verts[f[:, 1]]) * F32(0.5)).astype(F32))
            out.append(((verts[f[:, 0]] + verts[f[:, 1]] + verts[f[:, 2]]) / F32(3)).astype(F32))
    out.append(np.array([[1e3, -2e3, 5e2], [-7e5, 1.0, 3.0], [0.0, 0.0, 1e6]], F32))
    out.append(np.array([[np.nan, 0, 0], [0, np.inf, 0], [1, 2, -np.inf]], F32))
    return np.concatenate(out).astype(F32)


def _queries(verts, faces, n, reach, seed=1):
    ok = meshquery.valid_faces_host(verts, faces) if faces.shape[0] else np.zeros(0, bool)
    if ok.any():
        near = cases.queries_near(verts, faces[ok], n, reach, seed)
    else:
        near = np.random.default_rng(seed).normal(size=(n, 3)).astype(F32)
    return np.concatenate((near, _special_queries(verts, faces, seed)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same_bits(got, want, what=""):
    idx, d, closest = (t.cpu().numpy() for t in got)
    assert idx.dtype == np.int64 and d.dtype == F32 and closest.dtype == F32
    bad = np.nonzero(idx != want[0])[0]
    assert bad.size == 0, (what, "face_idx", bad[:5], idx[bad[:5]], want[0][bad[:5]], d[bad[:5]], want[1][bad[:5]])
    bad = np.nonzero(_bits(d) != _bits(want[1]))[0]
    assert bad.size == 0, (what, "sq_dist", bad[:5], d[bad[:5]], want[1][bad[:5]])
    bad = np.nonzero((_bits(closest) != _bits(want[2])).any(axis=1))[0]
    assert bad.size == 0, (what, "closest", bad[:5], closest[bad[:5]], want[2][bad[:5]])


def _on_gpu(q, verts, faces):
    return (torch.tensor(q, device=DEV), torch.tensor(verts, device=DEV), torch.tensor(faces, device=DEV))


def check(q, verts, faces, what=""):
    want = closest_triangles_host(q, verts, faces)
    tq, tv, tf = _on_gpu(q, verts, faces)
    got = meshquery.closest_triangles(tq, tv, tf, return_points=True)
    assert_same_bits(got, want, what)
    # (above: asked in Morton order and put back; here: in the caller's order -- an answer is a function of its own query alone)
    assert_same_bits(meshquery._query(tq, meshquery.plan(tv, tf), True, sort_queries=False), want, what + ", caller's order")
    short = meshquery.closest_triangles(tq, tv, tf)                 # closest = NULL: the same ids and distances
    assert len(short) == 2 and torch.equal(short[0], got[0]) and torch.equal(short[1].view(torch.int32), got[1].view(torch.int32))
    return want


# ---- the tree's shape changes, the wave's edges ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 2, 63, 64, 65, 1024, 1025, 16385])
def test_every_tree_shape(F):
    verts, faces = cases.sphere_with_faces(F, seed=F)
    q = _queries(verts, faces, 280, 0.4, seed=F)
    want = check(q, verts, faces, f"F = {F}")
    assert (want[0] >= 0).sum() == len(q) - 3 and (want[1] == 0).sum() >= 10      # only the non-finite miss; the surface points hit


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_every_wave_edge(n):
    verts, faces = cases.sphere_with_faces(1025, seed=7)
    q = _queries(verts, faces, 1000, 0.3, seed=11)
    q = np.concatenate((q[-3:], q[:-3]))[:n] if n > 1 else q[:1]     # (the non-finite ones first, where n allows them)
    check(q, verts, faces, f"n = {n}")


# ---- the meshes ---------------------------------------------------------------------------------------------------------------------
def _plane_with_ties():
    verts, faces = cases.grid_plane(30, 20, 1.0)                     # 1200 faces, integer coordinates: every tie is exact
    even = faces[::2]
    above = verts + np.asarray((0, 0, 0.75), F32)
    mids = ((verts[even[:, 0]] + verts[even[:, 2]]) * F32(0.5) + np.asarray((0, 0, 2.0), F32)).astype(F32)
    sides = ((verts[even[:, 0]] + verts[even[:, 1]]) * F32(0.5) + np.asarray((0, 0, -1.5), F32)).astype(F32)
    on = np.concatenate((verts, mids - np.asarray((0, 0, 2.0), F32)))
    return verts, faces, np.concatenate((above, mids, sides, on)).astype(F32)


def test_exact_ties_above_vertices_and_edges():
    verts, faces, q = _plane_with_ties()
    want = check(np.concatenate((q, _special_queries(verts, faces))), verts, faces, "plane")
    V = verts.shape[0]
    lowest = np.array([np.nonzero((faces == v).any(axis=1))[0].min() for v in range(V)])
    assert np.array_equal(want[0][:V], lowest) and np.all(want[1][:V] == F32(0.5625))
    # the same plane with its faces in a random order: other indices tie, the lowest still wins
    order = np.random.default_rng(5).permutation(faces.shape[0])
    want = check(q, verts, faces[order], "plane, random face order")
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size)
    assert np.array_equal(want[0][:V], np.array([rank[np.nonzero((faces == v).any(axis=1))[0]].min() for v in range(V)]))


def test_every_face_duplicated():
    verts, faces = cases.sphere_with_faces(700, seed=2)
    q = _queries(verts, faces, 500, 0.4, seed=3)
    once = closest_triangles_host(q, verts, faces)
    want = check(q, verts, np.concatenate((faces, faces)), "duplicated")
    assert np.array_equal(want[0], once[0]) and want[0].max() < 700
    order = np.random.default_rng(8).permutation(1400)
    check(q, verts, np.concatenate((faces, faces))[order], "duplicated, shuffled")


def test_degenerate_faces_mixed_in():
    verts, faces = cases.sphere_with_faces(1100, seed=4)
    g = np.random.default_rng(6)
    a = g.uniform(-1.2, 1.2, (60, 3))
    step = g.normal(size=(60, 3)) * 0.2
    extra = np.concatenate((np.stack((a[:30], a[:30] + step[:30], a[:30] + 2 * step[:30]), 1).reshape(-1, 3),      # collinear
                            np.repeat(a[30:], 3, axis=0))).astype(F32)                                               # three equal vertices
    more = (np.arange(extra.shape[0]).reshape(-1, 3) + verts.shape[0]).astype(np.int64)
    verts2 = np.concatenate((verts, extra))
    faces2 = np.concatenate((faces, more, faces[:40, [0, 0, 1]], faces[40:80, [2, 2, 2]]))[g.permutation(1100 + 60 + 80)]
    q = np.concatenate((_queries(verts2, faces2, 500, 0.4, seed=5), extra[::3], (extra[::3] + F32(0.01)).astype(F32)))
    want = check(q, verts2, faces2, "degenerate")
    assert np.all(np.isfinite(want[1][want[0] >= 0]))


def test_one_vertex_far_away_stretches_the_bounds():
    verts, faces = cases.sphere_with_faces(1300, seed=9)
    verts = verts.copy()
    verts[faces[17, 1]] = (1e4, -1e4, 1e4)
    q = np.concatenate((_queries(verts, faces, 500, 0.4, seed=10), np.array([[5e3, -5e3, 5e3], [1e4, -1e4, 1e4], [9e3, 0, 0]], F32)))
    check(q, verts, faces, "far vertex")


def test_invalid_faces_are_never_answered():
    verts, faces = cases.sphere_with_faces(3000, seed=12)
    verts, faces = verts.copy(), faces.copy()
    g = np.random.default_rng(13)
    bad = g.permutation(3000)[:30]
    faces[bad[:8], g.integers(0, 3, 8)] = verts.shape[0]
    faces[bad[8:14], g.integers(0, 3, 6)] = -1
    faces[bad[14:18], 0] = 1 << 40
    extra = np.full((12, 3), 0.5, F32)
    extra[np.arange(12), g.integers(0, 3, 12)] = [np.nan, np.inf, -np.inf] * 4
    faces[bad[18:], g.integers(0, 3, 12)] = verts.shape[0] + np.arange(12)
    verts = np.concatenate((verts, extra))
    assert (~meshquery.valid_faces_host(verts, faces)).sum() == 30
    q = _queries(verts, faces, 600, 0.4, seed=14)
    want = check(q, verts, faces, "1 % invalid")
    assert not np.isin(want[0], bad).any()
    # all of them invalid, and no faces at all: every query gets (-1, +inf, 0 0 0)
    for f in (faces[np.sort(bad)], faces[:0]):
        want = check(q, verts, f, f"{f.shape[0]} faces, none valid")
        assert np.all(want[0] == -1) and np.all(np.isposinf(want[1])) and np.all(want[2] == 0)
    check(q, verts[:0], faces[:5], "no vertices")
    got = meshquery.closest_triangles(torch.zeros((0, 3), device=DEV), *_on_gpu(q, verts, faces)[1:], return_points=True)
    assert [tuple(t.shape) for t in got] == [(0,), (0,), (0, 3)]


# ---- the call ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere_case():
    verts, faces = cases.sphere_with_faces(2100, seed=20)
    q = _queries(verts, faces, 900, 0.4, seed=21)
    return q, verts, faces, closest_triangles_host(q, verts, faces)


@pytest.mark.parametrize("fill", [0xFF, 0x55])
def test_every_output_element_is_written(sphere_case, fill):
    from autovfx_amd import _lib
    q, verts, faces, want = sphere_case
    tq, tv, tf = _on_gpu(q, verts, faces)
    plan = meshquery.plan(tv, tf)
    n = len(q)
    raw = [torch.full((8 * n,), fill, dtype=torch.uint8, device=DEV), torch.full((4 * n,), fill, dtype=torch.uint8, device=DEV),
           torch.full((12 * n,), fill, dtype=torch.uint8, device=DEV)]
    _lib.call("gsr_closest_tri_query", n, tq.data_ptr(), plan.buffer.data_ptr(), plan.buffer.numel(), raw[0].data_ptr(), raw[1].data_ptr(),
              raw[2].data_ptr(), device=tq.device)
    got = (raw[0].view(torch.int64), raw[1].view(torch.float32), raw[2].view(torch.float32).reshape(n, 3))
    assert_same_bits(got, want, f"fill {fill:#x}")


def test_a_plan_serves_many_batches_and_streams(sphere_case):
    q, verts, faces, want = sphere_case
    tq, tv, tf = _on_gpu(q, verts, faces)
    plan = meshquery.plan(tv, tf)
    assert plan.F == 2100 and plan.V == verts.shape[0] and plan.buffer.dtype == torch.uint8 and plan.buffer.is_cuda
    half = len(q) // 2
    first = meshquery.closest_triangles(tq[:half], tv, tf, plan=plan, return_points=True)
    second = meshquery.closest_triangles(tq[half:], tv, tf, plan=plan, return_points=True)
    assert_same_bits(tuple(torch.cat(p) for p in zip(first, second)), want, "two batches")
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        again = meshquery.closest_triangles(tq, tv, tf, plan=plan, return_points=True)
    side.synchronize()
    assert_same_bits(again, want, "side stream")
    with pytest.raises(ValueError, match="not of this one"):
        meshquery.closest_triangles(tq, tv, tf[:-1], plan=plan)


def test_non_contiguous_inputs_are_copied(sphere_case):
    q, verts, faces, want = sphere_case
    wide_q = torch.zeros((2 * len(q), 4), device=DEV)
    wide_q[::2, :3] = torch.tensor(q, device=DEV)
    wide_v = torch.full((verts.shape[0], 5), 7.0, device=DEV)
    wide_v[:, 1:4] = torch.tensor(verts, device=DEV)
    wide_f = torch.full((3, faces.shape[0]), -1, dtype=torch.int64, device=DEV)
    wide_f[:] = torch.tensor(faces, device=DEV).t()
    tq, tv, tf = wide_q[::2, :3], wide_v[:, 1:4], wide_f.t()
    assert not (tq.is_contiguous() or tv.is_contiguous() or tf.is_contiguous())
    assert_same_bits(meshquery.closest_triangles(tq, tv, tf, return_points=True), want, "strided")


def test_scene_adapter_from_numpy(sphere_case):
    q, verts, faces, want = sphere_case
    scene = meshquery.Scene(verts.astype(np.float64), faces.astype(np.int32), device=DEV)
    for points in (q, q.astype(np.float64), torch.tensor(q)):
        ans = scene.compute_closest_points(points)
        assert set(ans) >= {"primitive_ids", "points", "distances"} and all(t.is_cuda for t in ans.values())
        assert_same_bits((ans["primitive_ids"], ans["squared_distances"], ans["points"]), want, "Scene")
        assert torch.equal(ans["distances"].view(torch.int32), torch.sqrt(ans["squared_distances"]).view(torch.int32))


def test_a_header_that_does_not_match_answers_nothing(sphere_case):
    """The query kernel compares the plan's header with the size it is handed before anything indexes the plan: a cleared header, a
    header of another mesh and a truncated plan all answer (-1, +inf, 0 0 0) and read nothing past the header.  (The Python entry
    point refuses a buffer of the wrong size before that, from the plan's own F.)"""
    from autovfx_amd import _lib
    q, verts, faces, _ = sphere_case
    tq, tv, tf = _on_gpu(q[:200], verts, faces)
    plan = meshquery.plan(tv, tf)
    cleared = plan.buffer.clone()
    cleared[:256] = 0
    other = plan.buffer.clone()
    other[:256] = meshquery.plan(tv, tf[:100]).buffer[:256]
    cut = plan.buffer[:plan.buffer.numel() // 512 * 256]
    for name, buffer in (("cleared", cleared), ("of another mesh", other)):
        idx, d, closest = meshquery.closest_triangles(tq, tv, tf, plan=meshquery.Plan(buffer, plan.F, plan.V), return_points=True)
        assert bool((idx == -1).all()) and bool(torch.isposinf(d).all()) and bool((closest == 0).all()), name
    with pytest.raises(ValueError, match="a plan of 2100 faces is"):
        meshquery.closest_triangles(tq, tv, tf, plan=meshquery.Plan(cut, plan.F, plan.V))
    n = tq.shape[0]
    idx = torch.full((n,), 7, dtype=torch.int64, device=DEV)
    d, closest = torch.zeros(n, device=DEV), torch.ones((n, 3), device=DEV)
    _lib.call("gsr_closest_tri_query", n, tq.data_ptr(), cut.data_ptr(), cut.numel(), idx.data_ptr(), d.data_ptr(), closest.data_ptr(),
              device=tq.device)
    assert bool((idx == -1).all()) and bool(torch.isposinf(d).all()) and bool((closest == 0).all())
