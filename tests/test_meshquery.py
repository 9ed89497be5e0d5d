"""The closest-triangle query without a GPU (autovfx_amd/meshquery.py, gsr_meshquery.hip): the numpy restatement of the contract
against an independent float64 brute force, its clamps and its tie rule, what the C ABI refuses before it launches anything, and how
the frame loop reads its option."""
from __future__ import annotations

import os
import types

import numpy as np
import pytest
import torch

from autovfx_amd import frame_loop, meshquery
from autovfx_amd.meshquery import closest_triangles_host, triangle_distance_host

import meshquery_cases as cases
from helpers import fake_gpu as _gpu

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))


# ---- the restatement against the truth ----------------------------------------------------------------------------------------------
# Translated coordinates carry u = 2^-24 relative error; the closest point then has an error of roughly 40 u L^2 / e with L <= 5 e
# (queries within 4 e of a surface of edge length e): about 6e-5 e.  The bound is 16 times that estimate.
TRUTH_TOL = 1e-3


def _truth_meshes():
    out = {"plane e=1": cases.grid_plane(9, 7, 1.0),
           "plane e=0.01 off origin": cases.grid_plane(8, 8, 0.01, origin=(3.0, -2.0, 5.0)),
           "sphere": cases.cube_sphere(6, 1.0, (0.3, -0.2, 0.5)),
           "small sphere off origin": cases.cube_sphere(5, 0.05, (-4.0, 2.5, 1.0))}
    return out


@pytest.mark.parametrize("name", list(_truth_meshes()))
def test_restatement_against_float64_truth(name):
    verts, faces = _truth_meshes()[name]
    e = float(cases.edge_lengths(verts, faces).min())          # the shortest edge: the strictest reading of "edge length e"
    q = cases.queries_near(verts, faces, 600, 4.0 * e, seed=5)
    idx, d, closest = closest_triangles_host(q, verts, faces)
    truth = cases.truth_distances(q, verts, faces)
    d_true = truth.min(axis=1)
    err_d = np.abs(np.sqrt(d.astype(np.float64)) - d_true)
    err_f = np.abs(truth[np.arange(len(q)), idx] - d_true)
    print(f"{name}: e = {e:.4g}, worst |sqrt(d) - truth| = {err_d.max() / e:.3g} e, worst named-face excess = {err_f.max() / e:.3g} e")
    assert np.all(idx >= 0) and np.all(idx < faces.shape[0])
    assert np.all(err_d <= TRUTH_TOL * e)
    assert np.all(err_f <= TRUTH_TOL * e)
    # ... and the point it returns lies at that distance
    gap = np.linalg.norm(closest.astype(np.float64) - q.astype(np.float64), axis=1)
    assert np.all(np.abs(gap - d_true) <= TRUTH_TOL * e + 4 * 2.0 ** -24 * np.abs(q).max())


def test_restatement_is_chunk_independent():
    verts, faces = cases.cube_sphere(4)
    q = cases.queries_near(verts, faces, 200, 0.5, seed=2)
    ref = closest_triangles_host(q, verts, faces)
    for chunk in (1, 97, 1 << 24):
        got = closest_triangles_host(q, verts, faces, chunk_elems=chunk)
        assert all(np.array_equal(a, b) for a, b in zip(got, ref))


# ---- the clamps ---------------------------------------------------------------------------------------------------------------------
def _hard_triangles():
    g = np.random.default_rng(3)
    n = 300
    a = g.uniform(-1, 1, (n, 3))
    along = g.normal(size=(n, 3))
    slivers = np.stack((a, a + along, a + 0.5 * along + 1e-7 * g.normal(size=(n, 3))), 1)                 # nearly collinear
    collinear = np.stack((a, a + along, a + 2 * along), 1)
    dots = np.stack((a, a + 1e-7 * g.normal(size=(n, 3)), a + 1e-7 * g.normal(size=(n, 3))), 1)          # point-like
    same = np.stack((a, a, a), 1)
    far = np.stack((a, a + g.normal(size=(n, 3)), a + g.normal(size=(n, 3))), 1) + (1e4 * along / np.linalg.norm(along, axis=1, keepdims=True))[:, None, :]
    return {"slivers": slivers, "collinear": collinear, "point-like": dots, "three equal vertices": same, "1e4 away": far}


@pytest.mark.parametrize("kind", list(_hard_triangles()))
def test_the_distance_stays_between_its_box_and_its_nearest_corner(kind):
    tri = _hard_triangles()[kind].astype(F32)
    q = np.random.default_rng(4).uniform(-1, 1, (tri.shape[0], 3)).astype(F32)
    got = triangle_distance_host(q, tri[:, 0], tri[:, 1], tri[:, 2])
    assert np.all(np.isfinite(got["d"])) and np.all(got["d"] >= 0)
    assert np.all(got["d_box"] <= got["d"]) and np.all(got["d"] <= got["d_vtx"])
    # the interval really brackets the truth (to the rounding of its own few operations)
    verts = tri.reshape(-1, 3)
    faces = np.arange(verts.shape[0], dtype=np.int64).reshape(-1, 3)
    truth = cases.truth_distances(q, verts, faces)[np.arange(len(q)), np.arange(len(q))] ** 2
    slack = 8 * 2.0 ** -24
    assert np.all(got["d_box"].astype(np.float64) <= truth * (1 + slack) + 1e-30)
    assert np.all(got["d_vtx"].astype(np.float64) >= truth * (1 - slack))
    if kind == "1e4 away":    # where d_tri alone is badly conditioned the answer is still within the clamps' reach of the truth
        assert np.all(np.abs(np.sqrt(got["d"].astype(np.float64)) - np.sqrt(truth)) <= 1e-5 * np.sqrt(truth))


# ---- ties ---------------------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_lower_face_index():
    verts, faces = cases.grid_plane(6, 5, 1.0)
    # above every vertex, exactly: every face around it is at the same distance, bit for bit
    q = verts + np.asarray((0.0, 0.0, 0.75), F32)
    idx, d, closest = closest_triangles_host(q, verts, faces)
    want = np.array([np.nonzero((faces == v).any(axis=1))[0].min() for v in range(verts.shape[0])])
    assert np.array_equal(idx, want)
    assert np.all(d == F32(0.5625)) and np.array_equal(closest, verts)
    # above edge midpoints: the two faces of an inner edge tie
    even = faces[::2]                                         # (i, j), (i + 1, j), (i + 1, j + 1): corners 0 and 2 span the cell's diagonal
    mid = ((verts[even[:, 0]] + verts[even[:, 2]]) * F32(0.5) + np.asarray((0.0, 0.0, 2.0), F32)).astype(F32)
    idx, d, _ = closest_triangles_host(mid, verts, faces)
    assert np.array_equal(idx, np.arange(0, faces.shape[0], 2)) and np.all(d == F32(4.0))
    # a duplicated face never answers
    both = np.concatenate((faces, faces))
    q = cases.queries_near(verts, faces, 300, 1.5, seed=9)
    idx2, d2, _ = closest_triangles_host(q, verts, both)
    idx1, d1, _ = closest_triangles_host(q, verts, faces)
    assert np.array_equal(idx2, idx1) and np.array_equal(d2, d1) and idx2.max() < faces.shape[0]
    # ... also in the other order of the copies
    order = np.random.default_rng(1).permutation(both.shape[0])
    idx3, d3, _ = closest_triangles_host(q, verts, both[order])
    assert np.array_equal(d3, d1)
    assert np.array_equal(order[idx3] % faces.shape[0], idx1)
    twin = np.array([np.nonzero(order % faces.shape[0] == f)[0].min() for f in idx1])
    assert np.array_equal(idx3, twin)


def test_invalid_faces_and_non_finite_queries():
    verts, faces = cases.grid_plane(4, 4, 1.0)
    verts = verts.copy()
    faces = faces.copy()
    verts[7, 1] = np.nan
    faces[3, 2] = verts.shape[0]
    faces[5, 0] = -1
    bad = np.zeros(faces.shape[0], bool)
    bad[[3, 5]] = True
    bad |= (faces == 7).any(axis=1) & ~bad
    assert np.array_equal(meshquery.valid_faces_host(verts, faces), ~bad)
    q = cases.queries_near(verts[:5], np.array([[0, 1, 2]]), 100, 3.0, seed=3)
    q[10, 0], q[20, 2] = np.inf, np.nan
    idx, d, closest = closest_triangles_host(q, verts, faces)
    ok = np.ones(100, bool)
    ok[[10, 20]] = False
    assert np.all(idx[~ok] == -1) and np.all(np.isposinf(d[~ok])) and np.all(closest[~ok] == 0)
    assert not np.isin(idx[ok], np.nonzero(bad)[0]).any() and np.all(idx[ok] >= 0) and np.all(np.isfinite(d[ok]))
    for none in (faces[bad], faces[:0]):
        idx, d, closest = closest_triangles_host(q, verts, none)
        assert np.all(idx == -1) and np.all(np.isposinf(d)) and np.all(closest == 0)


# ---- the C ABI: sizes and refusals need no device -----------------------------------------------------------------------------------
def test_cabi_sizes_and_refusals_need_no_device():
    from autovfx_amd import _lib
    L = _lib.lib
    assert L.gsr_abi_version() == 20 == _lib.ABI_VERSION
    sizes = [L.gsr_closest_tri_plan_bytes(F) for F in (0, 1, 63, 64, 65, 1024, 1025, 16385, 10 ** 6, (1 << 30) - 1)]
    assert sizes[0] == 256 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[1] > sizes[0]
    assert all(s % 256 == 0 for s in sizes)
    assert 48 * 10 ** 6 < sizes[8] < 52 * 10 ** 6
    scratch = [L.gsr_closest_tri_plan_scratch_bytes(F) for F in (0, 1, 65, 1025, 10 ** 6)]
    assert scratch[0] == 0 and all(a <= b for a, b in zip(scratch, scratch[1:])) and scratch[1] > 0
    for bad in (-1, 1 << 30, 1 << 40):
        assert L.gsr_closest_tri_plan_bytes(bad) == 0 and L.gsr_closest_tri_plan_scratch_bytes(bad) == 0

    V, F = 500, 1000
    verts, faces, plan, work = 4096, 8192, 1 << 20, 1 << 24            # addresses that are never read: every call is refused
    pb, sb = L.gsr_closest_tri_plan_bytes(F), L.gsr_closest_tri_plan_scratch_bytes(F)

    def plan_refused(*args, word):
        return L.gsr_closest_tri_plan(*args, None) != 0 and word in _lib.last_error()

    assert plan_refused(-1, verts, F, faces, plan, pb, work, sb, word="negative")
    assert plan_refused(V, verts, -1, faces, plan, pb, work, sb, word="negative")
    assert plan_refused(V, verts, 1 << 30, faces, plan, 1 << 40, work, 1 << 40, word="2^30")
    assert plan_refused(1 << 31, verts, F, faces, plan, pb, work, sb, word="2^31")
    for hole in range(4):
        ptrs = [verts, faces, plan, work]
        ptrs[hole] = None
        assert plan_refused(V, ptrs[0], F, ptrs[1], ptrs[2], pb, ptrs[3], sb, word="null"), hole
    assert plan_refused(V, verts, 0, None, None, 256, None, 0, word="null")           # an empty mesh still needs its plan
    assert plan_refused(V, verts + 2, F, faces, plan, pb, work, sb, word="aligned")
    assert plan_refused(V, verts, F, faces + 4, plan, pb, work, sb, word="aligned")
    assert plan_refused(V, verts, F, faces, plan + 128, pb, work, sb, word="aligned")
    assert plan_refused(V, verts, F, faces, plan, pb, work + 64, sb, word="aligned")
    assert plan_refused(V, verts, F, faces, plan, pb - 1, work, sb, word="plan too small")
    assert plan_refused(V, verts, F, faces, plan, pb, work, sb - 1, word="scratch too small")
    assert plan_refused(V, verts, 0, None, plan, 255, None, 0, word="plan too small")

    n, points, ids, dist, near = 300, 4096, 8192, 1 << 16, 1 << 17

    def query_refused(*args, word):
        return L.gsr_closest_tri_query(*args, None) != 0 and word in _lib.last_error()

    assert L.gsr_closest_tri_query(0, None, None, 0, None, None, None, None) == 0     # n == 0: nothing to do, nothing looked at
    assert query_refused(-1, points, plan, pb, ids, dist, near, word="negative")
    assert query_refused(1 << 31, points, plan, pb, ids, dist, near, word="2^31")
    for hole in range(4):
        ptrs = [points, plan, ids, dist]
        ptrs[hole] = None
        assert query_refused(n, ptrs[0], ptrs[1], pb, ptrs[2], ptrs[3], near, word="null"), hole
    assert query_refused(n, points + 2, plan, pb, ids, dist, near, word="aligned")
    assert query_refused(n, points, plan + 16, pb, ids, dist, near, word="aligned")
    assert query_refused(n, points, plan, pb, ids + 4, dist, near, word="aligned")
    assert query_refused(n, points, plan, pb, ids, dist + 1, near, word="aligned")
    assert query_refused(n, points, plan, pb, ids, dist, near + 2, word="aligned")
    assert query_refused(n, points, plan, 0, ids, dist, near, word="not the size of a plan")
    assert query_refused(n, points, plan, 128, ids, dist, near, word="not the size of a plan")
    assert query_refused(n, points, plan, pb + 1, ids, dist, near, word="not the size of a plan")


# ---- the plan's layout and its restatement ------------------------------------------------------------------------------------------
def test_plan_layout_is_the_librarys_arithmetic():
    from autovfx_amd import _lib
    sizes = sorted({64 * 16 ** k + step for k in range(6) for step in (-1, 0, 1)} | {0, 1, (1 << 30) - 1})
    for F in sizes:
        L = meshquery.plan_layout(F)
        assert L.bytes == _lib.lib.gsr_closest_tri_plan_bytes(F) and L.bytes % 256 == 0, F
        assert L.records == 256 and L.boxes % 256 == 0 and L.boxes >= 256 + 48 * F and L.bytes >= L.boxes + 32 * sum(L.counts), F
        assert L.leaves == L.counts[0] == -(-F // 64) and L.top == len(L.counts) - 1 <= 5 and L.counts[-1] <= 16, F
        assert L.offsets == tuple(sum(L.counts[:k]) for k in range(len(L.counts))), F
    # by hand: leaves of 64, levels of 16 up to the first of at most 16 boxes
    by_hand = {16384: (256, 16), 16385: (257, 17, 2), 262144: (4096, 256, 16), 262145: (4097, 257, 17, 2)}
    for F, counts in by_hand.items():
        L = meshquery.plan_layout(F)
        assert L.counts == counts and L.top == len(counts) - 1, F
    assert meshquery.plan_layout(262145).offsets == (0, 4097, 4354, 4371)
    assert meshquery.plan_layout((1 << 30) - 1).counts == (1 << 24, 1 << 20, 1 << 16, 4096, 256, 16)
    for bad in (-1, 1 << 30):
        with pytest.raises(ValueError, match="faces"):
            meshquery.plan_layout(bad)


def _small_plan_meshes():
    """The meshes of tests/test_meshquery_deep_gpu.py at sizes a CPU test can walk leaf by leaf."""
    out = {f"sphere F={F}": cases.sphere_with_faces(F, seed=F) for F in (1, 64, 65, 1025, 3000)}
    out["flat plane"] = cases.grid_plane(30, 20, 1.0)
    verts, faces = cases.sphere_with_faces(300, seed=2)
    out["duplicated x 8"] = (verts, np.concatenate([faces] * 8))
    verts, faces = cases.sphere_with_faces(1300, seed=9)
    verts = verts.copy()
    verts[faces[17, 1]] = (1e4, -1e4, 1e4)
    out["far vertex"] = (verts, faces)
    out["overflowing centroid"] = cases.sphere_with_overflowing_centroid(700, seed=3)
    out["empty boxes"] = cases.sphere_with_invalid(1088, 1152, seed=4)[:2]           # 35 leaves, 18 of them empty; 3 boxes, 1 empty
    out["shared tail leaf"] = cases.sphere_with_invalid(1000, 1240, seed=4)[:2]
    out["none valid"] = (verts, np.full((130, 3), -1, np.int64))
    out["spanners and slivers"] = cases.sphere_with_spanners(2000, 20, 60, seed=5)
    return out


@pytest.mark.parametrize("name", list(_small_plan_meshes()))
def test_plan_host_invariants(name):
    verts, faces = _small_plan_meshes()[name]
    F = faces.shape[0]
    L = meshquery.plan_layout(F)
    order, records, levels = meshquery.plan_host(verts, faces)
    valid = meshquery.valid_faces_host(verts, faces)
    n_valid = int(valid.sum())
    # a permutation, the valid faces first, the invalid ones last in ascending index
    assert order.shape == (F,) and np.array_equal(np.sort(order), np.arange(F))
    assert valid[order[:n_valid]].all() and np.array_equal(order[n_valid:], np.nonzero(~valid)[0])
    # the codes along it do not decrease, and equal codes come in ascending face index (the sort is stable)
    codes = meshquery.morton_codes_host(verts, faces)
    assert np.all(codes[valid] < np.uint64(1 << 63)) and np.all(codes[~valid] == np.uint64(1 << 63))
    along = codes[order]
    assert np.all(along[1:] >= along[:-1])
    same = along[1:] == along[:-1]
    assert np.all(order[1:][same] > order[:-1][same])
    # the records
    words = records.view(np.uint32)
    assert records.shape == (F, 3, 4) and records.dtype == F32
    assert np.array_equal(records[:n_valid, :, :3], verts[faces[order[:n_valid]]])
    assert np.array_equal(words[:n_valid, 0, 3], order[:n_valid].astype(np.uint32)) and np.all(words[:n_valid, 1:, 3] == 0)
    assert np.all(np.isnan(records[n_valid:, :, :3])) and np.all(words[n_valid:, :, 3] == 0xFFFFFFFF)
    # every leaf is exactly the union of its valid members' boxes, every parent exactly the union of its children
    assert [lo.shape for lo, _ in levels] == [(count, 3) for count in L.counts] == [hi.shape for _, hi in levels]
    lo, hi = levels[0]
    for leaf in range(L.leaves):
        members = order[64 * leaf:64 * leaf + 64]
        corners = verts[faces[members[valid[members]]]].reshape(-1, 3)
        if corners.shape[0] == 0:
            assert np.all(lo[leaf] == np.inf) and np.all(hi[leaf] == -np.inf), leaf
        else:
            assert np.array_equal(lo[leaf], corners.min(axis=0)) and np.array_equal(hi[leaf], corners.max(axis=0)), leaf
    for level in range(1, L.top + 1):
        (lo, hi), (below_lo, below_hi) = levels[level], levels[level - 1]
        for p in range(L.counts[level]):
            assert np.array_equal(lo[p], below_lo[16 * p:16 * p + 16].min(axis=0)), (level, p)
            assert np.array_equal(hi[p], below_hi[16 * p:16 * p + 16].max(axis=0)), (level, p)
    if name == "empty boxes":
        assert L.counts == (35, 3) and all(np.all(levels[0][0][leaf] == np.inf) for leaf in range(17, 35))
        assert np.all(levels[1][0][2] == np.inf) and np.all(levels[1][1][2] == -np.inf) and np.all(np.isfinite(levels[1][0][:2]))
    if name == "shared tail leaf":
        tail = order[64 * 15:64 * 16]
        assert 0 < valid[tail].sum() < 64 and np.all(np.isfinite(levels[0][0][15])) and np.all(levels[0][0][16] == np.inf)
    if name == "none valid":
        assert all(np.all(lo == np.inf) and np.all(hi == -np.inf) for lo, hi in levels)
    if name == "overflowing centroid":       # +inf and -inf in the bounds: x and y collapse to cell 0, z still sorts
        cells_xy = codes[valid] & np.uint64(0x1249249249249249 | (0x1249249249249249 << 1))
        assert np.all(cells_xy == 0) and np.unique(codes[valid]).size > 100


def _leaf_diagonals(verts, faces, order):
    corners = verts.astype(np.float64)[faces[order]]                  # (all valid, F a multiple of nothing: the tail leaf is short)
    total = 0.0
    for at in range(0, order.size, 64):
        c = corners[at:at + 64].reshape(-1, 3)
        total += float(np.linalg.norm(c.max(axis=0) - c.min(axis=0)))
    return total


def test_plan_host_packs_neighbours_into_leaves():
    """A restatement whose order ignored where the faces lie would satisfy every invariant above.  On a 3000-face sphere in random
    face order the leaf boxes' diagonals sum to 156.8 when the faces are packed as given (47 leaves, each as wide as the sphere) and
    to 58.85 in ``plan_host``'s order: 2.66 times less, computed from the restatement alone, no kernel involved.  Half of that ratio
    is asserted: 1.33.  An order that does not follow the centroids (a code without its high word, which at this size holds all
    but the lowest ten bits per axis; a grid collapsed to one cell) gives about 1."""
    verts, faces = cases.sphere_with_faces(3000, seed=12)
    order, _, levels = meshquery.plan_host(verts, faces)
    packed, sorted_ = _leaf_diagonals(verts, faces, np.arange(3000)), _leaf_diagonals(verts, faces, order)
    print(f"summed leaf diagonals: {packed:.4g} in face order, {sorted_:.4g} in plan_host's order: {packed / sorted_:.3g} x")
    assert np.isclose(sorted_, np.linalg.norm((levels[0][1] - levels[0][0]).astype(np.float64), axis=1).sum(), rtol=1e-6)
    assert packed / sorted_ >= 0.5 * 2.66


# ---- the pruned restatement ---------------------------------------------------------------------------------------------------------
OVERFLOWING = np.array([[1e20, 0, 0], [3e38, -3e38, 1]], F32)


def _pruned_cases():
    out = {}
    verts, faces = cases.grid_plane(6, 5, 1.0)
    even = faces[::2]
    above = verts + np.asarray((0.0, 0.0, 0.75), F32)
    mids = ((verts[even[:, 0]] + verts[even[:, 2]]) * F32(0.5) + np.asarray((0.0, 0.0, 2.0), F32)).astype(F32)
    out["plane ties"] = (np.concatenate((above, mids, verts)), verts, faces)
    both = np.concatenate((faces, faces))
    out["duplicated faces"] = (cases.queries_near(verts, faces, 300, 1.5, seed=9), verts, both[np.random.default_rng(1).permutation(both.shape[0])])
    for kind, tri in _hard_triangles().items():
        tri = tri.astype(F32)[:120]
        q = np.concatenate((np.random.default_rng(4).uniform(-1, 1, (150, 3)).astype(F32), tri[::7, 0], tri[::5].mean(axis=1).astype(F32)))
        out["degenerate: " + kind] = (q, tri.reshape(-1, 3), np.arange(3 * tri.shape[0], dtype=np.int64).reshape(-1, 3))
    verts, faces, bad = cases.sphere_with_invalid(600, 100, seed=6)
    out["invalid faces"] = (cases.queries_near(verts[:-50], faces[np.setdiff1d(np.arange(700), bad)], 300, 0.4, seed=7), verts, faces)
    verts, faces = cases.sphere_with_faces(1300, seed=9)
    verts = verts.copy()
    verts[faces[17, 1]] = (1e4, -1e4, 1e4)
    far = np.array([[5e3, -5e3, 5e3], [1e4, -1e4, 1e4], [9e3, 0, 0], [0.3, -0.2, 0.5], [np.nan, 0, 0], [0, -np.inf, 0]], F32)
    out["far vertex"] = (np.concatenate((cases.queries_near(verts, faces, 300, 0.4, seed=10), far)), verts, faces)
    return out


@pytest.mark.parametrize("name", list(_pruned_cases()))
def test_pruned_restatement_equals_the_brute_force(name):
    q, verts, faces = _pruned_cases()[name]
    q = np.concatenate((q, OVERFLOWING))
    want = closest_triangles_host(q, verts, faces)
    bits = lambda t: np.ascontiguousarray(t).view(np.uint32) if t.dtype == F32 else t
    for chunk in (1 << 20, 1, 997):
        got = closest_triangles_host(q, verts, faces, chunk_elems=chunk, pruned=True)
        assert all(a.dtype == b.dtype and np.array_equal(bits(a), bits(b)) for a, b in zip(got, want)), chunk
    fine = np.all(np.isfinite(q), axis=1)
    assert np.all(want[0][fine] >= 0) and np.all(want[0][~fine] == -1) and np.all(np.isposinf(want[1][-2:]))


def test_direct_calls_raise_value_error_with_the_reason():
    v, f, p = _gpu(8, 3), _gpu(4, 3, dtype=torch.int64), _gpu(5, 3)
    with pytest.raises(ValueError, match="GPU"):
        meshquery.closest_triangles(torch.zeros(5, 3), torch.zeros(8, 3), torch.zeros(4, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="GPU"):
        meshquery.plan(torch.zeros(8, 3), torch.zeros(4, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="GPU"):
        meshquery.closest_triangles(torch.zeros(5, 3), v, f)
    with pytest.raises(ValueError, match="faces must be int64"):
        meshquery.closest_triangles(p, v, _gpu(4, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match="verts must be float32"):
        meshquery.plan(_gpu(8, 3, dtype=torch.float64), f)
    with pytest.raises(ValueError, match=r"\[V, 3\]"):
        meshquery.plan(_gpu(8, 2), f)
    with pytest.raises(ValueError, match=r"\[F, 3\]"):
        meshquery.plan(v, _gpu(4, 4, dtype=torch.int64))
    with pytest.raises(ValueError, match="points must be float32"):
        meshquery.closest_triangles(_gpu(5, 3, dtype=torch.float16), v, f)
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        meshquery.closest_triangles(_gpu(5, 2), v, f)
    with pytest.raises(ValueError, match="torch.Tensor"):
        meshquery.closest_triangles(np.zeros((5, 3), F32), v, f)
    with pytest.raises(ValueError, match="not of this one"):
        meshquery.closest_triangles(p, v, f, plan=meshquery.Plan(_gpu(512, dtype=torch.uint8), 9, 8))
    with pytest.raises(ValueError, match="a plan of 4 faces is 768 bytes"):    # header 256, records 4 x 48 -> 256, one box -> 256
        meshquery.closest_triangles(p, v, f, plan=meshquery.Plan(_gpu(512, dtype=torch.uint8), 4, 8))
    with pytest.raises(ValueError, match="meshquery.Plan"):
        meshquery.closest_triangles(p, v, f, plan=object())


def test_morton_order_is_a_permutation_that_groups_neighbours():
    g = np.random.default_rng(12)
    pts = g.uniform(-1, 1, (5000, 3)).astype(F32)
    pts[17], pts[99, 1], pts[4000, 2] = np.nan, np.inf, -np.inf
    order = meshquery.morton_order(torch.tensor(pts)).numpy()
    assert np.array_equal(np.sort(order), np.arange(5000))
    fine = np.all(np.isfinite(pts[order]), axis=1)
    groups = pts[order][fine][:4928].reshape(-1, 64, 3)            # 64 consecutive queries: one wave
    spread = (groups.max(axis=1) - groups.min(axis=1)).max(axis=1)
    # an octree cell 0.5 wide holds 5000 / 64 = 78 of these points, so 64 consecutive ones mostly stay inside its parent, 1.0 wide;
    # in the drawn order a wave's box is nearly the whole cube, 2 wide
    drawn = pts[np.all(np.isfinite(pts), axis=1)][:4928].reshape(-1, 64, 3)
    assert np.median(spread) <= 1.0 < 1.8 < np.median((drawn.max(axis=1) - drawn.min(axis=1)).max(axis=1))
    one = meshquery.morton_order(torch.zeros((7, 3)))              # no extent: any order will do
    assert sorted(one.tolist()) == list(range(7))


# ---- the frame loop's option --------------------------------------------------------------------------------------------------------
def _load_by_path(name, path):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_melt_closest_mode_reads_the_variable(monkeypatch):
    monkeypatch.delenv("AUTOVFX_AMD_MELT_CLOSEST", raising=False)
    assert frame_loop.melt_closest_mode() == "host"
    for value in ("host", "gpu"):
        monkeypatch.setenv("AUTOVFX_AMD_MELT_CLOSEST", value)
        assert frame_loop.melt_closest_mode() == value
    for value in ("", "GPU", "1", "open3d"):
        monkeypatch.setenv("AUTOVFX_AMD_MELT_CLOSEST", value)
        with pytest.raises(ValueError, match="AUTOVFX_AMD_MELT_CLOSEST"):
            frame_loop.melt_closest_mode()


class _Loaded(Exception):
    pass


class _SceneThatMustNotLoad:
    def load_scene(self):
        raise _Loaded()


def test_a_wrong_value_raises_at_the_start_of_the_call(monkeypatch):
    scene = _SceneThatMustNotLoad()
    monkeypatch.setenv("AUTOVFX_AMD_MELT_CLOSEST", "embree")
    with pytest.raises(ValueError, match="embree"):
        frame_loop.render_from_3DGS(scene)
    monkeypatch.setenv("AUTOVFX_AMD_MELT_CLOSEST", "host")
    with pytest.raises(_Loaded):                       # a right one gets as far as the scene
        frame_loop.render_from_3DGS(scene)


@pytest.mark.parametrize("value", [None, "host"])
def test_unset_and_host_ask_the_modules_own_o3d(monkeypatch, tmp_path, value):
    """The default melting plan, with doubles for everything around it: the closest-triangle questions go to ``mod.o3d`` -- once per
    object for the Gaussians, once per frame and melting mesh for the centres -- and the masks are ``np.isin`` of its answers."""
    trimesh = _load_by_path("_mq_shims_trimesh", os.path.join(HERE, "shims", "trimesh", "__init__.py"))
    o3d = _load_by_path("_mq_shims_open3d", os.path.join(HERE, "shims", "open3d", "__init__.py"))
    asked = []
    real = o3d.RaycastingScene.compute_closest_points
    monkeypatch.setattr(o3d.RaycastingScene, "compute_closest_points", lambda self, pts: (asked.append(len(pts)), real(self, pts))[1])
    monkeypatch.setattr(frame_loop, "_make_mesh_scene", lambda *a: pytest.fail("the GPU path was taken"))
    if value is None:
        monkeypatch.delenv("AUTOVFX_AMD_MELT_CLOSEST", raising=False)
    else:
        monkeypatch.setenv("AUTOVFX_AMD_MELT_CLOSEST", value)

    root = str(tmp_path)
    os.makedirs(os.path.join(root, "assets", "chair", "mesh"))
    verts, faces = cases.grid_plane(3, 3, 1.0)
    mesh_path = os.path.join(root, "assets", "chair", "mesh", "chair.obj")
    trimesh.save_mesh(mesh_path, verts, faces)
    melting = os.path.join(root, "cache", "blend", "melting_meshes")
    os.makedirs(os.path.join(melting, "chair"))
    trimesh.save_mesh(os.path.join(melting, "chair", "001_obj.stl"), verts[:8], faces[:4])
    trimesh.save_mesh(os.path.join(melting, "chair", "002_obj.stl"), verts, faces[:6])
    trimesh.save_mesh(os.path.join(melting, "chair", "002_obj_dup.stl"), verts, faces[10:13])
    xyz = torch.tensor(cases.queries_near(verts, faces, 40, 0.3, seed=8))
    gaussians = types.SimpleNamespace(_xyz=xyz, active_sh_degree=3)
    mod = types.SimpleNamespace(o3d=o3d, trimesh=trimesh, load_gaussians=lambda path, degree: gaussians)
    scene = types.SimpleNamespace(
        rb_transform_info=None, blender_cache_dir=os.path.join(root, "cache"), gaussians=gaussians,
        hparams=types.SimpleNamespace(blender_output_dir_name="blend", max_sh_degree=4),
        blender_cfg={"insert_object_info": [{"object_id": "chair", "object_path": mesh_path}]})
    composed = []
    dynamic = types.SimpleNamespace(compose_model=lambda placed, slot=0: (composed.append(placed), "model")[1])
    monkeypatch.setattr(frame_loop, "_make_dynamic_scene", lambda *a: dynamic)

    plan = frame_loop._plan(scene, mod, 3, 1, frame_loop.melt_closest_mode())
    assert isinstance(plan, frame_loop._MeltingPlan) and plan.closest == "host" and asked == [40]
    assert plan.model_for_frame(0, 0) == "model" and asked == [40, 4]
    assert plan.model_for_frame(1, 0) == "model" and asked == [40, 4, 6, 3]
    assert plan.model_for_frame(2, 0) is gaussians and len(asked) == 4           # no mesh for frame 003: the scene's own model
    scene_double = o3d.RaycastingScene()
    scene_double.add_triangles(trimesh.load_mesh(mesh_path))
    ids_g = real(scene_double, xyz.numpy())["primitive_ids"].numpy()
    centres = np.array(trimesh.load_mesh(os.path.join(melting, "chair", "002_obj_dup.stl")).triangles_center).astype(F32)
    want = np.isin(ids_g, real(scene_double, centres)["primitive_ids"].numpy())
    assert [len(p) for p in composed] == [1, 2]
    got = composed[1][1]
    assert got[:4] == ("chair", None, None, None) and isinstance(got[4], np.ndarray) and np.array_equal(got[4], want)
