"""The closest-triangle plan and walk (gsr_meshquery.hip) where tests/test_meshquery_gpu.py does not reach.

* The plan itself, region by region, against ``meshquery.plan_host``: the search is exact on any tree whose boxes contain their
  members, so a Morton sort that lost its high word, a grid collapsed to one cell or a parent ten times too large answer every query
  right and only cost time.  Comparing answers cannot see them; comparing the buffer does.
* The walk on trees of three and four box levels (F = 262144 and 262145; test_meshquery_gpu.py stops at 16385, three levels with two
  boxes on top), all three outputs bit for bit against the pruned mode of ``closest_triangles_host``, asked in Morton order and in
  the caller's (shuffled) order: a sphere, the same sphere far from the origin, an integer plane in random face order with exact
  ties across leaves, and a mesh with leaves as large as the mesh.
* Trees with wholly empty leaves and parents, boxes of (+inf, -inf), which the walk must neither open nor trip over.

Every deep mesh is asked at most 192 queries: the numpy reference is the cost (under a second per mesh), the GPU side milliseconds.
Not run, for that cost: trees of five and six levels (F > 4.2 M and F > 67 M)."""
from __future__ import annotations

import time

import numpy as np
import pytest

from autovfx_amd import meshquery
from autovfx_amd.meshquery import closest_triangles_host, plan_host, plan_layout

import meshquery_cases as cases
from test_meshquery_gpu import _on_gpu, _queries, assert_same_bits

pytestmark = pytest.mark.gpu
F32 = np.float32
OVERFLOWING = np.array([[1e20, 0, 0], [3e38, -3e38, 1]], F32)      # every squared distance is +inf: nothing is pruned, face 0 wins
MAX_QUERIES = 192


# ---- the plan, region by region -----------------------------------------------------------------------------------------------------
def assert_same_plan(verts, faces, what=""):
    """``meshquery.plan``'s buffer against ``plan_host``.  Compared: the header's three fields, every record, every box of every
    level.  Not compared: the 240 bytes after the header's fields and the padding between the regions (never written)."""
    F = faces.shape[0]
    L = plan_layout(F)
    order, records, levels = plan_host(verts, faces)
    _, tv, tf = _on_gpu(np.zeros((1, 3), F32), verts, faces)
    plan = meshquery.plan(tv, tf)
    raw = plan.buffer.cpu().numpy()
    assert raw.dtype == np.uint8 and raw.shape == (L.bytes,), (what, raw.shape, L)
    assert raw[:4].tobytes() == meshquery.PLAN_MAGIC and int(raw[4:8].view(np.uint32)[0]) == F, (what, raw[:8])
    assert int(raw[8:16].view(np.uint64)[0]) == L.bytes, what

    got = raw[L.records:L.records + 48 * F].view(np.uint32).reshape(F, 3, 4)
    want = records.view(np.uint32)
    named = got[:, 0, 3].astype(np.int64)
    bad = np.nonzero(named != want[:, 0, 3])[0]
    assert bad.size == 0, (what, "the order of the records: first at", bad[:5], "face", named[bad[:5]], "for", order[bad[:5]], "of", bad.size)
    live = want[:, 0, 3] != meshquery.NO_FACE
    bad = np.nonzero((got[live] != want[live]).any(axis=(1, 2)))[0]
    assert bad.size == 0, (what, "records", bad[:5], got[live][bad[:5]], want[live][bad[:5]])
    # an invalid record: NaN in x, y, z (whichever NaN) and ~0 in w, all three rows
    dead = got[~live]
    assert np.all(np.isnan(dead[:, :, :3].view(F32))) and np.all(dead[:, :, 3] == meshquery.NO_FACE), (what, "invalid records")

    # Boxes by value, -0 equal to +0: a box is a min / max reduction, and IEEE min(-0, +0) may return either, so the sign of a zero
    # depends on the order of the reduction (64 lanes by butterfly here, a numpy loop there).  No box holds a NaN.
    for level, (lo, hi) in enumerate(levels):
        at = L.boxes + 32 * L.offsets[level]
        box = raw[at:at + 32 * L.counts[level]].view(F32).reshape(L.counts[level], 2, 4)
        for name, g, w in (("lo", box[:, 0, :3], lo), ("hi", box[:, 1, :3], hi)):
            bad = np.nonzero((g != w).any(axis=1))[0]
            assert bad.size == 0, (what, f"level {level} {name}: first at", bad[:5], g[bad[:5]], w[bad[:5]], "of", bad.size)
    return order, records, levels


@pytest.mark.parametrize("F", [1, 64, 65, 1024, 1025, 16384, 16385, 262144, 262145])
def test_plan_at_every_tree_shape(F):
    verts, faces = cases.sphere_with_faces(F, seed=F)
    _, _, levels = assert_same_plan(verts, faces, f"F = {F}")
    assert len(levels) == plan_layout(F).top + 1 == {1: 1, 64: 1, 65: 1, 1024: 1, 1025: 2, 16384: 2, 16385: 3, 262144: 3, 262145: 4}[F]


def _far_vertex():
    verts, faces = cases.sphere_with_faces(1300, seed=9)
    verts = verts.copy()
    verts[faces[17, 1]] = (1e4, -1e4, 1e4)
    return verts, faces


def _duplicated():
    verts, faces = cases.sphere_with_faces(300, seed=2)
    return verts, np.concatenate([faces] * 8)            # eight equal codes in a row, 2400 faces: runs that cross leaf seams


PLAN_MESHES = {
    "flat integer plane": lambda: cases.grid_plane(30, 20, 1.0),                     # extent 0 in z: cell 0 for every face
    "flat plane, random face order": lambda: cases.plane_in_random_order(37, 29, seed=3),
    "every face eight times": _duplicated,
    "one vertex at 1e4": _far_vertex,
    "overflowing centroid": lambda: cases.sphere_with_overflowing_centroid(700, seed=3),
    "overflowing centroid, one face": lambda: cases.sphere_with_overflowing_centroid(1, seed=3),
    "empty boxes": lambda: cases.sphere_with_invalid(16384, 1216, seed=4)[:2],
    "shared tail leaf": lambda: cases.sphere_with_invalid(16350, 1250, seed=4)[:2],
    "spanners and slivers": lambda: cases.sphere_with_spanners(20000, 50, 200, seed=5),
}


@pytest.mark.parametrize("name", list(PLAN_MESHES))
def test_plan_of_the_hard_meshes(name):
    verts, faces = PLAN_MESHES[name]()
    order, _, levels = assert_same_plan(verts, faces, name)
    if name == "every face eight times":       # the eight copies of a face are neighbours, in ascending index
        runs = order.reshape(-1, 8)
        assert np.all(runs % 300 == runs[:, :1] % 300) and np.all(np.diff(runs, axis=1) == 300)
    if name == "overflowing centroid":         # the bounds hold +inf in x and -inf in y: both collapse, z still sorts
        x_and_y = np.uint64(0x1249249249249249 | (0x1249249249249249 << 1))
        codes = meshquery.morton_codes_host(verts, faces)
        assert np.all(codes & x_and_y == 0) and np.unique(codes).size > 100


# ---- the deep meshes and their references -------------------------------------------------------------------------------------------
def _sphere_queries(verts, faces, centre, seed):
    """Within two median edge lengths of the surface; corners, edge midpoints and centroids of faces; three far points, three
    non-finite ones (``_queries`` of test_meshquery_gpu.py); the sphere's centre, from where almost no box is farther than the nearest
    corner, so nothing is pruned at a finite distance; the two queries whose distances overflow, where nothing is pruned at all."""
    valid = meshquery.valid_faces_host(verts, faces)
    edge = float(np.median(cases.edge_lengths(verts, faces[valid])))
    q = _queries(verts, faces, 140, 2.0 * edge, seed=seed)
    return np.concatenate((q, np.asarray([centre], F32), OVERFLOWING)).astype(F32)


def _plane_queries(verts, faces, nx, ny, seed):
    """0.75 above 60 vertices, 60 midpoints of grid edges and 60 midpoints of cell diagonals.  At each, the faces that hold the
    vertex (or both ends of the edge) are at 0.5625 exactly, up to six of them: returns the queries, the lowest such face of each
    and the tying faces' indices."""
    g = np.random.default_rng(seed)
    i, j = g.integers(0, nx, 180), g.integers(0, ny, 180)
    i[:4], j[:4] = (0, 0, nx, 5), (0, ny, 0, 0)                       # the border too: two faces, one, one, three
    at = lambda a, b: a * (ny + 1) + b
    ends = np.stack((at(i, j), at(i, j)), -1)                         # a vertex: both ends the same
    along_x = np.arange(60) % 2 == 0
    ends[60:120, 1] = np.where(along_x, at(i[60:120] + 1, j[60:120]), at(i[60:120], j[60:120] + 1))
    ends[120:, 1] = at(i[120:] + 1, j[120:] + 1)
    q = ((verts[ends[:, 0]] + verts[ends[:, 1]]) * F32(0.5) + np.asarray((0, 0, 0.75), F32)).astype(F32)
    tying = [np.nonzero((faces == v0).any(axis=1) & (faces == v1).any(axis=1))[0] for v0, v1 in ends]
    return q, np.asarray([t.min() for t in tying]), tying


def _build(name):
    extra = {}
    if name in ("sphere F=262144", "sphere F=262145"):
        F = int(name.split("=")[1])
        verts, faces = cases.sphere_with_faces(F, seed=F)
        q = _sphere_queries(verts, faces, (0.3, -0.2, 0.5), seed=F)
    elif name == "sphere at (4096, -2048, 8192)":
        # the same faces; the coordinates' spacing there (2^-12, 2^-11 and 2^-10 on the three axes) is about a twentieth of an edge
        # (0.014): near-ties and exact ties everywhere
        centre = (4096.3, -2048.2, 8192.5)
        verts, faces = cases.sphere_with_faces(262144, seed=262144, centre=centre)
        q = _sphere_queries(verts, faces, centre, seed=32)
    elif name == "integer plane, random face order":
        verts, faces = cases.plane_in_random_order(363, 362, seed=33)          # 262812 faces
        q, extra["expect"], extra["tying"] = _plane_queries(verts, faces, 363, 362, seed=34)
        q = np.concatenate((q, OVERFLOWING, np.array([[np.nan, 0, 0], [0, np.inf, 0], [1, 2, -np.inf]], F32)))
    elif name == "spanners and slivers":
        verts, faces = cases.sphere_with_spanners(20000, 50, 200, seed=5)
        q = _sphere_queries(verts, faces, (0.3, -0.2, 0.5), seed=35)
    elif name in ("empty boxes", "shared tail leaf"):
        valid, invalid = (16384, 1216) if name == "empty boxes" else (16350, 1250)
        verts, faces, extra["bad"] = cases.sphere_with_invalid(valid, invalid, seed=4)
        q = _sphere_queries(verts, faces, (0.3, -0.2, 0.5), seed=36)
    assert len(q) <= MAX_QUERIES
    # the caller's order, shuffled: the 64 queries of a wave span the mesh (the surface points, the far ones and the rest mixed)
    shuffle = np.random.default_rng(37).permutation(len(q))
    q = np.ascontiguousarray(q[shuffle])
    where = np.argsort(shuffle)                                      # where the query built at k went
    t0 = time.perf_counter()
    want = closest_triangles_host(q, verts, faces, pruned=True)
    print(f"\n[{name}] {faces.shape[0]} faces, {len(q)} queries: reference in {time.perf_counter() - t0:.2f} s on the host")
    tq, tv, tf = _on_gpu(q, verts, faces)
    return dict(name=name, q=q, verts=verts, faces=faces, want=want, tq=tq, tv=tv, tf=tf, plan=meshquery.plan(tv, tf), where=where, **extra)


DEEP = ["sphere F=262144", "sphere F=262145", "sphere at (4096, -2048, 8192)", "integer plane, random face order",
        "spanners and slivers", "empty boxes", "shared tail leaf"]


@pytest.fixture(scope="module", params=DEEP)
def deep(request):
    return _build(request.param)


# ---- the walk -----------------------------------------------------------------------------------------------------------------------
def test_walk_asked_in_morton_order(deep):
    got = meshquery.closest_triangles(deep["tq"], deep["tv"], deep["tf"], plan=deep["plan"], return_points=True)
    assert_same_bits(got, deep["want"], deep["name"])


def test_walk_asked_in_the_callers_order(deep):
    got = meshquery._query(deep["tq"], deep["plan"], True, sort_queries=False)
    assert_same_bits(got, deep["want"], deep["name"] + ", caller's order")


def test_the_reference_is_what_the_case_is_for(deep):
    """What the two tests above compare with, looked at on its own: only the non-finite queries miss, no closest point is NaN (bits
    of a NaN would compare unequal for no reason), and each case really holds what it was built for."""
    name, q, verts, faces, (idx, d, closest) = (deep[k] for k in ("name", "q", "verts", "faces", "want"))
    fine = np.all(np.isfinite(q), axis=1)
    assert (~fine).sum() == 3 and np.array_equal(idx >= 0, fine) and not np.isnan(closest).any() and not np.isnan(d).any()
    valid = meshquery.valid_faces_host(verts, faces)
    assert valid[idx[fine]].all()
    # the overflowing queries: +inf from every face, so the lowest valid face
    over = np.nonzero((np.abs(q) >= 1e20).any(axis=1) & fine)[0]
    assert over.size == 2 and np.all(np.isposinf(d[over])) and np.all(idx[over] == np.nonzero(valid)[0][0])
    L = plan_layout(faces.shape[0])
    if name.startswith("sphere"):
        assert L.top == (3 if faces.shape[0] == 262145 else 2) and (d == 0).sum() >= 12          # the corners lie on their faces
    if name in ("sphere F=262144", "sphere F=262145"):
        # the centre: the nearest corner is no nearer than almost any face's own box, so a bound prunes next to nothing
        c = np.asarray((0.3, -0.2, 0.5), F32)
        at = np.nonzero((q == c).all(axis=1))[0]
        assert at.size == 1
        tri = meshquery.triangle_distance_host(c, *(verts[faces[:, k]] for k in range(3)))
        assert (tri["d_box"] <= tri["d_vtx"].min()).mean() > 0.9 and abs(float(d[at[0]]) - 1.0) < 1e-3
    if name == "integer plane, random face order":
        expect, tying, where = deep["expect"], deep["tying"], deep["where"][:180]
        assert np.array_equal(idx[where], expect) and np.all(d[where] == F32(0.5625))
        ties = np.asarray([t.size for t in tying])
        assert ties.max() == 6 and ties.min() == 1 and (ties[:60] == 6).sum() >= 50 and (ties[60:] == 2).sum() >= 100
        leaf_of = np.empty(faces.shape[0], np.int64)
        leaf_of[plan_host(verts, faces)[0]] = np.arange(faces.shape[0]) // 64
        seams = sum(np.unique(leaf_of[t]).size > 1 for t in tying)
        print(f"{seams} of {len(tying)} ties cross a leaf seam")
        assert seams >= 30                                            # the lowest of the tying faces wins across leaves
    if name == "spanners and slivers":
        _, _, levels = plan_host(verts, faces)
        width = (levels[0][1] - levels[0][0]).max(axis=1)
        assert (width > 1.9).sum() >= 3 and L.top == 2                                         # leaves as wide as the mesh (2.0)
    if name in ("empty boxes", "shared tail leaf"):
        bad = deep["bad"]
        assert np.array_equal(np.nonzero(~valid)[0], bad) and not np.isin(idx, bad).any()
        half = bad.size // 2
        assert (faces[bad] >= verts.shape[0]).any(axis=1).sum() + (faces[bad] < 0).any(axis=1).sum() >= half
        order, _, levels = plan_host(verts, faces)
        empty = [np.all(lo == np.inf, axis=1) & np.all(hi == -np.inf, axis=1) for lo, hi in levels]
        assert L.counts == (275, 18, 2) and all(np.all(np.isfinite(lo[~e])) and np.all(np.isfinite(hi[~e])) for (lo, hi), e in zip(levels, empty))
        assert np.array_equal(np.nonzero(empty[0])[0], np.arange(256, 275))
        assert np.array_equal(np.nonzero(empty[1])[0], [16, 17]) and np.array_equal(np.nonzero(empty[2])[0], [1])
        shared = valid[order[64 * 255:64 * 256]].sum()
        assert shared == (64 if name == "empty boxes" else 30)
