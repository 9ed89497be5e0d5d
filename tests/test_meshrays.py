"""The first-hit contract as meshquery.first_hits_host restates it, on the CPU: against a float64 truth where the truth
is well conditioned, its pruned form against brute force bit for bit, and the ties, misses and flat boxes the contract speaks of."""
from __future__ import annotations

import numpy as np
import pytest

from autovfx_amd import meshquery
from autovfx_amd.meshquery import first_hits_host

import meshquery_cases as cases
import meshrays_cases as rays

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same(got, want, what=""):
    assert np.array_equal(got[0], want[0]), (what, "face_idx", np.nonzero(got[0] != want[0])[0][:5])
    assert np.array_equal(_bits(got[1]), _bits(want[1])), (what, "t", np.nonzero(_bits(got[1]) != _bits(want[1]))[0][:5])
    assert np.array_equal(_bits(got[2]), _bits(want[2])), (what, "bary")


@pytest.mark.parametrize("sub", [2, 3])
@pytest.mark.parametrize("origin", [(0.1, 0.2, -0.15), (0.0, 0.0, 0.0), (0.5, 0.5, 0.5)])
def test_icosphere_from_inside_misses_nothing_and_meets_the_float64_truth(sub, origin):
    """Rays from inside a closed mesh through every vertex, edge midpoint and centroid, and 500 random ones: every ray hits, and
    every ray whose float64 hit lies more than 1e-4 (barycentric) inside its face has that face; at least half of the rays do."""
    verts, faces = rays.icosphere(sub)
    o, d = rays.rays_through_features(verts, faces, origin)
    face, t, bary = first_hits_host(o, d, verts, faces)
    assert face.dtype == np.int64 and t.dtype == F32 and bary.dtype == F32 and bary.shape == (len(o), 3)
    assert (face >= 0).all() and np.isfinite(t).all() and (t > 0).all()
    want, want_t, margin = rays.truth64(o, d, verts, faces)
    safe = margin > 1e-4
    print(f"sub {sub} origin {origin}: {len(o)} rays, {int(safe.sum())} with a margin above 1e-4")
    # every ray through a centroid (margin 1/3) and nearly every random one has the margin; the rays aimed at a vertex or an edge
    # midpoint have it only where rounding the fp32 direction moved them off the edge.  On 320 faces that makes more than half of the
    # 1462 rays (820 from the first origin); on 1280 faces 2562 of the 4342 rays are aimed at a vertex or an edge, so half cannot be.
    assert int(safe.sum()) >= len(faces) + 450
    if sub == 2:
        assert 2 * int(safe.sum()) >= len(o)
    assert np.array_equal(face[safe], want[safe])
    # t and the barycentrics are those of the truth up to rounding (fp32 inputs: a few ulp of the coordinates' scale)
    assert np.abs(t[safe] - want_t[safe]).max() <= 1e-5 * np.abs(want_t[safe]).max()
    assert np.abs(bary.sum(1) - 1).max() <= 1e-5 and bary[safe].min() > 0
    hit = o + t[:, None] * d
    corners = verts[faces[face]]
    assert np.abs((corners * bary[:, :, None]).sum(1) - hit)[safe].max() <= 1e-5


def test_pruned_equals_brute_force_on_16385_faces():
    verts, faces = rays.rippled_sphere(16385, seed=3)
    o, d = rays.mixed_rays(verts, 192, seed=4)
    brute = first_hits_host(o, d, verts, faces)
    assert_same(first_hits_host(o, d, verts, faces, pruned=True), brute, "pruned")
    assert_same(first_hits_host(o, d, verts, faces, pruned=True, chunk_elems=1 << 17), brute, "pruned, smaller chunks")
    hits = int((brute[0] >= 0).sum())
    assert 96 <= hits < 192                                      # hits and misses both


_closed_faces_at = rays.closed_faces_at


@pytest.mark.parametrize("down", [True, False])
def test_ties_go_to_the_lowest_face_index(down):
    """Integer coordinates make every tie exact: a ray through a shared vertex hits up to six faces at one t, a ray through the
    midpoint of a shared edge two; a duplicated face ties with its copy everywhere."""
    verts, faces = cases.plane_in_random_order(9, 7, seed=5)         # 126 faces in z = 0
    z = 2.0 if down else -3.0
    at = [(float(i), float(j)) for i in range(10) for j in range(8)]                     # vertices
    at += [(i + 0.5, float(j)) for i in range(9) for j in range(8)]                      # midpoints of the edges along x
    at += [(float(i), j + 0.5) for i in range(10) for j in range(7)]                     # ... along y
    at += [(i + 0.5, j + 0.5) for i in range(9) for j in range(7)]                       # ... of the diagonals
    o = np.array([(x, y, z) for x, y in at], F32)
    d = np.broadcast_to(np.array([0, 0, -4.0 if down else 0.5], F32), o.shape)
    face, t, bary = first_hits_host(o, d, verts, faces)
    shared = [_closed_faces_at(verts, faces, x, y) for x, y in at]
    assert max(len(s) for s in shared) == 6 and min(len(s) for s in shared) == 1
    assert np.array_equal(face, np.array([s.min() for s in shared]))
    assert np.array_equal(t, np.full(len(at), 0.5 if down else 6.0, F32))
    twice = np.concatenate((faces, faces))
    again = first_hits_host(o, d, verts, twice)
    assert_same(again, (face, t, bary), "every face duplicated")
    flipped = np.concatenate((faces[::-1], faces))                   # the copy with the lower index is the one of faces[::-1]
    assert np.array_equal(first_hits_host(o, d, verts, flipped)[0], np.array([(len(faces) - 1 - s).min() for s in shared]))


def test_what_misses():
    verts, faces = rays.icosphere(2)
    inside = np.zeros(3, F32)
    g = np.random.default_rng(2)
    d = g.normal(size=(40, 3)).astype(F32)
    o = np.broadcast_to(inside, d.shape).copy()
    # a non-finite component, a zero direction
    o[1, 0], o[2, 2], d[3, 1], d[4, 0], d[5] = np.nan, np.inf, -np.inf, np.nan, 0.0
    d[6] = (0.0, -0.0, 0.0)
    face, t, bary = first_hits_host(o, d, verts, faces)
    missed = np.arange(40) < 7
    missed[0] = False
    assert (face[missed] == -1).all() and np.isposinf(t[missed]).all() and (bary[missed] == 0).all()
    assert (face[~missed] >= 0).all()
    # from outside, pointing away: the line meets the sphere, the ray (t >= 0) does not
    out = (3.0 * d[10:] / np.linalg.norm(d[10:], axis=1, keepdims=True)).astype(F32)
    face, t, _ = first_hits_host(out, out, verts, faces)
    assert (face == -1).all() and np.isposinf(t).all()
    assert (first_hits_host(out, -out, verts, faces)[0] >= 0).all()
    # no face at all, no valid face
    assert (first_hits_host(o, d, verts, faces[:0])[0] == -1).all()
    assert (first_hits_host(o, d, verts, faces + len(verts))[0] == -1).all()


def test_invalid_faces_are_never_hit():
    verts, faces, bad = cases.sphere_with_invalid(900, 100, seed=8)
    o, d = rays.mixed_rays(verts[np.isfinite(verts).all(1)], 150, seed=9)
    got = first_hits_host(o, d, verts, faces)
    keep = np.setdiff1d(np.arange(len(faces)), bad)
    assert np.array_equal(keep, np.nonzero(meshquery.valid_faces_host(verts, faces))[0])
    only = first_hits_host(o, d, verts, faces[keep])
    assert (got[0] >= 0).sum() >= 50 and not np.isin(got[0], bad).any()
    assert_same(got, (np.where(only[0] >= 0, keep[only[0]], -1), only[1], only[2]), "the valid faces alone")


def test_axis_parallel_rays_and_flat_boxes():
    """d_k == 0 on two axes, and every face's own box is flat on one: rays through the cube's corners, edges and faces all hit, at
    the exact distance."""
    verts, faces = rays.cube()
    grid = np.array([0, 0.25, 0.5, 1], F32)
    base = np.array([[x, y, -1.5] for x in grid for y in grid], F32)
    for axis in range(3):
        o = np.roll(base, axis + 1, 1)
        for sign, want in ((1.0, 1.5), (-1.0, None)):
            d = np.zeros_like(o)
            d[:, axis] = 2.0 * sign
            face, t, bary = first_hits_host(o, d, verts, faces)
            if want is None:
                assert (face == -1).all()
                continue
            assert (face >= 0).all() and np.array_equal(t, np.full(len(o), want / 2.0, F32)), (axis, t)
            assert (verts[faces[face]][:, :, axis] == 0).all()       # the near side
            assert_same(first_hits_host(o, d, verts, faces, pruned=True), (face, t, bary), "pruned")
        inside = o.copy()
        inside[:, axis] = 0.5
        d = np.zeros_like(o)
        d[:, axis] = -1.0
        face, t, _ = first_hits_host(inside, d, verts, faces)
        assert (face >= 0).all() and np.array_equal(t, np.full(len(o), 0.5, F32))


def test_the_clamp_moves_t_by_rounding_error_only():
    verts, faces = rays.icosphere(3)
    o, d = rays.rays_through_features(verts, faces, (0.1, 0.2, -0.15), extra=100)
    face, t, _ = first_hits_host(o, d, verts, faces)
    got = meshquery.ray_triangle_host(o, d, *(verts[faces[face, k]] for k in range(3)))
    assert got["hit"].all() and np.array_equal(got["t"], t)
    # both t_tri (a dozen rounded operations) and the interval's ends (two each, and the pad of 2 ulp) are within a few ulp of the truth
    assert np.abs(got["t"] - got["t_tri"]).max() <= 16 * np.finfo(F32).eps * t.max()
    assert (got["t_enter"] <= got["t"]).all() and (got["t"] <= got["t_exit"]).all()


# ---- the branches of the contract, family by family (meshrays_cases; tests/test_meshrays_gpu.py asks the kernel the same rays) --------
def _both_forms(case, what):
    """The brute-force answers of the restatement, which its pruned form must equal in their bits."""
    with np.errstate(all="ignore"):
        brute = first_hits_host(case.o, case.d, case.verts, case.faces)
        assert_same(first_hits_host(case.o, case.d, case.verts, case.faces, pruned=True), brute, what + ", pruned")
    return brute


@pytest.mark.parametrize("mesh", ["cube", "icosphere"])
def test_every_shear_and_the_ties_between_them(mesh):
    case = rays.shears(mesh)
    rays.expect_shears(case, *_both_forms(case, mesh))


def test_axis_parallel_rays_from_both_sides_with_negative_zeros():
    case = rays.axis_parallel()
    rays.expect_axis_parallel(case, *_both_forms(case, "axis-parallel"))


def test_the_clamp_is_active_on_flat_boxes():
    """At least one hit in twenty has t != t_tri at every distance, and over the three both ends of the interval are taken."""
    enter = leave = 0
    for distance in (3.0, 1e2, 1e4):
        case = rays.oblique_onto_cube(distance)
        counts = rays.expect_oblique_onto_cube(case, *_both_forms(case, f"from {distance}"))
        enter, leave = enter + counts[1], leave + counts[2]
    assert enter >= 1 and leave >= 1


def test_origins_on_the_surface_and_faces_without_area():
    case = rays.surface_origins()
    rays.expect_surface_origins(case, *_both_forms(case, "origins on the surface"))


def test_denormal_components_and_overflow():
    case = rays.denormal_rays()
    rays.expect_denormal_rays(case, *_both_forms(case, "denormal components"))
    rays.expect_all_miss(case.huge, *_both_forms(case.huge, "coordinates of 1e38"))


@pytest.mark.parametrize("F", [1025, 16385])
def test_comb_rays_that_prune_nothing_and_exact_hits(F):
    case = rays.comb(F)
    rays.expect_comb(case, *_both_forms(case, f"a comb of {F}"))


def test_ties_between_the_leaves_of_a_plan():
    case = rays.copies()
    rays.expect_copies(case, *_both_forms(case, "301 copies of one face"))
    case = rays.plane_vertex_rays(9, 7, 5)
    assert len(case.o) == 6 * 80
    rays.expect_plane_vertex_rays(case, *_both_forms(case, "diagonal rays through the vertices of a plane"))


def test_four_levels_pruned_in_two_chunk_sizes():
    case = rays.four_levels()
    got = first_hits_host(case.o, case.d, case.verts, case.faces, pruned=True)
    assert_same(first_hits_host(case.o, case.d, case.verts, case.faces, pruned=True, chunk_elems=1 << 17), got, "smaller chunks")
    rays.expect_four_levels(case, *got)
