"""autovfx_amd.meshloss without a GPU: the numpy restatements of the contract against pytorch3d's route in float64 and on exact cases, the
drop-in's plumbing, the hook's row for ``pytorch3d.loss`` and the C ABI's refusals."""
from __future__ import annotations

import importlib
import sys

import numpy as np
import pytest
import torch

import meshloss_cases as cases
from autovfx_amd import hook, meshloss
from autovfx_amd.meshloss import mesh_normal_consistency_backward_host, mesh_normal_consistency_host, plan_host
from helpers import OnOtherGpu as _OnOtherGpu, fake_gpu as _gpu

F = np.float32


def _with_bad_faces(verts, faces, seed):
    """Faces with an index ``>= V`` or ``< 0`` spliced in among the valid ones; returns the mesh and the mask of the valid faces."""
    rng = np.random.default_rng(seed)
    V = len(verts)
    bad = faces[rng.integers(0, len(faces), 5)].copy()
    bad[0, 0], bad[1, 1], bad[2, 2], bad[3, 0], bad[4, 1] = V, -1, V + 7, -(2 ** 40), 2 ** 40
    at = np.sort(rng.integers(0, len(faces) + 1, len(bad)))
    mixed = np.insert(faces, at, bad, axis=0)
    valid = np.ones(len(mixed), bool)
    valid[at + np.arange(len(bad))] = False
    assert np.array_equal(mixed[valid], faces)
    return verts, mixed, valid


MESHES = {
    "torus": cases.torus(12, 9, seed=1),
    "torus_odd": cases.torus(31, 17, seed=2),
    "random": cases.random_mesh(40, 200, seed=3),
    "fan": cases.fan(50, seed=4),
    "grid": cases.grid(7, 5),
    "cube": cases.cube(),
    "tetrahedron": cases.tetrahedron(),
    "book": cases.book(7, seed=5),
    "strip": cases.strip(9, seed=6),
    "one_face": cases.random_mesh(3, 1, seed=7),
    "bad_indices": _with_bad_faces(*cases.torus(6, 5, seed=8), seed=9)[:2],
}


def _lexsort_plan(faces, V):
    """The plan said another way: ``numpy.lexsort`` on ``(lo, hi, id)`` and a count per position over the whole list."""
    n = 3 * len(faces)
    ids = np.arange(n)
    f, k = ids // 3, ids % 3
    valid = ((faces >= 0) & (faces < V)).all(1)[f]
    a, b = faces[f, (k + 1) % 3], faces[f, (k + 2) % 3]
    lo, hi = np.where(valid, np.minimum(a, b), V), np.where(valid, np.maximum(a, b), V)
    order = np.lexsort((ids, hi, lo))
    partners = np.array([0 if lo[i] == V else sum(1 for j in order[s + 1:] if lo[j] == lo[i] and hi[j] == hi[i]) for s, i in enumerate(order)],
                        np.int64).reshape(n)
    return order, partners


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(MESHES))
def test_plan_host_is_the_lexsort_plan(name):
    verts, faces = MESHES[name]
    order, partners, P = plan_host(faces, len(verts))
    want_order, want_partners = _lexsort_plan(faces, len(verts))
    assert order.dtype == np.int32 and partners.dtype == np.int32 and order.shape == partners.shape == (3 * len(faces),)
    assert np.array_equal(order, want_order) and np.array_equal(partners, want_partners) and P == int(want_partners.sum())
    if name != "bad_indices":
        c = cases.edge_counts(faces, len(verts))
        assert P == int((c * (c - 1) // 2).sum())


def test_the_plan_of_nothing():
    order, partners, P = plan_host(np.zeros((0, 3), np.int64), 5)
    assert order.shape == partners.shape == (0,) and P == 0
    order, partners, P = plan_host(np.array([[0, 1, 2]]), 0)              # no vertex: every index is out of range
    assert np.array_equal(order, [0, 1, 2]) and not partners.any() and P == 0


# ---- exact cases ------------------------------------------------------------------------------------------------------------------------

def _ulps(got, truth):
    return abs(float(got) - float(truth)) / float(np.spacing(F(abs(truth))))


def test_a_flat_grid_costs_nothing():
    verts, faces = cases.grid(7, 5)
    loss, terms = mesh_normal_consistency_host(verts, faces)
    assert loss.dtype == F and terms.dtype == F and terms.shape == (3 * len(faces),)
    print(f"flat grid: loss {float(loss):.3e}")
    assert 0 <= loss <= 2.0 ** -22


def test_a_cube_costs_two_thirds():
    """Twelve folds of 90 degrees among 18 edges; the coordinates are 0 and 1, so every term is exactly 0 or 1."""
    verts, faces = cases.cube()
    loss, terms = mesh_normal_consistency_host(verts, faces)
    truth, _ = cases.gradients_torch(verts, faces, 1.0, torch.float64)
    assert plan_host(faces, 8)[2] == 18 and sorted(terms[terms != 0].tolist()) == [1.0] * 12
    assert abs(float(truth) - 2 / 3) < 1e-15 and _ulps(loss, 2 / 3) <= 2


def test_an_open_strip_counts_its_interior_edges():
    verts, faces = cases.strip(9, seed=6)
    order, partners, P = plan_host(faces, len(verts))
    assert P == 8 and sorted(partners.tolist()) == [0] * 19 + [1] * 8
    loss, _ = mesh_normal_consistency_host(verts, faces)
    truth, _ = cases.gradients_torch(verts, faces, 1.0, torch.float64)
    assert abs(float(loss) - float(truth)) <= 2.0 ** -20


def test_one_face_and_two_faces():
    verts, faces = cases.random_mesh(3, 1, seed=7)
    loss, terms = mesh_normal_consistency_host(verts, faces)
    assert loss == 0 and not terms.any() and plan_host(faces, 3)[2] == 0
    grad, added, rows = mesh_normal_consistency_backward_host(verts, faces, 1.0)
    assert not grad.any() and len(added) == 0 and len(rows) == 0
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5]], F)
    faces = np.array([[0, 1, 2], [2, 1, 3]])
    order, partners, P = plan_host(faces, 4)
    assert P == 1 and partners.sum() == 1
    loss, terms = mesh_normal_consistency_host(verts, faces)
    truth, _ = cases.gradients_torch(verts, faces, 1.0, torch.float64)
    assert np.count_nonzero(terms) == 1 and loss == terms.sum() and _ulps(loss, truth) <= 4
    assert mesh_normal_consistency_host(np.zeros((0, 3), F), np.zeros((0, 3), np.int64))[0] == 0


# ---- the restatements against the float64 truth -------------------------------------------------------------------------------------------

TORI = [cases.torus(12, 9, seed=1), cases.torus(31, 17, seed=2), cases.torus(40, 23, seed=3, jitter=0.35)]


@pytest.mark.parametrize("index", range(len(TORI)))
def test_loss_restatement_against_truth(index):
    """The tree adds at most 146 < 256 times on any path and a lane at most ``c_max - 1`` times, on non-negative terms:
    ``(256 + c_max) 2^-24`` of the truth covers the sums and the division; what fp32 puts on the terms themselves is bounded from float64
    geometry by ``cases.term_error_bound``."""
    verts, faces = TORI[index]
    c_max = int(cases.edge_counts(faces, len(verts)).max())
    truth, _ = cases.gradients_torch(verts, faces, 1.0, torch.float64)
    loss, terms = mesh_normal_consistency_host(verts, faces)
    bound = (256 + c_max) * 2.0 ** -24 * float(truth) + cases.term_error_bound(verts, faces)
    err = abs(float(loss) - float(truth))
    print(f"torus {index}: c_max {c_max}, loss {float(loss):.8f}, truth {float(truth):.10f}, error {err:.3e}, bound {bound:.3e}")
    assert (terms >= -2.0 ** -22).all() and c_max == 2 and err <= bound       # (a flat pair's term may round to a few ulp of 1 below 0)


@pytest.mark.parametrize("index", range(len(TORI)))
def test_backward_restatement_against_truth(index):
    """The yardstick of tests/test_meshattrs.py, no bar fixed in advance: torch's own fp32 CPU autograd of pytorch3d's route, against the
    same float64 truth and in units of the sum of the absolute per-pair products (cases.normal_consistency_gradient_scale), is the
    measure; the restatement may be at most 4 x that.  No normal is near the clamp."""
    verts, faces = TORI[index]
    grad_loss = 0.37
    _, truth = cases.gradients_torch(verts, faces, grad_loss, torch.float64)
    _, torch32 = cases.gradients_torch(verts, faces, grad_loss, torch.float32)
    got, added, rows = mesh_normal_consistency_backward_host(verts, faces, grad_loss)
    P = plan_host(faces, len(verts))[2]
    assert got.dtype == F and got.shape == verts.shape and added.shape == (4 * P, 3) and rows.shape == (4 * P,)
    scale = cases.normal_consistency_gradient_scale(verts, faces, grad_loss)
    e_torch, e_ours = cases.relative_to(scale, torch32, truth), cases.relative_to(scale, got, truth)
    print(f"torus {index}: grad_verts, torch fp32 autograd {e_torch:.3e}, restatement {e_ours:.3e} of the scale")
    assert 0 < e_torch and e_ours <= 4 * e_torch
    again = np.zeros_like(got)
    np.add.at(again, rows, added)
    assert np.array_equal(again, got)


# ---- degenerate inputs --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [3, 5, 40])
def test_a_book_of_c_faces(c):
    verts, faces = cases.book(c, seed=c)
    order, partners, P = plan_host(faces, len(verts))
    assert P == c * (c - 1) // 2 and sorted(partners.tolist(), reverse=True)[:c] == list(range(c - 1, -1, -1))
    loss, terms = mesh_normal_consistency_host(verts, faces)
    truth, grad64 = cases.gradients_torch(verts, faces, 1.0, torch.float64)
    assert abs(float(loss) - float(truth)) <= (256 + c) * 2.0 ** -24 * float(truth) + cases.term_error_bound(verts, faces)
    _, grad32 = cases.gradients_torch(verts, faces, 1.0, torch.float32)
    got, _, _ = mesh_normal_consistency_backward_host(verts, faces, 1.0)
    scale = cases.normal_consistency_gradient_scale(verts, faces, 1.0)
    e_torch, e_ours = cases.relative_to(scale, grad32, grad64), cases.relative_to(scale, got, grad64)
    print(f"book of {c}: torch fp32 autograd {e_torch:.3e}, restatement {e_ours:.3e} of the scale")
    assert 0 < e_torch and e_ours <= 4 * e_torch


def test_a_duplicated_face():
    """The same three indices twice: every edge of the face has two incidences more, and the pair of the two copies costs 2 (their
    normals are equal, pytorch3d negates one)."""
    verts, faces = cases.torus(6, 5, seed=11)
    twice = np.concatenate((faces, faces[7:8]))
    P0, P1 = plan_host(faces, len(verts))[2], plan_host(twice, len(verts))[2]
    assert P1 == P0 + 3 * 2                                             # each of its edges goes from two incidences to three: 1 pair -> 3
    loss, terms = mesh_normal_consistency_host(verts, twice)
    truth, grad64 = cases.gradients_torch(verts, twice, 1.0, torch.float64)
    assert abs(float(loss) - float(truth)) <= (256 + 4) * 2.0 ** -24 * float(truth) + cases.term_error_bound(verts, twice)
    alone, alone_terms = mesh_normal_consistency_host(verts, np.concatenate((faces[7:8], faces[7:8])))       # the face and its copy only
    assert np.count_nonzero(alone_terms) == 3 and np.abs(alone_terms[alone_terms != 0] - 2).max() <= 2.0 ** -22 and abs(float(alone) - 2) <= 2.0 ** -22
    got, _, _ = mesh_normal_consistency_backward_host(verts, twice, 1.0)
    _, grad32 = cases.gradients_torch(verts, twice, 1.0, torch.float32)
    scale = cases.normal_consistency_gradient_scale(verts, twice, 1.0)
    assert cases.relative_to(scale, got, grad64) <= 4 * cases.relative_to(scale, grad32, grad64)


def test_a_face_that_repeats_an_index():
    """Its normal is exactly zero on every incidence, so its pairs cost exactly 1; it gets no gradient and gives none."""
    verts, faces = cases.torus(6, 5, seed=12)
    V = len(verts)
    verts = np.concatenate((verts, [[0.3, 0.2, 0.9], [0.1, 0.8, 0.7]])).astype(F)      # V, V + 1: only the degenerate faces use them
    a, b = int(faces[0, 0]), int(faces[0, 1])
    extra = np.array([[a, b, b], [a, V, V], [V + 1, V + 1, V + 1]])
    mixed = np.concatenate((faces[:9], extra, faces[9:]))
    order, partners, P = plan_host(mixed, len(verts))
    P0 = plan_host(faces, V)[2]
    loss, terms = mesh_normal_consistency_host(verts, mixed)
    loss0, terms0 = mesh_normal_consistency_host(verts[:V], faces)
    # edge (a, b): two more incidences beside the two faces' (2 * 2 pairs with them and one between themselves); (b, b) alone;
    # (a, V) twice, (V, V) once; (V + 1, V + 1) three times
    assert P == P0 + 5 + 1 + 3
    assert float(terms.astype(np.float64).sum() - terms0.astype(np.float64).sum()) == pytest.approx(9.0, abs=1e-5)
    own = np.isin(order // 3, (9, 10, 11))                             # the positions of the three faces' own incidences: every term is 1
    assert np.array_equal(terms[own], partners[own].astype(F)) and partners[own].sum() >= 5
    grad, added, rows = mesh_normal_consistency_backward_host(verts, mixed, 0.5)
    grad0, added0, rows0 = mesh_normal_consistency_backward_host(verts[:V], faces, 0.5 * P0 / P)
    assert not grad[V:].any() and not np.isin(rows, (V, V + 1)).any() and len(rows) == len(rows0) == 4 * P0
    scale = cases.normal_consistency_gradient_scale(verts[:V], faces, 0.5 * P0 / P)
    assert cases.relative_to(scale, grad[:V], grad0.astype(np.float64)) <= 4 * 2.0 ** -24     # (the same terms, scaled by another c)
    assert np.isfinite(grad).all() and np.isfinite(loss)


def test_faces_with_an_index_out_of_range_are_ignored():
    verts, faces = cases.torus(6, 5, seed=8)
    _, mixed, valid = _with_bad_faces(verts, faces, seed=9)
    order, partners, P = plan_host(mixed, len(verts))
    bad_ids = (3 * np.nonzero(~valid)[0][:, None] + np.arange(3)).reshape(-1)
    assert np.array_equal(order[-len(bad_ids):], bad_ids) and not partners[-len(bad_ids):].any()
    assert P == plan_host(faces, len(verts))[2]
    loss, terms = mesh_normal_consistency_host(verts, mixed)
    loss0, terms0 = mesh_normal_consistency_host(verts, faces)
    assert np.array_equal(terms[:-len(bad_ids)], terms0) and not terms[-len(bad_ids):].any() and abs(float(loss) - float(loss0)) <= 2.0 ** -22
    grad, added, rows = mesh_normal_consistency_backward_host(verts, mixed, 1.0)
    grad0, added0, rows0 = mesh_normal_consistency_backward_host(verts, faces, 1.0)
    assert np.array_equal(grad, grad0) and np.array_equal(added, added0) and np.array_equal(rows, rows0)
    # a neighbour of a face that becomes invalid loses that partner
    broken = faces.copy()
    broken[4, 2] = len(verts)
    assert plan_host(broken, len(verts))[2] == P - 3
    kept = np.delete(faces, 4, axis=0)
    assert mesh_normal_consistency_host(verts, broken)[0] == pytest.approx(float(cases.gradients_torch(verts, kept, 1.0, torch.float64)[0]), abs=1e-6)


def test_unreferenced_vertices_get_exactly_zero():
    verts, faces = cases.torus(6, 5, seed=13)
    more = np.concatenate((verts[:10], [[9, 9, 9]], verts[10:], [[np.nan, np.inf, -1]])).astype(F)
    moved = np.where(faces >= 10, faces + 1, faces)
    grad, _, rows = mesh_normal_consistency_backward_host(more, moved, 1.0)
    assert not grad[10].any() and not grad[-1].any() and np.isfinite(grad).all() and 10 not in rows
    assert np.array_equal(np.delete(grad, (10, len(more) - 1), axis=0), mesh_normal_consistency_backward_host(verts, faces, 1.0)[0])


def _clamped_formula_torch(verts, faces, grad_loss, dtype):
    """The contract's own formula in torch, ``1 + d / (clamp_min(|n_s|, eps) clamp_min(|n_t|, eps))`` over the truth's pair table, and its
    autograd: ``clamp_min`` passes no gradient at or below the bound."""
    v = torch.from_numpy(np.asarray(verts, F)).to(dtype).requires_grad_(True)
    edges_packed, edge_idx, vert_idx, _num, pairs = cases.topology_torch(torch.from_numpy(np.asarray(faces, np.int64)), v.shape[0])
    v0, v1 = v[edges_packed[edge_idx, 0]], v[edges_packed[edge_idx, 1]]
    n = sum(torch.cross(v1 - v0, v[vert_idx[:, i]] - v0, dim=1) for i in range(3))
    ns, nt = n[pairs[:, 0]], n[pairs[:, 1]]
    norm = lambda x: torch.sqrt((x * x).sum(1)).clamp_min(1e-8)
    loss = (1 + (ns * nt).sum(1) / (norm(ns) * norm(nt))).sum() / pairs.shape[0]
    (loss * grad_loss).backward()
    return loss.detach().numpy(), v.grad.numpy()


def test_normals_below_the_clamp_follow_it():
    """Edges of 1e-5: every normal is about 1e-10, far below 1e-8, and a term is ``1 + d / 1e-16``.  The loss is pytorch3d's.  The
    gradient is that of the contract's formula, with the norm's derivative off below the clamp; the installed torch's
    ``cosine_similarity`` clamps outside autograd and lets the norm's derivative through (about 1 % of these gradients), which the
    contract does not follow (difference 5)."""
    base, faces = cases.grid(3, 2)
    rng = np.random.default_rng(5)
    verts = ((base + 0.3 * rng.uniform(-1, 1, base.shape)) * 1e-5).astype(F)
    loss, terms = mesh_normal_consistency_host(verts, faces)
    truth, _ = cases.gradients_torch(verts, faces, 1.0, torch.float64)
    assert abs(float(loss) - float(truth)) <= 1e-6 and 0.99 < float(loss) < 1.01
    want_loss, want = _clamped_formula_torch(verts, faces, 1.0, torch.float64)
    assert abs(float(want_loss) - float(truth)) <= 1e-12
    got, _, _ = mesh_normal_consistency_backward_host(verts, faces, 1.0)
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
    # and above it the two agree: the same mesh a thousand times larger
    _, truth_big = cases.gradients_torch(verts * F(1e3), faces, 1.0, torch.float64)
    _, want_big = _clamped_formula_torch(verts * F(1e3), faces, 1.0, torch.float64)
    assert np.abs(truth_big - want_big).max() <= 1e-9 * np.abs(want_big).max()


def test_the_tree_sum_is_the_contracts():
    rng = np.random.default_rng(0)
    for count in (1, 255, 256, 257, 70000):
        t = rng.uniform(0, 2, count).astype(F)
        S = meshloss.tree_sum_host(t)
        exact = t.astype(np.float64).sum()
        assert S.dtype == F and abs(float(S) - exact) <= 146 * 2.0 ** -24 * exact
    assert meshloss.tree_sum_host(np.zeros(0, F)) == 0
    # 256 leaves, leaf i + 128 onto leaf i first: two halves of an ulp survive when they meet each other before they meet the 1
    t = np.zeros(256, F)
    t[0], t[1], t[129] = 1.0, 2.0 ** -24, 2.0 ** -24
    assert meshloss.tree_sum_host(t) == F(1.0) + F(2.0 ** -23)
    t[129], t[2] = 0.0, 2.0 ** -24
    assert meshloss.tree_sum_host(t) == F(1.0)


# ---- which calls the kernels take, and the drop-in -----------------------------------------------------------------------------------------

def test_direct_calls_say_why_not():
    verts, faces = _gpu(7, 3), _gpu(5, 3, dtype=torch.int64)
    assert meshloss._why_not(verts, faces) is None and meshloss._why_not(_gpu(3, 7).t(), _gpu(3, 5, dtype=torch.int64).t()) is None
    assert meshloss._why_not(_gpu(0, 3), _gpu(0, 3, dtype=torch.int64)) is None
    refused = (((torch.zeros(7, 3), faces), "GPU"), ((_gpu(7, 3, dtype=torch.float64), faces), "float32"), ((_gpu(7, 2), faces), r"\[V, 3\]"),
               ((_gpu(21), faces), r"\[V, 3\]"), ((verts, _gpu(5, 3, dtype=torch.int32)), "int64"), ((verts, _gpu(5, 4, dtype=torch.int64)), r"\[F, 3\]"),
               ((verts, torch.zeros(5, 3, dtype=torch.int64)), "faces must be on a GPU"), ((verts, _gpu(5, 3, dtype=torch.int64, cls=_OnOtherGpu)), "cuda:0"),
               ((np.zeros((7, 3), F), faces), "torch.Tensor"), ((verts, None), "torch.Tensor"))
    for args, word in refused:
        with pytest.raises(ValueError, match=word):
            meshloss.mesh_normal_consistency(*args)
        with pytest.raises(ValueError, match=word):
            meshloss.mesh_normal_consistency_terms(*args)
    good = meshloss.NormalConsistencyPlan(_gpu(15, dtype=torch.int32), _gpu(15, dtype=torch.int32), _gpu(1, dtype=torch.int64))
    assert meshloss._why_not(verts, faces, good) is None
    for bad in (good._replace(order=_gpu(12, dtype=torch.int32)), good._replace(partners=_gpu(15, dtype=torch.int64)),
                good._replace(pairs=torch.zeros(1, dtype=torch.int64)), good._replace(order=None)):
        with pytest.raises(ValueError, match="plan"):
            meshloss.mesh_normal_consistency(verts, faces, bad)
    for args, word in (((torch.zeros(5, 3, dtype=torch.int64), 7), "GPU"), ((_gpu(5, 3), 7), "int64"), ((faces, -1), "V"), ((faces, 1 << 31), "2\\^31"),
                       ((faces, 7.0), "V")):
        with pytest.raises(ValueError, match=word):
            meshloss.plan(*args)


def test_a_capturing_stream_is_not_taken(monkeypatch):
    from autovfx_amd import _lib
    verts, faces = _gpu(7, 3), _gpu(5, 3, dtype=torch.int64)
    monkeypatch.setattr(_lib, "capturing", lambda: True)
    with pytest.raises(ValueError, match="capturing"):
        meshloss.mesh_normal_consistency(verts, faces)
    with pytest.raises(ValueError, match="capturing"):
        meshloss.plan(faces, 7)
    calls = []
    ours = meshloss.drop_in(lambda meshes: calls.append(meshes) or "the original's result")
    meshes = cases.StubMeshes(verts, faces)
    assert ours(meshes) == "the original's result" and calls == [meshes]


def test_the_drop_in_hands_every_other_call_to_the_original():
    calls = []

    def original(*args, **kwargs):
        calls.append((args, kwargs))
        return "the original's result"

    ours = meshloss.drop_in(original)
    assert ours.__name__ == "mesh_normal_consistency" and ours.fallback is original
    verts, faces = _gpu(7, 3), _gpu(5, 3, dtype=torch.int64)
    assert meshloss._packed(cases.StubMeshes(verts, faces)) is not None              # the one shape that is taken
    others = (cases.StubMeshes(torch.zeros(7, 3), torch.zeros(5, 3, dtype=torch.int64)),                     # a CPU mesh
              cases.StubMeshes(verts, faces, count=2),                                                    # a batch
              cases.StubMeshes(_gpu(0, 3), _gpu(0, 3, dtype=torch.int64)),                                # an empty mesh
              cases.StubMeshes(verts, _gpu(0, 3, dtype=torch.int64)),
              cases.StubMeshes(_gpu(7, 3, dtype=torch.float64), faces),                                   # other dtypes
              cases.StubMeshes(_gpu(7, 3, dtype=torch.float16), faces),
              cases.StubMeshes(verts, _gpu(5, 3, dtype=torch.int32)),
              cases.StubMeshes(verts, _gpu(5, 3, dtype=torch.int64, cls=_OnOtherGpu)),
              object(), None, [verts], "meshes")                                                          # nothing like a Meshes
    for meshes in others:
        assert ours(meshes) == "the original's result"
        assert len(calls[-1][0]) == 1 and calls[-1][0][0] is meshes and calls[-1][1] == {}
    assert len(calls) == len(others)
    taken = cases.StubMeshes(verts, faces)
    assert ours(meshes=taken) == "the original's result" and calls[-1] == ((), {"meshes": taken})
    assert ours() == "the original's result" and ours(taken, taken) == "the original's result" and len(calls) == len(others) + 3


# ---- the hook ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def stub_pytorch3d(tmp_path):
    """A ``pytorch3d.loss`` package on disk whose ``__init__`` does the ``from``-import, and trainers that bind the function."""
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k.split(".")[0] == "pytorch3d" or k in cases.STUB_MODULES}
    cases.write_stub_package(tmp_path)
    path = list(sys.path)
    sys.path.insert(0, str(tmp_path))
    importlib.invalidate_caches()
    try:
        yield
    finally:
        hook.uninstall()
        sys.path[:] = path
        for k in list(sys.modules):
            if k.split(".")[0] == "pytorch3d" or k in cases.STUB_MODULES:
                sys.modules.pop(k)
        sys.modules.update(saved)
        importlib.invalidate_caches()


def _slots():
    """Every place the function is bound: the defining module, the package, the three trainers."""
    mods = {name: importlib.import_module(name) for name in cases.STUB_MODULES}
    return {"leaf": (mods["pytorch3d.loss.mesh_normal_consistency"], "mesh_normal_consistency"),
            "package": (mods["pytorch3d.loss"], "mesh_normal_consistency"),
            "refine": (mods["stub_trainer_refine"], "mesh_normal_consistency"),
            "coarse": (mods["stub_trainer_coarse"], "consistency"),
            "other": (mods["stub_trainer_other"], "mesh_normal_consistency")}


@pytest.mark.parametrize("imported", ["before", "after"])
def test_hook_binds_the_replacement_everywhere_and_uninstall_restores(stub_pytorch3d, imported):
    if imported == "before":
        slots = _slots()
        original = getattr(*slots["leaf"])
        assert all(getattr(*slot) is original for slot in slots.values())
        hook.install(path=False)
    else:
        hook.install(path=False)
        slots = _slots()
        original = slots["leaf"][0].reference_mesh_normal_consistency
    leaf = slots["leaf"][0]
    ours = leaf.mesh_normal_consistency
    assert ours is not original and ours.fallback is original and ours.__name__ == "mesh_normal_consistency"
    assert original.__module__ == "pytorch3d.loss.mesh_normal_consistency" and leaf.reference_mesh_normal_consistency is original
    assert all(getattr(*slot) is ours for slot in slots.values()), {k: getattr(*slot) for k, slot in slots.items()}
    assert hook.patched_modules.count("pytorch3d.loss.mesh_normal_consistency") == 1
    hook.install(path=False)                                                           # a second install changes nothing
    assert all(getattr(*slot) is ours for slot in slots.values()) and leaf.reference_mesh_normal_consistency is original
    # a CPU mesh reaches the original with the caller's argument, through a trainer's own name
    verts, faces = cases.tetrahedron()
    meshes = cases.StubMeshes(torch.from_numpy(verts), torch.from_numpy(faces))
    out = slots["refine"][0].mesh_normal_consistency(meshes)
    assert leaf.calls == [meshes] and float(out) == pytest.approx(4 / 3, abs=1e-6)
    hook.uninstall()
    assert all(getattr(*slot) is original for slot in slots.values()) and not hasattr(leaf, "reference_mesh_normal_consistency")
    assert hook.patched_modules == []


def test_a_module_of_that_name_without_the_function_is_left_alone(stub_pytorch3d, tmp_path):
    (tmp_path / "elsewhere").mkdir()
    (tmp_path / "elsewhere" / "__init__.py").write_text("")
    (tmp_path / "elsewhere" / "mesh_normal_consistency.py").write_text("threshold = 3\n")
    importlib.invalidate_caches()
    hook.install(path=False)
    try:
        mod = importlib.import_module("elsewhere.mesh_normal_consistency")
        assert mod.threshold == 3 and not hasattr(mod, "reference_mesh_normal_consistency") and mod.__name__ not in hook.patched_modules
    finally:
        sys.modules.pop("elsewhere.mesh_normal_consistency", None)
        sys.modules.pop("elsewhere", None)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------

def test_cabi_refusals_need_no_device():
    from autovfx_amd import _lib
    L = _lib.lib
    assert L.gsr_abi_version() == 20 == _lib.ABI_VERSION
    a, b, c, d, e, f, g, h = ((1 << 20) * i for i in range(1, 9))      # never read: every call is refused
    F_max = ((1 << 30) - 1) // 3                                       # the most faces: 3 F = 2^30 - 1
    assert 3 * (F_max + 1) >= 1 << 30 > 3 * F_max

    def refused(name, args, word):
        rc = getattr(L, name)(*args, None)
        return rc == -1 and word in _lib.last_error() and name in _lib.last_error()

    plan_bytes, fwd_bytes = L.gsr_normal_consistency_plan_scratch_bytes(50), L.gsr_normal_consistency_scratch_bytes(50)
    assert plan_bytes >= 5 * 4 * 150 and fwd_bytes == 4
    assert L.gsr_normal_consistency_scratch_bytes(86) == 8 and L.gsr_normal_consistency_scratch_bytes(0) == 0
    for query in (L.gsr_normal_consistency_plan_scratch_bytes, L.gsr_normal_consistency_scratch_bytes):
        assert query(-1) == 0 and query(F_max + 1) == 0 and query(1 << 62) == 0 and query(F_max) > 0
    table = {
        # V F faces order partners pairs scratch scratch_bytes
        "gsr_normal_consistency_plan": ([100, 50, a, b, c, d, e, plan_bytes], [
            (0, -1, "negative"), (1, -1, "negative"), (1, F_max + 1, "2^30"), (1, 1 << 40, "2^30"), (0, 1 << 31, "2^31"),
            (2, None, "null"), (3, None, "null"), (4, None, "null"), (5, None, "null"), (6, None, "null"),
            (2, a + 4, "aligned"), (3, b + 2, "aligned"), (4, c + 1, "aligned"), (5, d + 4, "aligned"), (6, e + 128, "aligned"),
            (7, plan_bytes - 1, "scratch too small"), (7, 0, "scratch too small")]),
        # V F verts faces order partners pairs loss terms_or_null scratch scratch_bytes
        "gsr_normal_consistency_forward": ([100, 50, a, b, c, d, e, f, g, h, fwd_bytes], [
            (0, -1, "negative"), (1, -1, "negative"), (1, F_max + 1, "2^30"), (0, 1 << 31, "2^31"),
            (2, None, "null"), (3, None, "null"), (4, None, "null"), (5, None, "null"), (6, None, "null"), (7, None, "null"), (9, None, "null"),
            (2, a + 2, "aligned"), (3, b + 4, "aligned"), (4, c + 2, "aligned"), (5, d + 1, "aligned"), (6, e + 4, "aligned"),
            (7, f + 3, "aligned"), (8, g + 2, "aligned"), (9, h + 1, "aligned"), (10, fwd_bytes - 1, "scratch too small")]),
        # V F verts faces order partners pairs grad_loss grad_verts
        "gsr_normal_consistency_backward": ([100, 50, a, b, c, d, e, f, g], [
            (0, -1, "negative"), (1, -1, "negative"), (1, F_max + 1, "2^30"), (0, 1 << 31, "2^31"),
            (2, None, "null"), (3, None, "null"), (4, None, "null"), (5, None, "null"), (6, None, "null"), (7, None, "null"), (8, None, "null"),
            (2, a + 2, "aligned"), (3, b + 4, "aligned"), (4, c + 2, "aligned"), (5, d + 1, "aligned"), (6, e + 4, "aligned"),
            (7, f + 3, "aligned"), (8, g + 2, "aligned")]),
    }
    for name, (ok, cases_) in table.items():
        for at, value, word in cases_:
            args = list(ok)
            args[at] = value
            assert refused(name, args, word), (name, at, value, _lib.last_error())
    # nothing to do without a vertex: the backward returns before any launch
    assert L.gsr_normal_consistency_backward(0, 0, None, None, None, None, None, None, None, None) == 0
