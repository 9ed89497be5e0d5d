"""Meshes, rays and an independent float64 truth shared by the first-hit tests (tests/test_meshrays.py, tests/test_meshrays_gpu.py)."""
from __future__ import annotations

import numpy as np

import meshquery_cases as cases

F32 = np.float32


def icosphere(sub: int):
    """The unit icosphere after ``sub`` subdivisions: 20 * 4^sub faces that share their vertices (a closed, watertight mesh)."""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1),
         (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, float) / np.linalg.norm(p) for p in v]
    for _ in range(sub):
        cache, nf = {}, []

        def mid(i, j):
            k = (min(i, j), max(i, j))
            if k not in cache:
                m = v[i] + v[j]
                v.append(m / np.linalg.norm(m))
                cache[k] = len(v) - 1
            return cache[k]

        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v, F32), np.array(f, np.int64)


def edges(faces):
    return np.unique(np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), 1), axis=0)


def rays_through_features(verts, faces, origin, extra: int = 500, seed: int = 0):
    """Rays from ``origin`` through every vertex, every edge midpoint and every face centroid, plus ``extra`` random directions."""
    g = np.random.default_rng(seed)
    e = edges(faces)
    targets = np.concatenate([verts, ((verts[e[:, 0]] + verts[e[:, 1]]) * F32(0.5)).astype(F32), verts[faces].mean(1).astype(F32)])
    origin = np.asarray(origin, F32)
    d = np.concatenate([(targets - origin).astype(F32), g.normal(size=(extra, 3)).astype(F32)])
    return np.ascontiguousarray(np.broadcast_to(origin, d.shape)), d


def truth64(o, d, verts, faces):
    """The first hit in float64 by Moeller and Trumbore's test, written independently of the contract: ``face [n]`` (-1: none),
    ``t [n]`` and ``margin [n]``, the smallest barycentric coordinate of the hit (how far inside the face it lies)."""
    o, d, v = np.asarray(o, np.float64), np.asarray(d, np.float64), verts.astype(np.float64)
    a, b, c = (v[faces[:, k]] for k in range(3))
    e1, e2 = b - a, c - a
    face, tt, margin = np.full(len(o), -1, np.int64), np.full(len(o), np.inf), np.zeros(len(o))
    for i in range(len(o)):
        p = np.cross(d[i], e2)
        det = (e1 * p).sum(1)
        ok = np.abs(det) > 1e-300
        den = np.where(ok, det, 1.0)
        s = o[i] - a
        u = (s * p).sum(1) / den
        q = np.cross(s, e1)
        w = (q * d[i]).sum(1) / den
        t = (e2 * q).sum(1) / den
        t = np.where(ok & (u >= 0) & (w >= 0) & (u + w <= 1) & (t >= 0), t, np.inf)
        j = int(np.argmin(t))
        if np.isfinite(t[j]):
            face[i], tt[i], margin[i] = j, t[j], min(u[j], w[j], 1 - u[j] - w[j])
    return face, tt, margin


def rippled_sphere(F: int, seed: int = 0, depth: float = 0.15, centre=(0.3, -0.2, 0.5)):
    """``cases.sphere_with_faces(F)`` with its radius rippled by ``depth``: a ray from inside can cross several folds, so the first
    hit is not the only one."""
    verts, faces = cases.sphere_with_faces(F, seed, 1.0, centre)
    p = verts.astype(np.float64) - np.asarray(centre)
    r = 1.0 + depth * np.sin(9.0 * p[:, 0]) * np.cos(7.0 * p[:, 1] + 1.0) * np.sin(8.0 * p[:, 2] + 0.5)
    return (p * r[:, None] + np.asarray(centre)).astype(F32), faces


def mixed_rays(verts, n: int, seed: int = 0):
    """``n`` rays against a mesh around its vertices' mean: a third from points inside (0.3 of the mesh's reach), a third from
    outside aimed at the mesh (most hit, some graze past), a third from outside aimed anywhere (most miss); unnormalised."""
    g = np.random.default_rng(seed)
    mean = verts.astype(np.float64).mean(0)
    reach = np.abs(verts.astype(np.float64) - mean).max()
    kind = np.arange(n) % 3
    unit = g.normal(size=(n, 3))
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    o = mean + unit * np.where(kind == 0, 0.3 * reach * g.uniform(0, 1, n), reach * g.uniform(2.0, 4.0, n))[:, None]
    aim = mean + g.normal(size=(n, 3)) * 0.6 * reach
    d = np.where((kind == 2)[:, None], g.normal(size=(n, 3)), aim - o) * g.uniform(0.2, 3.0, n)[:, None]
    return o.astype(F32), d.astype(F32)


def cube():
    """The unit cube, 12 faces: every face's own box has zero thickness on one axis."""
    v = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], F32)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 7, 5], [4, 6, 7], [0, 5, 1], [0, 4, 5], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7],
                  [1, 7, 3]], np.int64)
    return v, f
