"""Meshes and queries shared by the closest-triangle tests (tests/test_meshquery.py, tests/test_meshquery_gpu.py)."""
from __future__ import annotations

import numpy as np

F32 = np.float32


def grid_plane(nx: int, ny: int, e: float = 1.0, origin=(0.0, 0.0, 0.0)):
    """A planar grid of nx x ny cells of edge ``e`` in z = origin.z, two triangles per cell: ``verts [V, 3]`` float32, ``faces [F, 3]`` int64."""
    xs, ys = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="ij")
    verts = np.stack((xs.ravel() * e, ys.ravel() * e, np.zeros(xs.size)), -1) + np.asarray(origin)
    at = lambda i, j: i * (ny + 1) + j
    faces = []
    for i in range(nx):
        for j in range(ny):
            faces.append((at(i, j), at(i + 1, j), at(i + 1, j + 1)))
            faces.append((at(i, j), at(i + 1, j + 1), at(i, j + 1)))
    return verts.astype(F32), np.asarray(faces, np.int64).reshape(-1, 3)


def cube_sphere(n: int, radius: float = 1.0, centre=(0.0, 0.0, 0.0)):
    """A sphere from the six faces of a cube, n x n cells each, pushed onto the sphere: 12 n^2 nearly even triangles (the faces
    do not share vertices along the cube's edges: a closest-point query does not care)."""
    verts, faces = [], []
    t = np.linspace(-1.0, 1.0, n + 1)
    u, v = np.meshgrid(t, t, indexing="ij")
    one = np.ones_like(u)
    for axis in range(3):
        for sign in (-1.0, 1.0):
            cols = [None, None, None]
            cols[axis], cols[(axis + 1) % 3], cols[(axis + 2) % 3] = sign * one, u, v
            p = np.stack(cols, -1).reshape(-1, 3)
            base = sum(len(x) for x in verts)
            verts.append(p / np.linalg.norm(p, axis=1, keepdims=True))
            at = lambda i, j: base + i * (n + 1) + j
            for i in range(n):
                for j in range(n):
                    faces.append((at(i, j), at(i + 1, j), at(i + 1, j + 1)))
                    faces.append((at(i, j), at(i + 1, j + 1), at(i, j + 1)))
    verts = np.concatenate(verts) * radius + np.asarray(centre)
    return verts.astype(F32), np.asarray(faces, np.int64).reshape(-1, 3)


def sphere_with_faces(F: int, seed: int = 0, radius: float = 1.0, centre=(0.3, -0.2, 0.5)):
    """Exactly ``F`` faces of a cube sphere (the smallest that has them, a random subset in a random order)."""
    n = 1
    while 12 * n * n < F:
        n += 1
    verts, faces = cube_sphere(n, radius, centre)
    keep = np.random.default_rng(seed).permutation(faces.shape[0])[:F]
    return verts, np.ascontiguousarray(faces[keep])


def edge_lengths(verts, faces):
    t = verts.astype(np.float64)[faces]
    return np.concatenate([np.linalg.norm(t[:, k] - t[:, (k + 1) % 3], axis=1) for k in range(3)])


def queries_near(verts, faces, n: int, reach: float, seed: int = 1):
    """``n`` float32 points at random places on random faces, pushed off by up to ``reach`` in a random direction."""
    g = np.random.default_rng(seed)
    t = verts.astype(np.float64)[faces[g.integers(0, faces.shape[0], n)]]
    w = g.dirichlet((1.0, 1.0, 1.0), n)
    on = (t * w[:, :, None]).sum(1)
    step = g.normal(size=(n, 3))
    step *= (g.uniform(0.0, reach, n) / np.linalg.norm(step, axis=1))[:, None]
    return (on + step).astype(F32)


def truth_distances(points, verts, faces):
    """float64 distances ``[n, F]`` from every point to every triangle, written independently of the contract: the projection onto
    the triangle's plane where it falls inside (barycentric test), else the nearest of the three edges (clamped projection)."""
    p = points.astype(np.float64)[:, None, :]
    t = verts.astype(np.float64)[faces]
    a, b, c = t[None, :, 0], t[None, :, 1], t[None, :, 2]

    def segment(u, v):
        uv = v - u
        ll = (uv * uv).sum(-1)
        s = np.where(ll > 0, ((p - u) * uv).sum(-1) / np.where(ll > 0, ll, 1.0), 0.0)
        s = np.clip(s, 0.0, 1.0)
        return np.linalg.norm(p - (u + s[..., None] * uv), axis=-1)

    best = np.minimum(np.minimum(segment(a, b), segment(b, c)), segment(c, a))
    ab, ac = b - a, c - a
    nrm = np.cross(ab, ac)
    nn = (nrm * nrm).sum(-1)
    ok = nn > 0
    safe = np.where(ok, nn, 1.0)
    ap = p - a
    # barycentric coordinates of the projection
    w_c = (np.cross(ab, ap) * nrm).sum(-1) / safe
    w_b = (np.cross(ap, ac) * nrm).sum(-1) / safe
    inside = ok & (w_b >= 0) & (w_c >= 0) & (w_b + w_c <= 1)
    plane = np.abs((ap * nrm).sum(-1)) / np.sqrt(safe)
    return np.where(inside, np.minimum(plane, best), best)
