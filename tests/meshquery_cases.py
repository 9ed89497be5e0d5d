"""Meshes and queries shared by the closest-triangle tests (tests/test_meshquery.py, tests/test_meshquery_gpu.py,
tests/test_meshquery_deep_gpu.py)."""
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


def plane_in_random_order(nx: int, ny: int, seed: int = 0):
    """``grid_plane(nx, ny)`` (integer coordinates: every tie is exact) with its faces in a random order."""
    verts, faces = grid_plane(nx, ny, 1.0)
    return verts, np.ascontiguousarray(faces[np.random.default_rng(seed).permutation(faces.shape[0])])


def sphere_with_invalid(valid: int, invalid: int, seed: int = 0):
    """``valid + invalid`` faces of a cube sphere of which ``invalid``, scattered through the face order, are invalid: the first half
    of them by an index outside ``[0, V)``, the rest by a corner with a non-finite coordinate (vertices appended for that, which no
    other face names).  Returns ``verts``, ``faces`` and the ascending indices of the invalid faces."""
    verts, faces = sphere_with_faces(valid + invalid, seed)
    faces = faces.copy()
    g = np.random.default_rng(seed + 1)
    bad = g.permutation(faces.shape[0])[:invalid]
    half = invalid // 2
    extra = np.full((invalid - half, 3), 0.5, F32)
    extra[np.arange(invalid - half), g.integers(0, 3, invalid - half)] = np.resize(np.array([np.nan, np.inf, -np.inf], F32), invalid - half)
    V = verts.shape[0] + extra.shape[0]
    faces[bad[:half], g.integers(0, 3, half)] = np.resize(np.array([V, -1, 1 << 40, V + 7, -(1 << 33)], np.int64), half)
    faces[bad[half:], g.integers(0, 3, invalid - half)] = verts.shape[0] + np.arange(invalid - half)
    return np.concatenate((verts, extra)), faces, np.sort(bad)


def sphere_with_spanners(F: int = 20000, spanners: int = 50, slivers: int = 200, seed: int = 0):
    """``F`` faces of a cube sphere, ``spanners`` triangles whose corners lie near corners of the sphere's bounding box (each as wide
    as the mesh) and ``slivers`` nearly collinear triangles about one radius long, all in a random order."""
    verts, faces = sphere_with_faces(F, seed)
    g = np.random.default_rng(seed + 2)
    lo, hi = verts.min(axis=0).astype(np.float64), verts.max(axis=0).astype(np.float64)
    at = g.integers(0, 2, (spanners, 3, 3))
    at[:, 1] = 1 - at[:, 0]                                          # two corners diagonally opposite: the whole bounds
    wide = lo + (hi - lo) * (at + g.uniform(-0.02, 0.02, at.shape))
    a = g.uniform(lo, hi, (slivers, 3))
    along = g.normal(size=(slivers, 3))
    along /= np.linalg.norm(along, axis=1, keepdims=True)
    thin = np.stack((a, a + along, a + 0.5 * along + 1e-6 * g.normal(size=(slivers, 3))), 1)
    more = np.concatenate((wide, thin)).reshape(-1, 3).astype(F32)
    faces = np.concatenate((faces, (np.arange(more.shape[0]).reshape(-1, 3) + verts.shape[0]).astype(np.int64)))
    return np.concatenate((verts, more)), np.ascontiguousarray(faces[g.permutation(faces.shape[0])])


def sphere_with_overflowing_centroid(F: int, seed: int = 0):
    """``F`` faces of a cube sphere of which one (face 5, or the only one) has three finite corners near (3e38, -3e38, 1): a valid
    face whose centroid sum overflows, so the bounds of the centroids hold +inf in x and -inf in y."""
    verts, faces = sphere_with_faces(F, seed)
    faces = faces.copy()
    huge = np.array([[3.0e38, -3.0e38, 1.0], [3.1e38, -3.1e38, 1.5], [3.2e38, -2.9e38, 0.5]], F32)
    faces[min(5, F - 1)] = verts.shape[0] + np.arange(3)
    return np.concatenate((verts, huge)), faces


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
