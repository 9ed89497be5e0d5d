"""Meshes, rays and an independent float64 truth shared by the first-hit tests (tests/test_meshrays.py, tests/test_meshrays_gpu.py)."""
from __future__ import annotations

import functools
import itertools
from types import SimpleNamespace

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


# ---- the branches of the contract, one family of rays each ("Branch families") -----------------------------------------
# Every builder is cached and returns a SimpleNamespace of read-only arrays: ``o``, ``d``, ``verts``, ``faces`` and what the family's
# own expectations need, and has an ``expect_...`` beside it: what the contract's restatement must answer, asserted on a result of
# meshquery.first_hits_host.  tests/test_meshrays.py holds the restatement to those expectations (and its pruned form to brute force),
# tests/test_meshrays_gpu.py the kernel to the restatement, bit for bit.
OFF = np.asarray((0.3, -0.2, 0.5), F32)


def _case(**fields):
    for x in fields.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return SimpleNamespace(**fields)


def closed_faces_at(verts, faces, x, y):
    """The faces of a z = 0 mesh whose closed triangle holds (x, y): orientation tests, exact on halves of integers."""
    t = verts.astype(np.float64)[faces][:, :, :2]
    p = np.array([x, y], np.float64)
    side = lambda u, v: (v[:, 0] - u[:, 0]) * (p[1] - u[:, 1]) - (v[:, 1] - u[:, 1]) * (p[0] - u[:, 0])
    s = np.stack([side(t[:, 0], t[:, 1]), side(t[:, 1], t[:, 2]), side(t[:, 2], t[:, 0])], 1)
    return np.nonzero((s >= 0).all(1) | (s <= 0).all(1))[0]


def shear_directions():
    """Every sign pattern of (1,1,0), (1,0,1), (0,1,1), (1,1,1) (|d| ties at the maximum), of (2,1,1), (1,2,1), (1,1,2) (a strict
    maximum, a tie below it) and of the three axes; each direction with a zero also with -0.0 in its place; all of them also scaled
    by 0.25 and by 3 (Sz != +-1).  float32 ``[204, 3]``: every component is exact, so every tie is."""
    out = []
    for base in ((1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1), (2, 1, 1), (1, 2, 1), (1, 1, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
        axes = [k for k in range(3) if base[k]]
        for signs in itertools.product((1.0, -1.0), repeat=len(axes)):
            v = [0.0, 0.0, 0.0]
            for k, s in zip(axes, signs):
                v[k] = s * base[k]
            out.append(v)
            if len(axes) < 3:
                out.append([x if x else -0.0 for x in v])
    d = np.array(out, F32)
    return np.concatenate((d, d * F32(0.25), d * F32(3)))


def shear_ties(d):
    """How many rows of ``d`` tie in |d| at the maximum: on x and y alone, x and z, y and z, and on all three."""
    m = np.abs(d)
    top = m.max(1, keepdims=True)
    at = m == top
    return {"xy": int((at[:, 0] & at[:, 1] & ~at[:, 2]).sum()), "xz": int((at[:, 0] & ~at[:, 1] & at[:, 2]).sum()),
            "yz": int((~at[:, 0] & at[:, 1] & at[:, 2]).sum()), "xyz": int(at.all(1).sum())}


@functools.lru_cache(maxsize=None)
def shears(mesh: str, per: int = 3, seed: int = 21):
    """``per`` rays in each of ``shear_directions`` against the cube or the 320-face icosphere, shifted off the origin; every origin
    is a random point inside the mesh minus 3 d, so most rays hit."""
    verts, faces = cube() if mesh == "cube" else icosphere(2)
    verts = (verts + OFF).astype(F32)
    d = np.repeat(shear_directions(), per, axis=0)
    g = np.random.default_rng(seed)
    centre = OFF.astype(np.float64) + (0.5 if mesh == "cube" else 0.0)
    o = (centre + g.uniform(-0.4, 0.4, d.shape) - 3.0 * d).astype(F32)
    return _case(o=o, d=d, verts=verts, faces=faces)


@functools.lru_cache(maxsize=None)
def axis_parallel():
    """The unit cube and rays along +-x, +-y, +-z from the grid {0, 0.25, 0.5, 1}^2 on the two other axes (the cube's corners, edges
    and face interiors: o_k == lo_k == hi_k occurs where d_k == 0): from outside toward the cube (t = 0.75), from outside away from
    it (a miss) and from inside (t = 0.5), the zero components once as 0.0 and once as -0.0.  ``axis``, ``t`` (+inf: a miss) and
    ``near`` (the coordinate on ``axis`` of the side that is hit, -1: none) are per ray."""
    verts, faces = cube()
    grid = (0.0, 0.25, 0.5, 1.0)
    o, d, axis_of, t, near = [], [], [], [], []
    for axis, u, v, zero in itertools.product(range(3), grid, grid, (0.0, -0.0)):
        for start, step, want_t, want_near in ((-1.5, 2.0, 0.75, 0), (2.5, -2.0, 0.75, 1), (-1.5, -2.0, np.inf, -1), (2.5, 2.0, np.inf, -1),
                                               (0.5, -1.0, 0.5, 0), (0.5, 1.0, 0.5, 1)):
            oo, dd = [0.0, 0.0, 0.0], [zero, zero, zero]
            oo[axis], oo[(axis + 1) % 3], oo[(axis + 2) % 3], dd[axis] = start, u, v, step
            o.append(oo), d.append(dd), axis_of.append(axis), t.append(want_t), near.append(want_near)
    return _case(o=np.array(o, F32), d=np.array(d, F32), verts=verts, faces=faces, axis=np.array(axis_of), t=np.array(t, F32),
                 near=np.array(near))


@functools.lru_cache(maxsize=None)
def oblique_onto_cube(distance: float, n: int = 512, seed: int = 21):
    """``n`` rays aimed at random points inside the unit cube from ``distance`` away in random directions, unnormalised: every hit
    face has a flat box, so the interval [t_enter, t_exit] that t is clamped into is two to four ulp wide.  About one hit in six has a
    t_tri below t_enter; one above t_exit is rare (one batch of 512 in 170 has one), and the seed is one with which one of the three
    distances the tests use has it.  Both are conditions on the inputs, asserted in ``expect_oblique_onto_cube``."""
    verts, faces = cube()
    g = np.random.default_rng(seed + int(distance))
    p = g.uniform(0.05, 0.95, (n, 3))
    unit = g.normal(size=(n, 3))
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    o = (p - distance * unit).astype(F32)
    d = ((p - o.astype(np.float64)) * g.uniform(0.2, 3.0, n)[:, None]).astype(F32)
    return _case(o=o, d=d, verts=verts, faces=faces)


@functools.lru_cache(maxsize=None)
def surface_origins():
    """Origins exactly on the six sides of the unit cube, with directions pointing inward, outward and along the side (a ray in a
    face's plane: det == 0 for that side's two faces), and three faces of zero area on valid indices: ``degenerate`` (two equal
    corners spanning the cube's diagonal, so every ray that meets the cube enters its box; three collinear corners on a line
    parallel to x; three equal corners).  ``side_axis``, ``side_at`` (0 or 1) and ``kind`` (0 inward, 1 outward, 2 along) are per
    ray; ``normal`` marks the inward and outward rays whose largest component is the side's normal, for which t_tri is an exact
    zero."""
    verts, faces = cube()
    verts = np.concatenate((verts, np.array([(0.25, 0.5, 0.5), (0.5, 0.5, 0.5), (0.75, 0.5, 0.5)], F32)))
    degenerate = np.array([len(faces), len(faces) + 1, len(faces) + 2])
    faces = np.concatenate((faces, np.array([(0, 7, 7), (8, 9, 10), (9, 9, 9)], np.int64)))
    spots = ((0.25, 0.5), (0.5, 0.25), (0.5, 0.5), (0.75, 0.125), (0.0, 0.5), (1.0, 1.0))    # inside a face, on the diagonal, an edge, a corner
    along = ((1.0, 0.0), (0.0, -1.0), (1.0, 1.0), (0.25, -0.75), (-2.0, 0.5))
    tilt = ((0.0, 0.0), (0.25, -0.5), (-0.75, 0.25), (1.5, 0.5), (-0.5, -3.0))              # the last two: the largest component is not the normal
    o, d, side_axis, side_at, kind, normal = [], [], [], [], [], []
    for axis, at, (u, v) in itertools.product(range(3), (0.0, 1.0), spots):
        oo = [0.0, 0.0, 0.0]
        oo[axis], oo[(axis + 1) % 3], oo[(axis + 2) % 3] = at, u, v
        inward = 1.0 if at == 0.0 else -1.0
        for k, (p, q), scale in [(0, pq, s) for pq in tilt for s in (1.0, 0.5)] + [(1, pq, s) for pq in tilt for s in (1.0, 3.0)] + \
                                [(2, pq, 1.0) for pq in along]:
            dd = [0.0, 0.0, 0.0]
            dd[axis], dd[(axis + 1) % 3], dd[(axis + 2) % 3] = (0.0 if k == 2 else inward if k == 0 else -inward) * scale, p * scale, q * scale
            o.append(list(oo)), d.append(dd), side_axis.append(axis), side_at.append(at), kind.append(k)
            normal.append(k < 2 and max(abs(p), abs(q)) < 1.0)
    return _case(o=np.array(o, F32), d=np.array(d, F32), verts=verts, faces=faces, degenerate=degenerate, side_axis=np.array(side_axis),
                 side_at=np.array(side_at, F32), kind=np.array(kind), normal=np.array(normal))


TINY = (1e-39, 1e-42, -1e-45, 3e-39, -2.9e-39, 5e-39, 1.1e-38, -1.2e-38)    # 1 / x overflows below 2^-128 = 2.94e-39; all but the last are denormal


@functools.lru_cache(maxsize=None)
def denormal_rays():
    """The unit cube and rays with denormal or overflowing components.
      * along +-x, +-y, +-z from two units away, one or both other components of d in ``TINY``, the origin on the grid {0, 0.25, 1}^2
        of the other axes -- at 0 and 1 it coincides with a box face on a denormal axis: (lo - o) * inv is 0 * inf, a NaN;
      * every component denormal: (1e-40, 1e-41, 1e-39) (Sz overflows: a miss) and (5e-39, -4e-39, 1.1e-38) (a finite, huge t), in all
        sign patterns, from inside and outside;
      * |d| ~ 1e-30: t finite and huge.
    ``huge`` is the same cube and axis rays with every coordinate times 1e38 (``o``, ``verts``; ``d`` as it is or times 1e38): the
    determinants overflow, the answer is a miss."""
    verts, faces = cube()
    o, d = [], []
    grid = (0.0, 0.25, 1.0)
    for axis, (start, step), tiny, (u, v), which in itertools.product(range(3), ((2.0, -1.0), (-1.0, 1.0)), TINY, itertools.product(grid, grid),
                                                                      range(3)):
        oo, dd = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
        oo[axis], oo[(axis + 1) % 3], oo[(axis + 2) % 3], dd[axis] = start, u, v, step
        if which != 1:
            dd[(axis + 1) % 3] = tiny
        if which != 0:
            dd[(axis + 2) % 3] = -tiny if which == 2 else tiny
        o.append(oo), d.append(dd)
    for base, signs, start in itertools.product(((1e-40, 1e-41, 1e-39), (5e-39, -4e-39, 1.1e-38), (1.1e-38, 1e-42, -3e-39)),
                                                itertools.product((1.0, -1.0), repeat=3), ((0.25, 0.5, 0.5), (0.5, 0.25, 2.0), (-1.0, 0.0, 1.0),
                                                                                            (0.0, 0.0, 0.0))):
        o.append(list(start)), d.append([s * x for s, x in zip(signs, base)])
    for dd in ((0.0, 0.0, -1e-30), (3e-31, -2e-31, -1e-30), (1e-30, 1e-42, 0.0)):
        for start in ((0.25, 0.5, 2.0), (0.0, 1.0, 2.0), (-1.0, 0.5, 0.5)):
            o.append(list(start)), d.append(list(dd))
    o, d = np.array(o, F32), np.array(d, F32)
    flat = axis_parallel()
    big = F32(1e38)
    huge_o = np.concatenate((flat.o * big, flat.o * big, o[:200] * big))
    huge_d = np.concatenate((flat.d, flat.d * big, d[:200]))
    return _case(o=o, d=d, verts=verts, faces=faces, huge=_case(o=huge_o, d=huge_d, verts=verts * big, faces=faces))


@functools.lru_cache(maxsize=None)
def comb(F: int, seed: int = 41):
    """``F`` flat triangles, one in each plane x = i with corners (i,-1,-1), (i,1,-1), (i,0,1), the faces shuffled: face j lies in the
    plane ``perm[j]``.  Five kinds of ray, 64 of each:
      0  grazing: along +-x at (y, z) = (+-0.9, 0.9), inside every face's box and outside every triangle -- a miss that prunes nothing;
      1  from x = -2 along +x through every triangle: the first is the plane 0;   2  from x = F + 1 along -x: the plane F - 1;
      3  from between two planes, along +-x;
      4  oblique, +-(1, a, b): through (k, 0, 0) of a random plane k after passing the planes k -+ 1 and k -+ 2 outside their triangles.
    Laid out as one wave per kind, then the same 320 rays shuffled (every wave mixed), then one more wave of grazing rays.  All
    coordinates are small integers or short binary fractions but the grazing 0.9, so every ``t`` is exact: ``t`` and ``plane`` (-1: a
    miss) are what is expected per ray."""
    g = np.random.default_rng(seed)
    perm = g.permutation(F)
    x = perm.astype(np.float64)[:, None]
    verts = np.stack((np.repeat(x, 3, 1), np.tile((-1.0, 1.0, 0.0), (F, 1)), np.tile((-1.0, -1.0, 1.0), (F, 1))), -1).reshape(-1, 3)
    faces = np.arange(3 * F, dtype=np.int64).reshape(F, 3)
    inside = ((0.0, 0.0), (0.25, -0.5), (-0.25, -0.5), (0.0, 0.5))         # (y, z) inside the triangle
    slopes = ((0.75, 0.0), (-0.75, 0.25), (0.25, -0.875))                  # (a, b): (-a, -b) and (-2a, -2b) lie outside it
    speeds = (1.0, 2.0, 0.5, 4.0)
    o, d, t, plane = [], [], [], []
    for kind, i in itertools.product(range(5), range(64)):
        s, (y, z), fwd = speeds[i % 4], inside[(i // 4) % 4], i % 2 == 0
        if kind == 0:
            o.append((-2.0 if fwd else F + 1.0, 0.9 if i % 4 < 2 else -0.9, 0.9)), d.append((s if fwd else -s, 0.0, 0.0))
            t.append(np.inf), plane.append(-1)
        elif kind == 1:
            o.append((-2.0, y, z)), d.append((s, 0.0, 0.0)), t.append(2.0 / s), plane.append(0)
        elif kind == 2:
            o.append((F + 1.0, y, z)), d.append((-s, 0.0, 0.0)), t.append(2.0 / s), plane.append(F - 1)
        elif kind == 3:
            m = int(g.integers(0, F - 1))
            o.append((m + 0.5, y, z)), d.append((s if fwd else -s, 0.0, 0.0)), t.append(0.5 / s), plane.append(m + 1 if fwd else m)
        else:
            k, (a, b), sign = int(g.integers(3, F - 3)), slopes[i % 3], 1.0 if fwd else -1.0
            o.append((k - 2.5 * sign, -2.5 * a, -2.5 * b)), d.append((sign * s, a * s, b * s)), t.append(2.5 / s), plane.append(k)
    mix = g.permutation(320)
    layout = np.concatenate((np.arange(320), mix, np.arange(64)))
    o, d, t, plane = (np.array(a)[layout] for a in (o, d, t, plane))
    kind = (np.arange(320) // 64)[layout]
    return _case(o=o.astype(F32), d=d.astype(F32), verts=verts.astype(F32), faces=faces, perm=perm, t=t.astype(F32), plane=plane, kind=kind)


@functools.lru_cache(maxsize=None)
def copies(dup: int = 28, seed: int = 51):
    """The 320-face icosphere with its face ``dup`` appended 300 more times and the 620 faces shuffled: ``same`` are the indices of the
    301 copies, which the plan keeps side by side (one Morton code) in five leaves or more.  200 rays aimed at random points of that
    face with barycentrics >= 0.05: the first 100 from inside the sphere, the others from outside."""
    verts, faces = icosphere(2)
    g = np.random.default_rng(seed)
    perm = g.permutation(620)
    source = np.concatenate((np.arange(320), np.full(300, dup)))[perm]
    same = np.nonzero(source == dup)[0]
    w = 0.05 + 0.85 * g.dirichlet((1.0, 1.0, 1.0), 200)
    corners = verts[faces[dup]].astype(np.float64)
    p = w @ corners
    unit = g.normal(size=(200, 3))
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    outward = np.where((unit * p).sum(1, keepdims=True) < 0, -unit, unit)
    start = np.where((np.arange(200) < 100)[:, None], 0.5 * unit * g.uniform(0, 1, (200, 1)), p + 2.0 * (outward + 0.5 * p))
    o = start.astype(F32)
    d = ((p - o.astype(np.float64)) * g.uniform(0.2, 3.0, (200, 1))).astype(F32)
    return _case(o=o, d=d, verts=verts, faces=np.ascontiguousarray(faces[source]), same=same)


def leaf_entries(case):
    """Where the plan puts the faces and when each ray enters each leaf: ``leaf_of [F]`` (the leaf of every face) and ``t_enter
    [n, leaves]`` (+inf where the ray misses the leaf's box), from meshquery.plan_host and slab_host."""
    from autovfx_amd import meshquery

    order, _, levels = meshquery.plan_host(case.verts, case.faces)
    leaf_of = np.empty(len(order), np.int64)
    leaf_of[order] = np.arange(len(order)) // meshquery.LEAF
    lo, hi = levels[0]
    with np.errstate(all="ignore"):
        t_enter, t_exit = meshquery.slab_host(tuple(lo[None, :, k] for k in range(3)), tuple(hi[None, :, k] for k in range(3)),
                                              tuple(case.o[:, k][:, None] for k in range(3)), tuple(case.d[:, k][:, None] for k in range(3)))
    return leaf_of, np.where(t_enter <= t_exit, t_enter, F32(np.inf))


PLANE_DIRECTIONS = ((1, 1, -1), (-1, 1, -1), (1, 0, -1), (0, -1, -1), (2, 2, -2), (1, -1, 1))    # the last from below


@functools.lru_cache(maxsize=None)
def plane_vertex_rays(nx: int, ny: int, seed: int):
    """``cases.plane_in_random_order`` (z = 0, integer coordinates) and, for every direction of ``PLANE_DIRECTIONS``, a ray through
    every vertex from v - 2 d: t == 2 exactly, and up to six faces in several leaves tie.  ``lowest`` is the lowest index among the
    faces whose closed triangle holds the vertex."""
    verts, faces = cases.plane_in_random_order(nx, ny, seed)
    at = np.array([(i, j, 0) for i in range(nx + 1) for j in range(ny + 1)], np.float64)
    lowest = np.array([closed_faces_at(verts, faces, x, y).min() for x, y, _ in at])
    d = np.repeat(np.array(PLANE_DIRECTIONS, np.float64), len(at), axis=0)
    o = np.tile(at, (len(PLANE_DIRECTIONS), 1)) - 2.0 * d
    return _case(o=o.astype(F32), d=d.astype(F32), verts=verts, faces=faces, lowest=np.tile(lowest, len(PLANE_DIRECTIONS)))


def rays_that_answer_nothing(o, d):
    """``o``, ``d`` with six more rays, copies of the first six spoiled: a NaN and an infinity in the origin, a NaN and an infinity in
    the direction, a zero direction and one with a -0."""
    bad_o, bad_d = o[:6].copy(), d[:6].copy()
    bad_o[0, 1], bad_o[1, 0], bad_d[2, 2], bad_d[3, 0], bad_d[4], bad_d[5] = np.nan, np.inf, np.nan, -np.inf, 0.0, (0.0, -0.0, 0.0)
    return np.concatenate((o, bad_o)), np.concatenate((d, bad_d))


@functools.lru_cache(maxsize=None)
def four_levels(F: int = 262145):
    """A rippled sphere whose plan has four levels of boxes (4097 leaves, then 257, 17 and 2), one more than 16385 faces have: 192
    mixed rays and the six that answer nothing."""
    verts, faces = rippled_sphere(F, seed=7)
    o, d = rays_that_answer_nothing(*mixed_rays(verts, 192, seed=8))
    return _case(o=o, d=d, verts=verts, faces=faces)


# ---- what the restatement must answer on each family ---------------------------------------------------------------------------------
def expect_shears(case, face, t, bary):
    d = case.d
    kz = np.argmax(np.abs(d), axis=1)          # numpy's argmax ties to the first axis, as the contract's kz ties to the lowest
    seen = {(int(k), bool(s)) for k, s in zip(kz, d[np.arange(len(d)), kz] < 0)}
    ties = shear_ties(d)
    print(f"shears: {len(d)} rays, {int((face >= 0).sum())} hit, (kz, d[kz] < 0) seen: {sorted(seen)}, ties at the maximum: {ties}")
    assert seen == {(k, s) for k in range(3) for s in (False, True)}
    assert min(ties.values()) >= 1
    assert any(np.signbit(x) and x == 0 for x in d.ravel())
    # every ray passes through a point inside a closed mesh: the watertight test lets none through
    assert (face >= 0).all() and np.isfinite(t).all() and not np.signbit(t).any()


def expect_axis_parallel(case, face, t, bary):
    assert np.array_equal(face >= 0, case.near >= 0)
    assert np.array_equal(t, case.t)                                   # 0.75 from outside, 0.5 from inside, +inf pointing away
    hit = face >= 0
    side = case.verts[case.faces[face[hit]]][np.arange(int(hit.sum())), :, case.axis[hit]]       # [hits, 3 corners] on the ray's axis
    assert (side == case.near[hit][:, None]).all()                    # the near side
    on_a_box_face = ((case.o == 0) | (case.o == 1)) & (case.d == 0)
    assert on_a_box_face.any(1).sum() >= 100 and np.signbit(case.d[case.d == 0]).any()


def expect_oblique_onto_cube(case, face, t, bary):
    """Returns how many hits have an active clamp, how many of them sit at t_enter and how many at t_exit."""
    from autovfx_amd import meshquery

    hit = face >= 0
    got = meshquery.ray_triangle_host(case.o[hit], case.d[hit], *(case.verts[case.faces[face[hit], k]] for k in range(3)))
    assert got["hit"].all() and np.array_equal(got["t"], t[hit])
    active = got["t"] != got["t_tri"]
    enter, leave = int((active & (got["t"] == got["t_enter"])).sum()), int((active & (got["t"] == got["t_exit"])).sum())
    want, _, margin = truth64(case.o, case.d, case.verts, case.faces)
    safe = margin > 1e-4
    print(f"oblique: {int(hit.sum())} of {len(hit)} rays hit, the clamp is active on {int(active.sum())} ({enter} at t_enter, {leave} at "
          f"t_exit), {int(safe.sum())} rays with a margin above 1e-4")
    assert 20 * int(active.sum()) >= int(hit.sum()) > 0 and enter + leave == int(active.sum())
    assert 10 * int(safe.sum()) >= 9 * len(hit) and np.array_equal(face[safe], want[safe])
    return int(active.sum()), enter, leave


def expect_surface_origins(case, face, t, bary):
    from autovfx_amd import meshquery

    assert not np.signbit(t).any() and not np.isin(face, case.degenerate).any()
    in_side = np.zeros(len(face), bool)                               # the answered face lies in the side the origin is on
    hit = face >= 0
    rows = np.nonzero(hit)[0]
    in_side[rows] = (case.verts[case.faces[face[rows]]][np.arange(len(rows)), :, case.side_axis[rows]] == case.side_at[rows][:, None]).all(1)
    normal = case.normal
    assert normal.sum() >= 400 and (face[normal] >= 0).all() and (t[normal] == 0).all()
    off_the_edges = ((case.o > 0) & (case.o < 1)).sum(1) == 2         # (on an edge a perpendicular side holds the origin too)
    assert (normal & off_the_edges).sum() >= 250 and in_side[normal & off_the_edges].all()
    along = case.kind == 2
    assert (hit & along).sum() >= 100 and not in_side[along].any()    # det == 0: a miss for that side, a hit on a perpendicular one
    entered = []
    for f in case.degenerate:
        with np.errstate(all="ignore"):
            got = meshquery.ray_triangle_host(case.o, case.d, *(case.verts[case.faces[f, k]][None] for k in range(3)))
        assert not got["hit"].any()
        entered.append(int((got["t_enter"] <= got["t_exit"]).sum()))
    print(f"surface: {len(face)} rays, {int(hit.sum())} hit, {int((t == 0).sum())} at t == +0, the zero-area faces' boxes are entered by "
          f"{entered} rays")
    assert min(entered) >= 1                                          # ray_triangle is reached for each of them


def expect_denormal_rays(case, face, t, bary):
    with np.errstate(all="ignore"):
        inv = F32(1) / case.d
    overflowed = (np.isinf(inv) & (case.d != 0)).any(1)
    tiny = ((case.d != 0) & (np.abs(case.d) < np.finfo(F32).tiny)).any(1)
    hit = face >= 0
    print(f"denormal: {len(face)} rays, {int(tiny.sum())} with a denormal component, {int(overflowed.sum())} with an infinite 1 / d_k "
          f"({int((hit & overflowed).sum())} of them hit), {int(hit.sum())} hits in all, the largest finite t {t[np.isfinite(t)].max():.3g}")
    assert hit.any() and (~hit).any() and overflowed.any() and (hit & overflowed).any() and (~hit & overflowed).any()
    assert (tiny & ~overflowed & hit).any()                          # a denormal component whose reciprocal is finite
    assert t[np.isfinite(t)].max() > 1e29 and not np.signbit(t).any()
    assert np.array_equal(hit, np.isfinite(t))


def expect_all_miss(case, face, t, bary):
    assert (face == -1).all() and np.isposinf(t).all() and (bary == 0).all()


def expect_comb(case, face, t, bary):
    assert np.array_equal(t, case.t)
    assert np.array_equal(np.where(face >= 0, case.perm[face], -1), case.plane)
    waves = case.kind[:len(case.kind) // 64 * 64].reshape(-1, 64)
    pure, mixed = (waves == waves[:, :1]).all(1), np.array([len(set(w)) == 5 for w in waves])
    assert (pure & (waves[:, 0] == 0)).sum() == 2 and pure.sum() == 6 and mixed.sum() == 5      # ... a whole wave that grazes, in both layouts


def expect_copies(case, face, t, bary):
    lowest = int(case.same.min())
    assert len(case.same) == 301 and (face == lowest).all()
    leaf_of, t_enter = leaf_entries(case)
    leaves, own = np.unique(leaf_of[case.same]), int(leaf_of[lowest])
    # the kernel's root pushes the leaves by the wave minimum of t_enter, nearest on top: in these waves a leaf with higher copies is
    # popped before the leaf of the lowest one, whose record then has to replace an equal t with a higher index
    early = [(at // 64, int(j)) for at in range(0, len(face), 64) for j in leaves
             if j != own and t_enter[at:at + 64, j].min() < t_enter[at:at + 64, own].min()]
    print(f"copies: the 301 copies lie in the leaves {leaves.tolist()}, the lowest ({lowest}) in leaf {own}; (wave, leaf) entered before it: {early}")
    assert len(leaves) >= 5 and own != 0 and np.isfinite(t_enter[:, leaves]).all() and len(early) >= 1


def expect_plane_vertex_rays(case, face, t, bary):
    assert (face >= 0).all() and (t == 2).all()
    assert np.array_equal(face, case.lowest)


def expect_four_levels(case, face, t, bary):
    from autovfx_amd import meshquery

    layout = meshquery.plan_layout(len(case.faces))
    assert layout.counts == (4097, 257, 17, 2) and layout.top == meshquery.plan_layout(16385).top + 1 == 3
    hits = int((face[:-6] >= 0).sum())
    print(f"four levels: {hits} of {len(face) - 6} rays hit")
    assert (face[-6:] == -1).all() and 64 <= hits < len(face) - 6
