"""The closest triangle of a mesh to every query point, on the GPU: what Open3D's ``RaycastingScene.compute_closest_points``
answers for the melting frames of the frame loop (``scene_representation.py:385-412``) and for object extraction
(``extract/extract_object.py:105-110``).

The contract, pointwise.  A face is *valid* when its three indices lie in ``[0, V)`` and its nine
coordinates are finite.  The answer for query ``q`` is the valid face with the smallest ``(d(q, f), f)`` -- equal distances go to
the lower face index -- where, all in fp32 elementwise operations (no fused multiply-add), with ``dot(u, v) = (ux vx + uy vy) + uz vz``:

* ``A = a - q``, ``B = b - q``, ``C = c - q``; ``ab = B - A``, ``ac = C - A``; ``d1 = dot(ab, -A)``, ``d2 = dot(ac, -A)``,
  ``d3 = dot(ab, -B)``, ``d4 = dot(ac, -B)``, ``d5 = dot(ab, -C)``, ``d6 = dot(ac, -C)``; ``vc = d1 d4 - d3 d2``, ``vb = d5 d2 - d1 d6``,
  ``va = d3 d6 - d5 d4``; ``e = d4 - d3``, ``g = d5 - d6``;
* ``p'`` is the first of (Ericson's regions): ``A`` if ``d1 <= 0 and d2 <= 0``; ``B`` if ``d3 >= 0 and d4 <= d3``;
  ``A + (d1 / (d1 - d3)) ab`` if ``vc <= 0 and d1 >= 0 and d3 <= 0``; ``C`` if ``d6 >= 0 and d5 <= d6``;
  ``A + (d2 / (d2 - d6)) ac`` if ``vb <= 0 and d2 >= 0 and d6 <= 0``; ``B + (e / (e + g)) (C - B)`` if ``va <= 0 and e >= 0 and g >= 0``;
  else ``(A + (vb / s) ab) + (vc / s) ac`` with ``s = (va + vb) + vc``.  A quotient whose denominator is zero is 0: the region's first
  end point, so a degenerate triangle gives a finite answer;
* ``d_tri = dot(p', p')``; ``d_box`` = the squared gap between ``q`` and the triangle's own box, per axis
  ``max(max(lo - q, q - hi), 0)``, summed like ``dot``; ``d_vtx = min(min(dot(A, A), dot(B, B)), dot(C, C))``;
* ``d = fmin(fmax(d_tri, d_box), d_vtx)`` (a NaN ``d_tri``, from an overflow, is ignored); the closest point is ``q + p'``.

The true distance lies in ``[d_box, d_vtx]``, so the clamps only remove rounding error; and the bound of any tree box that contains
the triangle never exceeds ``d_box``, so the tree search of ``gsr_meshquery.hip`` finds exactly the brute-force answer, index ties
included.  A non-finite query, and any query when no face is valid, gets ``(-1, +inf, (0, 0, 0))``.

:func:`closest_triangles` runs the HIP kernels (C ABI ``gsr_closest_tri_plan`` / ``gsr_closest_tri_query``);
:func:`closest_triangles_host` restates the contract in numpy by brute force, the checker of the tests, :func:`plan_host` and
:func:`plan_layout` restate the build and the layout of the plan; :class:`Scene` is a small
adapter for code written against Open3D's ray-casting scene.  ``autovfx_amd.install()`` does not put it over Open3D: the frame loop
uses it when ``AUTOVFX_AMD_MELT_CLOSEST=gpu`` (``autovfx_amd/frame_loop.py``).

The same plan answers the other geometric question of the reference's own code, the first triangle a ray hits, which it asks of
trimesh on the host (``extract/extract_object.py:115-159``, ``:424-434``, ``:476-482``, ``:563-606``; only ever the first hit).

The ray contract, pointwise.  ``origins`` and ``dirs`` are fp32 and ``dirs`` are not normalised.  The answer
for a ray ``(o, d)`` is the valid face with the smallest ``(t, f)`` among the faces it hits -- equal ``t`` go to the lower face index.
A ray with a non-finite component or a zero direction, a ray that hits nothing, and any ray when no face is valid, gets
``(-1, +inf, (0, 0, 0))``.  All in fp32 elementwise operations in the order written (no fused multiply-add), ``fmin`` / ``fmax``
dropping a NaN:

* the triangle test is the watertight one of Woop, Benthin and Wald without its double-precision fallback: ``kz`` = the axis of the
  largest ``|d|`` (ties: the lowest axis), ``kx``, ``ky`` the next two cyclically, swapped when ``d[kz] < 0``; ``Sx = d[kx] / d[kz]``,
  ``Sy = d[ky] / d[kz]``, ``Sz = 1 / d[kz]``; ``A = a - o`` (``B``, ``C`` alike); ``Ax = A[kx] - Sx A[kz]``, ``Ay = A[ky] - Sy A[kz]``,
  ``Az = Sz A[kz]``; ``U = Cx By - Cy Bx``, ``V = Ax Cy - Ay Cx``, ``W = Bx Ay - By Ax``; a miss when one of them is ``< 0`` and
  another ``> 0`` (two-sided); ``det = (U + V) + W``, a miss when 0; ``t_tri = ((U Az + V Bz) + W Cz) / det``, a miss unless
  ``t_tri >= 0``; the barycentrics are ``U / det``, ``V / det``, ``W / det``, the weights of ``a``, ``b``, ``c``;
* the triangle's own box is tested by slabs: on an axis with ``d_k != 0`` the products ``(lo_k - o_k) (1 / d_k)`` and
  ``(hi_k - o_k) (1 / d_k)`` ordered by the sign of ``1 / d_k``, on an axis with ``d_k == 0`` all of the line when
  ``lo_k <= o_k <= hi_k`` and nothing otherwise; ``t_enter = fmax(fmax(fmax(0, near_x), near_y), near_z)``,
  ``t_exit = fmin(fmin(far_x, far_y), far_z) * 1.00000024f`` (the padding of Ize, "Robust BVH Ray Traversal");
* a face is hit iff the triangle test hits, ``t_enter <= t_exit`` and ``t < +inf``, with
  ``t = fmin(fmax(t_tri, t_enter), t_exit) + 0`` (the ``+ 0`` turns a ``-0`` into ``+0``).

The clamp moves ``t`` by rounding error only, and it makes a box search exact: any box that contains the triangle's box has a
``t_enter`` that is not larger and a ``t_exit`` that is not smaller, so skipping a box that is missed, or entered strictly after the
best ``t`` so far, never skips the answer or a tie with it.

:func:`first_hits` runs the HIP kernel (C ABI ``gsr_ray_first_hit``); :func:`first_hits_host` restates the contract in numpy;
:meth:`Scene.cast_rays` and :class:`RayIntersector` are small adapters for code written against Open3D's scene and trimesh's
``mesh.ray``; ``autovfx_amd.extract.triangle_votes`` is the voting loop of object extraction on top.  ``autovfx_amd.install()`` puts
none of them over trimesh or Open3D, whose choices at ties and at grazing rays are not known here.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _takes

MAX_FACES = (1 << 30) - 1
MAX_VERTS = (1 << 31) - 1
MAX_QUERIES = (1 << 31) - 1
_F = np.float32


# ---- the contract in numpy ----------------------------------------------------------------------------------------------------------
def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _sub(u, v):
    return (u[0] - v[0], u[1] - v[1], u[2] - v[2])


def _neg(u):
    return (-u[0], -u[1], -u[2])


def _along(u, s, v):
    return (u[0] + s * v[0], u[1] + s * v[1], u[2] + s * v[2])


def _guarded(num, den):
    ok = den != 0
    return np.where(ok, num / np.where(ok, den, _F(1)), _F(0))


def _box_bound(lo, hi, q):
    """gsr_tree.h's ``box_bound`` on per-axis tuples: the squared gap between ``q`` and the box, summed like ``dot``."""
    gaps = [np.fmax(np.fmax(lo[k] - q[k], q[k] - hi[k]), _F(0)) for k in range(3)]
    return (gaps[0] * gaps[0] + gaps[1] * gaps[1]) + gaps[2] * gaps[2]


def triangle_distance_host(q, a, b, c):
    """``d(q, f)`` of the contract for float32 arrays ``q``, ``a``, ``b``, ``c`` of shape ``[..., 3]`` that broadcast against each
    other.  Returns a dict of float32 arrays: ``d``, ``d_tri``, ``d_box``, ``d_vtx`` (shape ``[...]``) and ``p`` (``[..., 3]``, the point
    ``d_tri`` used, relative to the query).  Overflow and NaN pass through as in the kernel."""
    q, a, b, c = (np.asarray(t, dtype=_F) for t in (q, a, b, c))
    xyz = lambda t: (t[..., 0], t[..., 1], t[..., 2])
    qv, av, bv, cv = xyz(q), xyz(a), xyz(b), xyz(c)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        A, B, C = _sub(av, qv), _sub(bv, qv), _sub(cv, qv)
        ab, ac = _sub(B, A), _sub(C, A)
        ap, bp, cp = _neg(A), _neg(B), _neg(C)
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        e, g = d4 - d3, d5 - d6
        den = (va + vb) + vc
        regions = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                   (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e >= 0) & (g >= 0)]
        points = [A, B, _along(A, _guarded(d1, d1 - d3), ab), C, _along(A, _guarded(d2, d2 - d6), ac),
                  _along(B, _guarded(e, e + g), _sub(C, B))]
        inside = _along(_along(A, _guarded(vb, den), ab), _guarded(vc, den), ac)
        shape = np.broadcast(d1).shape
        p = tuple(np.select(regions, [np.broadcast_to(pt[k], shape) for pt in points], default=inside[k]).astype(_F, copy=False)
                  for k in range(3))
        d_tri = _dot(p, p)
        d_vtx = np.fmin(np.fmin(_dot(A, A), _dot(B, B)), _dot(C, C))
        lo = tuple(np.fmin(np.fmin(av[k], bv[k]), cv[k]) for k in range(3))
        hi = tuple(np.fmax(np.fmax(av[k], bv[k]), cv[k]) for k in range(3))
        d_box = _box_bound(lo, hi, qv)
        d = np.fmin(np.fmax(d_tri, d_box), d_vtx)
    return {"d": d, "d_tri": d_tri, "d_box": d_box, "d_vtx": d_vtx, "p": np.stack(p, -1)}


def valid_faces_host(verts: np.ndarray, faces: np.ndarray) -> np.ndarray:
    """The contract's validity, ``[F]`` bool: three indices in ``[0, V)``, nine finite coordinates."""
    V = verts.shape[0]
    ok = np.all((faces >= 0) & (faces < V), axis=1)
    fine = np.all(np.isfinite(verts), axis=1)
    ok[ok] = np.all(fine[faces[ok]], axis=1)
    return ok


def _closest_pruned(pts, rows, v, f, ids, chunk_elems, face_idx, sq_dist, closest):
    """``closest_triangles_host(..., pruned=True)`` for the finite queries ``rows`` and the valid faces ``ids`` (ascending)."""
    a, b, c = (v[f[ids, k]] for k in range(3))
    lo = tuple(np.fmin(np.fmin(a[:, k], b[:, k]), c[:, k])[None, :] for k in range(3))
    hi = tuple(np.fmax(np.fmax(a[:, k], b[:, k]), c[:, k])[None, :] for k in range(3))
    corners = v[np.unique(f[ids])]          # min over the faces of d_vtx = min over their corners of dot(A, A): the same values, once each
    step = max(1, chunk_elems // ids.size)
    with np.errstate(over="ignore", invalid="ignore"):
        for at in range(0, rows.size, step):
            r = rows[at:at + step]
            q = pts[r]
            qv = tuple(q[:, k][:, None] for k in range(3))
            A = tuple(corners[:, k][None, :] - qv[k] for k in range(3))
            u = np.min(_dot(A, A), axis=1)                          # (never NaN: a difference of finite numbers is none)
            row, col = np.nonzero(_box_bound(lo, hi, qv) <= u[:, None])     # row-major: per query, ascending face index
            starts = np.searchsorted(row, np.arange(r.size))
            assert np.all(np.diff(np.append(starts, row.size)) > 0)         # the winner itself has d_box <= d <= u
            got = triangle_distance_host(q[row], a[col], b[col], c[col])
            least = np.minimum.reduceat(got["d"], starts)
            first = np.nonzero(got["d"] == least[row])[0]
            first = first[np.unique(row[first], return_index=True)[1]]      # the first minimum of every query
            face_idx[r] = ids[col[first]]
            sq_dist[r] = got["d"][first]
            closest[r] = q + got["p"][first]


def closest_triangles_host(points, verts, faces, chunk_elems: int = 1 << 20, pruned: bool = False):
    """The contract restated in numpy: brute force over all valid faces, every operation an fp32 elementwise one in the contract's
    order, chunked over the queries.  ``points``, ``verts``: anything ``np.asarray`` takes, reshaped to ``[., 3]`` float32; ``faces``
    to ``[F, 3]`` int64.  Returns ``face_idx [n]`` int64, ``sq_dist [n]`` float32, ``closest [n, 3]`` float32.

    ``pruned``: the same answers, bit for bit and ties included, in a fraction of the time on a large mesh (185 queries around a
    sphere of 262145 faces: 0.9 s against 9 s), which is what makes meshes of 2^18 faces testable.  Per query ``u`` = the smallest ``d_vtx`` of any valid face, and ``d`` is evaluated only on the faces with
    ``d_box <= u``, the first minimum in ascending face index taken.  The contract's clamp gives ``d_box <= d <= d_vtx`` in the
    computed fp32 values, so the brute force's winner has ``d <= u``, hence ``d_box <= u``, and so has every face that ties with it.
    No tree and no order of the faces is involved: it shares nothing with the kernels' search but the contract."""
    pts = np.ascontiguousarray(np.asarray(points, dtype=_F).reshape(-1, 3))
    v = np.ascontiguousarray(np.asarray(verts, dtype=_F).reshape(-1, 3))
    f = np.ascontiguousarray(np.asarray(faces, dtype=np.int64).reshape(-1, 3))
    n = pts.shape[0]
    face_idx = np.full(n, -1, np.int64)
    sq_dist = np.full(n, np.inf, _F)
    closest = np.zeros((n, 3), _F)
    ids = np.nonzero(valid_faces_host(v, f))[0]                 # ascending: the first minimum of a row is the lowest face index
    rows = np.nonzero(np.all(np.isfinite(pts), axis=1))[0]
    if ids.size == 0 or rows.size == 0:
        return face_idx, sq_dist, closest
    if pruned:
        _closest_pruned(pts, rows, v, f, ids, chunk_elems, face_idx, sq_dist, closest)
        return face_idx, sq_dist, closest
    a, b, c = (v[f[ids, k]][None, :, :] for k in range(3))
    step = max(1, chunk_elems // ids.size)
    for at in range(0, rows.size, step):
        r = rows[at:at + step]
        q = pts[r]
        got = triangle_distance_host(q[:, None, :], a, b, c)
        best = np.argmin(got["d"], axis=1)                      # (d is never NaN: fmin / fmax drop one, d_box and d_vtx have none)
        pick = np.arange(r.size)
        face_idx[r] = ids[best]
        sq_dist[r] = got["d"][pick, best]
        with np.errstate(over="ignore", invalid="ignore"):
            closest[r] = q + got["p"][pick, best]
    return face_idx, sq_dist, closest


# ---- the ray contract in numpy --------------------------------------------------------------------------------------------------------
SLAB_PAD = _F(1.00000024)     # gsr_meshquery.hip's kSlabPad: 1 + 2^-22


def _pick(v, k):
    """Component ``k`` (an int array) of the per-axis tuple ``v``: gsr_meshquery.hip's ``pick``."""
    return np.where(k == 0, v[0], np.where(k == 1, v[1], v[2]))


def _ray_shear(d):
    """``kx, ky, kz, Sx, Sy, Sz`` of the per-axis tuple ``d`` (finite, not all zero): ``make_ray``."""
    mag = tuple(np.abs(x) for x in d)
    second = mag[1] > mag[0]
    kz = np.where(mag[2] > np.where(second, mag[1], mag[0]), 2, np.where(second, 1, 0))
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    dkz = _pick(d, kz)
    kx, ky = np.where(dkz < 0, ky, kx), np.where(dkz < 0, kx, ky)
    return kx, ky, kz, _pick(d, kx) / dkz, _pick(d, ky) / dkz, _F(1) / dkz


def slab_host(lo, hi, o, d):
    """``t_enter``, ``t_exit`` of the contract for per-axis tuples of float32 arrays that broadcast: gsr_meshquery.hip's ``slab``.  The
    box is hit iff ``t_enter <= t_exit``."""
    inf = _F(np.inf)
    near, far = [], []
    for k in range(3):
        moving = d[k] != 0
        inv = _F(1) / np.where(moving, d[k], _F(1))
        first, second = (lo[k] - o[k]) * inv, (hi[k] - o[k]) * inv
        inside = (lo[k] <= o[k]) & (o[k] <= hi[k])
        near.append(np.where(moving, np.where(inv < 0, second, first), np.where(inside, -inf, inf)))
        far.append(np.where(moving, np.where(inv < 0, first, second), np.where(inside, inf, -inf)))
    t_enter = np.fmax(np.fmax(np.fmax(_F(0), near[0]), near[1]), near[2])
    t_exit = np.fmin(np.fmin(far[0], far[1]), far[2]) * SLAB_PAD
    return t_enter, t_exit


def ray_triangle_host(o, d, a, b, c):
    """``t(ray, f)`` of the ray contract for float32 arrays ``o``, ``d``, ``a``, ``b``, ``c`` of shape ``[..., 3]`` that broadcast
    against each other; the rays finite with a direction that is not zero, the corners finite.  Returns a dict of arrays of shape
    ``[...]``: ``hit`` (bool), ``t`` (float32, meaningful where ``hit``), ``t_tri``, ``t_enter``, ``t_exit``, and ``bary``
    ``[..., 3]`` (``U / det``, ``V / det``, ``W / det``).  Overflow and NaN pass through as in the kernel."""
    o, d, a, b, c = (np.asarray(t, dtype=_F) for t in (o, d, a, b, c))
    xyz = lambda t: (t[..., 0], t[..., 1], t[..., 2])
    ov, dv, av, bv, cv = xyz(o), xyz(d), xyz(a), xyz(b), xyz(c)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        kx, ky, kz, Sx, Sy, Sz = _ray_shear(dv)
        A, B, C = _sub(av, ov), _sub(bv, ov), _sub(cv, ov)
        Akz, Bkz, Ckz = _pick(A, kz), _pick(B, kz), _pick(C, kz)
        Ax, Ay = _pick(A, kx) - Sx * Akz, _pick(A, ky) - Sy * Akz
        Bx, By = _pick(B, kx) - Sx * Bkz, _pick(B, ky) - Sy * Bkz
        Cx, Cy = _pick(C, kx) - Sx * Ckz, _pick(C, ky) - Sy * Ckz
        U, V, W = Cx * By - Cy * Bx, Ax * Cy - Ay * Cx, Bx * Ay - By * Ax
        hit = ~(((U < 0) | (V < 0) | (W < 0)) & ((U > 0) | (V > 0) | (W > 0)))
        det = (U + V) + W
        hit &= det != 0
        Az, Bz, Cz = Sz * Akz, Sz * Bkz, Sz * Ckz
        t_tri = ((U * Az + V * Bz) + W * Cz) / det
        hit &= t_tri >= 0
        lo = tuple(np.fmin(np.fmin(av[k], bv[k]), cv[k]) for k in range(3))
        hi = tuple(np.fmax(np.fmax(av[k], bv[k]), cv[k]) for k in range(3))
        t_enter, t_exit = slab_host(lo, hi, ov, dv)
        hit &= t_enter <= t_exit
        t = np.fmin(np.fmax(t_tri, t_enter), t_exit) + _F(0)
        hit &= t < _F(np.inf)
        bary = np.stack(np.broadcast_arrays(U / det, V / det, W / det), -1)
    return {"hit": hit, "t": t, "t_tri": t_tri, "t_enter": t_enter, "t_exit": t_exit, "bary": bary}


def first_hits_host(origins, dirs, verts, faces, chunk_elems: int = 1 << 20, pruned: bool = False):
    """The ray contract restated in numpy: brute force over all valid faces, every operation an fp32 elementwise one in the
    contract's order, chunked over the rays.  ``origins``, ``dirs``, ``verts``: anything ``np.asarray`` takes, reshaped to ``[., 3]``
    float32; ``faces`` to ``[F, 3]`` int64.  Returns ``face_idx [n]`` int64 (-1: no hit), ``t [n]`` float32 (+inf: no hit) and
    ``bary [n, 3]`` float32 (zeros: no hit).

    ``pruned``: the same answers, bit for bit and ties included, sooner on a large mesh.  The slab test of every triangle's own box
    is evaluated for every ray (a few operations), the triangle test only where ``t_enter <= t_exit``, which a hit requires by the
    contract; the first minimum in ascending face index is taken.  No tree and no order of the faces is involved."""
    o = np.ascontiguousarray(np.asarray(origins, dtype=_F).reshape(-1, 3))
    d = np.ascontiguousarray(np.asarray(dirs, dtype=_F).reshape(-1, 3))
    v = np.ascontiguousarray(np.asarray(verts, dtype=_F).reshape(-1, 3))
    f = np.ascontiguousarray(np.asarray(faces, dtype=np.int64).reshape(-1, 3))
    if o.shape != d.shape:
        raise ValueError(f"first_hits_host: {o.shape[0]} origins and {d.shape[0]} directions")
    n = o.shape[0]
    face_idx = np.full(n, -1, np.int64)
    t_hit = np.full(n, np.inf, _F)
    bary = np.zeros((n, 3), _F)
    ids = np.nonzero(valid_faces_host(v, f))[0]                 # ascending: the first minimum of a row is the lowest face index
    rows = np.nonzero(np.all(np.isfinite(o), axis=1) & np.all(np.isfinite(d), axis=1) & np.any(d != 0, axis=1))[0]
    if ids.size == 0 or rows.size == 0:
        return face_idx, t_hit, bary
    a, b, c = (v[f[ids, k]] for k in range(3))
    step = max(1, chunk_elems // ids.size)
    inf = _F(np.inf)
    for at in range(0, rows.size, step):
        r = rows[at:at + step]
        if pruned:
            lo = tuple(np.fmin(np.fmin(a[:, k], b[:, k]), c[:, k])[None, :] for k in range(3))
            hi = tuple(np.fmax(np.fmax(a[:, k], b[:, k]), c[:, k])[None, :] for k in range(3))
            with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
                t_enter, t_exit = slab_host(lo, hi, tuple(o[r, k][:, None] for k in range(3)), tuple(d[r, k][:, None] for k in range(3)))
            row, col = np.nonzero(t_enter <= t_exit)            # row-major: per ray, ascending face index
            if row.size == 0:
                continue
            got = ray_triangle_host(o[r][row], d[r][row], a[col], b[col], c[col])
            tt = np.where(got["hit"], got["t"], inf)
            least = np.full(r.size, inf, _F)
            np.minimum.at(least, row, tt)
            first = np.nonzero((tt == least[row]) & (tt < inf))[0]
            first = first[np.unique(row[first], return_index=True)[1]]      # the first minimum of every ray that hits
            face_idx[r[row[first]]] = ids[col[first]]
            t_hit[r[row[first]]] = tt[first]
            bary[r[row[first]]] = got["bary"][first]
            continue
        got = ray_triangle_host(o[r][:, None, :], d[r][:, None, :], a[None], b[None], c[None])
        tt = np.where(got["hit"], got["t"], inf)
        best = np.argmin(tt, axis=1)
        pick = np.arange(r.size)
        found = tt[pick, best] < inf
        face_idx[r[found]] = ids[best[found]]
        t_hit[r[found]] = tt[pick, best][found]
        bary[r[found]] = got["bary"][pick, best][found]
    return face_idx, t_hit, bary


# ---- the plan in numpy ----------------------------------------------------------------------------------------------------------------
LEAF = 64           # gsr_tree.h's kLeaf, kFan, kTreeMaxLevels, kAlign, kCellMax
FAN = 16
MAX_LEVELS = 6
ALIGN = 256
CELL_MAX = (1 << 21) - 1
NO_FACE = 0xFFFFFFFF
PLAN_MAGIC = b"TRIQ"


class PlanLayout(NamedTuple):
    """Where everything of a plan of ``F`` faces lies (gsr_meshquery.hip's ``tri_layout``, gsr_tree.h's ``tree_level``): ``counts[l]``
    boxes of level ``l`` (0: the leaves) start at box ``offsets[l]`` of the box region; ``records`` and ``boxes`` are byte offsets and
    ``bytes`` the whole, in 256-byte blocks.  A record is 48 bytes, a box 32 (two ``float4``: lo, hi)."""
    F: int
    leaves: int
    top: int
    counts: Tuple[int, ...]
    offsets: Tuple[int, ...]
    records: int
    boxes: int
    bytes: int


def _align_up(v: int) -> int:
    return (v + ALIGN - 1) // ALIGN * ALIGN


def plan_layout(F: int) -> PlanLayout:
    """The layout of the plan of a mesh of ``0 <= F < 2^30`` faces: pure arithmetic, ``tri_layout`` in Python."""
    F = int(F)
    if not 0 <= F <= MAX_FACES:
        raise ValueError(f"plan_layout: {F} faces (0 to 2^30 - 1)")
    counts = [(F + LEAF - 1) // LEAF]
    while counts[-1] > FAN and len(counts) < MAX_LEVELS:
        counts.append((counts[-1] + FAN - 1) // FAN)
    offsets = [sum(counts[:level]) for level in range(len(counts))]
    records = ALIGN
    boxes = _align_up(records + 48 * F)
    return PlanLayout(F, counts[0], len(counts) - 1, tuple(counts), tuple(offsets), records, boxes, _align_up(boxes + 32 * sum(counts)))


def _spread21_host(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.uint64) & np.uint64(0x1FFFFF)
    for shift, mask in ((32, 0x001F00000000FFFF), (16, 0x001F0000FF0000FF), (8, 0x100F00F00F00F00F), (4, 0x10C30C30C30C30C3),
                        (2, 0x1249249249249249)):
        x = (x | (x << np.uint64(shift))) & np.uint64(mask)
    return x


def _grid_cell_host(x: np.ndarray, lo, hi) -> np.ndarray:
    """``grid_cell``: ``t = (x - lo) / extent * 2097151`` when ``extent > 0``, else 0; the cell is ``uint(fmin(t, 2097151))`` when
    ``t >= 0``, else 0 (so a NaN, from infinite bounds, gives 0)."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        extent = _F(hi) - _F(lo)
        t = (x - _F(lo)) / extent * _F(CELL_MAX) if extent > 0 else np.zeros_like(x)
        keep = t >= 0
        return np.where(keep, np.fmin(np.where(keep, t, _F(0)), _F(CELL_MAX)), _F(0)).astype(np.uint32)


def morton_codes_host(verts, faces) -> np.ndarray:
    """The sort keys of the build, ``[F]`` uint64: the 63-bit Morton code of a valid face's centroid ``((a + b) + c) / 3`` on the
    bounds of the valid centroids, ``2^63`` for an invalid face.  All fp32, in the kernel's order."""
    v = np.ascontiguousarray(np.asarray(verts, dtype=_F).reshape(-1, 3))
    f = np.ascontiguousarray(np.asarray(faces, dtype=np.int64).reshape(-1, 3))
    codes = np.full(f.shape[0], 1 << 63, np.uint64)
    ids = np.nonzero(valid_faces_host(v, f))[0]
    if ids.size:
        with np.errstate(over="ignore", invalid="ignore"):
            m = ((v[f[ids, 0]] + v[f[ids, 1]]) + v[f[ids, 2]]) / _F(3)
        cells = [_spread21_host(_grid_cell_host(m[:, k], m[:, k].min(), m[:, k].max())) for k in range(3)]
        codes[ids] = cells[0] | (cells[1] << np.uint64(1)) | (cells[2] << np.uint64(2))
    return codes


def plan_host(verts, faces):
    """The build of ``gsr_meshquery.hip`` restated in numpy, operation for operation in fp32.  Returns ``order [F]`` int64 (the face
    of every record: a stable sort of ``morton_codes_host``, so equal codes, the invalid tail included, come in ascending face
    index), ``records [F, 3, 4]`` float32 (a valid face: ``(a, bits(f))``, ``(b, 0)``, ``(c, 0)``; an invalid one: NaN in x, y, z and
    0xFFFFFFFF in w, all three rows) and one ``(lo [n, 3], hi [n, 3])`` pair per level of ``plan_layout(F)``: a leaf is the union of
    its valid members' own boxes, every level above the union of up to 16 boxes below; a box without a valid member is
    (+inf, -inf).  The sign of a zero in a box is that of numpy's reduction, not necessarily the kernel's."""
    v = np.ascontiguousarray(np.asarray(verts, dtype=_F).reshape(-1, 3))
    f = np.ascontiguousarray(np.asarray(faces, dtype=np.int64).reshape(-1, 3))
    F = f.shape[0]
    layout = plan_layout(F)
    valid = valid_faces_host(v, f)
    order = np.argsort(morton_codes_host(v, f), kind="stable")
    ok = valid[order]
    records = np.full((F, 3, 4), np.nan, _F)
    words = records.view(np.uint32)
    words[:, :, 3] = NO_FACE
    corners = v[f[order[ok]]]                                        # [., 3 corners, 3 axes]
    records[ok, :, :3] = corners
    words[ok, 0, 3] = order[ok].astype(np.uint32)
    words[ok, 1:, 3] = 0
    lo = np.full((layout.leaves * LEAF, 3), np.inf, _F)
    hi = np.full((layout.leaves * LEAF, 3), -np.inf, _F)
    lo[:F][ok] = corners.min(axis=1)
    hi[:F][ok] = corners.max(axis=1)
    lo, hi = lo.reshape(layout.leaves, LEAF, 3).min(axis=1), hi.reshape(layout.leaves, LEAF, 3).max(axis=1)
    levels = [(lo, hi)]
    for count in layout.counts[1:]:
        wide_lo = np.full((count * FAN, 3), np.inf, _F)
        wide_hi = np.full((count * FAN, 3), -np.inf, _F)
        wide_lo[:lo.shape[0]], wide_hi[:hi.shape[0]] = lo, hi
        lo, hi = wide_lo.reshape(count, FAN, 3).min(axis=1), wide_hi.reshape(count, FAN, 3).max(axis=1)
        levels.append((lo, hi))
    return order, records, levels


# ---- the kernels ----------------------------------------------------------------------------------------------------------------------
class Plan:
    """The tree over one mesh: ``buffer``, one ``uint8`` device tensor (``gsr_closest_tri_plan``), and the mesh's ``F`` and ``V``."""
    __slots__ = ("buffer", "F", "V")

    def __init__(self, buffer: torch.Tensor, F: int, V: int):
        self.buffer, self.F, self.V = buffer, int(F), int(V)

    @property
    def device(self):
        return self.buffer.device


HOST = "closest_triangles_host"
ALLOCATES = "the call allocates its buffers and outputs"


def _why_not_mesh(verts, faces) -> Optional[str]:
    why = _takes.mesh(verts, faces, HOST)
    if why is None and (faces.shape[0] > MAX_FACES or verts.shape[0] > MAX_VERTS):
        why = f"{faces.shape[0]} faces and {verts.shape[0]} vertices: at most 2^30 - 1 and 2^31 - 1"
    return why


def _why_not_points(points, like, name: str = "points") -> Optional[str]:
    why = (_takes.tensors(((name, points, torch.float32),), like, HOST)
           or _takes.shaped(name, points, "[n, 3]", points.dim() == 2 and points.shape[1] == 3))
    if why is None and points.shape[0] > MAX_QUERIES:
        why = f"{points.shape[0]} {name}: at most 2^31 - 1"
    return why


def _why_not_plan(plan, verts, faces) -> Optional[str]:
    """``plan``: None, or the plan of this very mesh."""
    if plan is None:
        return None
    if not isinstance(plan, Plan):
        return f"plan must be a meshquery.Plan (got {type(plan).__name__})"
    if plan.F != int(faces.shape[0]) or plan.V != int(verts.shape[0]) or plan.device != verts.device:
        return (f"the plan is of a mesh with {plan.F} faces and {plan.V} vertices on {plan.device}, "
                f"not of this one ({int(faces.shape[0])}, {int(verts.shape[0])}, {verts.device})")
    if plan.buffer.dtype != torch.uint8 or int(plan.buffer.numel()) != _plan_bytes(plan.F):
        return (f"the plan's buffer is {int(plan.buffer.numel())} elements of {plan.buffer.dtype}, "
                f"a plan of {plan.F} faces is {_plan_bytes(plan.F)} bytes")
    return None


def _why_not_rays(origins, dirs, like) -> Optional[str]:
    why = _why_not_points(origins, like, "origins") or _why_not_points(dirs, like, "dirs")
    if why is None and origins.shape[0] != dirs.shape[0]:
        why = f"{origins.shape[0]} origins and {dirs.shape[0]} dirs"
    return why


def _plan_bytes(F: int) -> int:
    """Bytes of the plan of a mesh of ``F`` faces (``gsr_closest_tri_plan_bytes``; 0: more faces than the kernels take)."""
    from . import _lib

    return int(_lib.lib.gsr_closest_tri_plan_bytes(int(F)))


def _build(verts: torch.Tensor, faces: torch.Tensor) -> Plan:
    from . import _lib

    v, f = _takes.cs(verts, faces)
    V, F = int(v.shape[0]), int(f.shape[0])
    with torch.cuda.device(v.device):
        buffer, plan_bytes = _lib.scratch("gsr_closest_tri_plan_bytes", F, device=v.device)
        scratch, scratch_bytes = _lib.scratch("gsr_closest_tri_plan_scratch_bytes", F, device=v.device)
        _lib.call("gsr_closest_tri_plan", V, _lib.ptr(v), F, _lib.ptr(f), buffer.data_ptr(), plan_bytes, _lib.ptr(scratch), scratch_bytes,
                  device=v.device)
    return Plan(buffer, F, V)


def plan(verts: torch.Tensor, faces: torch.Tensor) -> Plan:
    """The tree over the mesh ``verts [V, 3]`` float32, ``faces [F, 3]`` int64 (both on one GPU), built on the current stream: pass it
    to :func:`closest_triangles` as often as the mesh is asked.  Raises ``ValueError`` with the reason for anything else."""
    _takes.refuse("meshquery.plan", _why_not_mesh(verts, faces) or _takes.capturing(ALLOCATES))
    return _build(verts, faces)


def closest_triangles(points: torch.Tensor, verts: torch.Tensor, faces: torch.Tensor, plan: Optional[Plan] = None,
                      return_points: bool = False):
    """For every point of ``points [n, 3]`` float32 the closest triangle of the mesh: ``face_idx [n]`` int64, ``sq_dist [n]`` float32
    and, with ``return_points``, ``closest [n, 3]`` float32 (the module docstring has the contract).  ``plan``: what :func:`plan`
    returned for this mesh (built here otherwise).  The queries are asked in Morton order and the answers put back (``_query``: the
    same answers, much sooner unless the caller's order is coherent already).  Queued on the current stream, no host synchronisation;
    not differentiable; non-contiguous inputs are copied.  Raises ``ValueError`` with the reason for CPU tensors, other dtypes or shapes, devices that
    differ, a plan of another mesh or of another size than its ``F`` asks for, and under graph capture."""
    _takes.refuse("closest_triangles", _why_not_mesh(verts, faces) or _why_not_points(points, verts) or _why_not_plan(plan, verts, faces)
                  or _takes.capturing(ALLOCATES))
    tree = plan if plan is not None else _build(verts, faces)
    return _query(points, tree, return_points)


def _spread21(x: torch.Tensor) -> torch.Tensor:
    """Bit k of an int64 ``x < 2^21`` -> bit 3k (gsr_tree.h's ``spread21``)."""
    x = (x | (x << 32)) & 0x001F00000000FFFF
    x = (x | (x << 16)) & 0x001F0000FF0000FF
    x = (x | (x << 8)) & 0x100F00F00F00F00F
    x = (x | (x << 4)) & 0x10C30C30C30C30C3
    x = (x | (x << 2)) & 0x1249249249249249
    return x


def morton_order(points: torch.Tensor) -> torch.Tensor:
    """Indices that put ``points [n, 3]`` in the order of their 63-bit Morton codes on their own bounds (non-finite coordinates count
    as 0): torch ops on the points' device, no host read.  The order only groups neighbours into waves: it never changes an answer."""
    p = torch.nan_to_num(points.detach(), nan=0.0, posinf=0.0, neginf=0.0)
    lo = p.min(dim=0).values
    extent = (p.max(dim=0).values - lo).clamp_min(torch.finfo(torch.float32).tiny)
    cell = ((p - lo) / extent * float((1 << 21) - 1)).to(torch.int64).clamp_(0, (1 << 21) - 1)
    code = _spread21(cell[:, 0]) | (_spread21(cell[:, 1]) << 1) | (_spread21(cell[:, 2]) << 2)
    return torch.argsort(code)


SORT_FROM = 128      # fewer queries than two waves are asked in the caller's order


def _query(points: torch.Tensor, tree: Plan, return_points: bool, sort_queries: bool = True):
    """The kernel gives a wave 64 consecutive queries and walks the tree once for all of them: it is fast when they are neighbours
    (measured on an MI355X, 1 M faces and 1 M queries drawn around the surface in random order: 6.9 ms with the sort and the way
    back in it, 215 ms asked as drawn; scripts/bench_meshquery.py).  So the queries are asked in Morton order and the answers put
    back; every answer is a function of its own query alone.  ``sort_queries=False`` (the tests, the benchmark) asks in the
    caller's order."""
    pts = _takes.c(points)
    n = int(pts.shape[0])
    face_idx = torch.empty(n, dtype=torch.int64, device=pts.device)
    sq_dist = torch.empty(n, dtype=torch.float32, device=pts.device)
    closest = torch.empty((n, 3), dtype=torch.float32, device=pts.device) if return_points else None
    _ask("gsr_closest_tri_query", (pts,), tree, (face_idx, sq_dist, closest), morton_order(pts) if sort_queries and n >= SORT_FROM else None)
    return (face_idx, sq_dist, closest) if return_points else (face_idx, sq_dist)


def _ask(entry: str, inputs, tree: Plan, outputs, order: Optional[torch.Tensor]) -> None:
    """A query entry point of the C ABI (``n``, the inputs, the plan and its size, the outputs) on the contiguous ``inputs [n, ...]``,
    asked in ``order`` (None: as given), the answers put back into ``outputs`` (each ``[n, ...]``, or None for one that is not
    wanted).  Nothing is asked of ``n == 0``."""
    from . import _lib

    n, dev = int(inputs[0].shape[0]), inputs[0].device
    if n == 0:
        return
    asked = inputs if order is None else [t[order] for t in inputs]
    out = outputs if order is None else [None if t is None else torch.empty_like(t) for t in outputs]
    with torch.cuda.device(dev):
        # the kernel reads the plan after this call returns, on THIS stream: a plan built on another one is not recycled under it
        tree.buffer.record_stream(torch.cuda.current_stream(dev))
        _lib.call(entry, n, *[t.data_ptr() for t in asked], tree.buffer.data_ptr(), int(tree.buffer.numel()), *[_lib.ptr(t) for t in out],
                  device=dev)
    if order is not None:
        for dst, src in zip(outputs, out):
            if dst is not None:
                dst.index_copy_(0, order, src)


def first_hits(origins: torch.Tensor, dirs: torch.Tensor, verts: torch.Tensor, faces: torch.Tensor, plan: Optional[Plan] = None,
               return_bary: bool = False, return_points: bool = False, sort: bool = True):
    """For every ray ``origins [n, 3]``, ``dirs [n, 3]`` (float32, not normalised) the first triangle of the mesh it hits:
    ``face_idx [n]`` int64 (-1: no hit) and ``t [n]`` float32 (+inf: no hit), then, with ``return_bary``, ``bary [n, 3]`` float32 (the
    weights of the face's three corners, zeros on a miss) and, with ``return_points``, ``points [n, 3]`` float32 (``o + t d``, zeros on
    a miss).  The contract is DESIGN.md 7m; :func:`first_hits_host` restates it.  ``plan``: what :func:`plan` returned for this mesh
    (built here otherwise): the plan of :func:`closest_triangles`.  The rays are asked in a coherent order (:func:`ray_order`) and the
    answers put back; ``sort=False`` asks them as given, which is sooner when they come side by side already, as the pixels of a
    camera do (``_cast`` has the measurements).  The answers are the same either way.  Queued on the current stream, no host synchronisation; not differentiable; non-contiguous inputs are copied.  Raises
    ``ValueError`` with the reason for what :func:`closest_triangles` refuses."""
    _takes.refuse("first_hits", _why_not_mesh(verts, faces) or _why_not_rays(origins, dirs, verts) or _why_not_plan(plan, verts, faces)
                  or _takes.capturing(ALLOCATES))
    tree = plan if plan is not None else _build(verts, faces)
    o, d = _takes.cs(origins, dirs)
    face_idx, t, bary = _cast(o, d, tree, return_bary, order=ray_order(o, d, verts) if sort and o.shape[0] >= SORT_FROM else None)
    out = [face_idx, t]
    if return_bary:
        out.append(bary)
    if return_points:
        # a multiplication, then an addition (no fused multiply-add), as first_hits_host's callers restate it
        out.append(torch.where((face_idx >= 0)[:, None], o + torch.where(face_idx >= 0, t, 0.0)[:, None] * d, 0.0))
    return tuple(out)


def ray_order(origins: torch.Tensor, dirs: torch.Tensor, verts: torch.Tensor) -> torch.Tensor:
    """Indices that put the rays in the Morton order of the point where each leaves the bounding box of the finite vertices (the
    origin clamped into the box for a ray that misses it, or when there is no finite vertex): rays that leave the box side by side
    cross much the same part of the tree.  torch ops on the rays' device, no host read.  The order only groups rays into waves: it
    never changes an answer."""
    o = torch.nan_to_num(origins.detach(), nan=0.0, posinf=0.0, neginf=0.0)
    if verts.shape[0] == 0:
        return morton_order(o)
    d = torch.nan_to_num(dirs.detach(), nan=0.0, posinf=0.0, neginf=0.0)
    v = verts.detach()
    fine = torch.isfinite(v).all(dim=1, keepdim=True)
    inf = float("inf")
    lo, hi = torch.where(fine, v, inf).min(dim=0).values, torch.where(fine, v, -inf).max(dim=0).values
    moving = d != 0
    inv = 1.0 / torch.where(moving, d, 1.0)
    inside = (lo <= o) & (o <= hi)
    far = torch.where(moving, torch.maximum((lo - o) * inv, (hi - o) * inv), torch.where(inside, inf, -inf))
    near = torch.where(moving, torch.minimum((lo - o) * inv, (hi - o) * inv), torch.where(inside, -inf, inf))
    t_exit = far.min(dim=1).values
    leaves = (near.max(dim=1).values.clamp_min(0.0) <= t_exit) & torch.isfinite(t_exit)
    at = torch.where(leaves[:, None], o + torch.where(leaves, t_exit, 0.0)[:, None] * d, torch.maximum(torch.minimum(o, hi), lo))
    return morton_order(at)


def _cast(origins: torch.Tensor, dirs: torch.Tensor, tree: Plan, return_bary: bool, order: Optional[torch.Tensor] = None):
    """``gsr_ray_first_hit`` on contiguous rays, asked in ``order`` (None: as given) and put back.  A wave takes 64 consecutive rays
    and walks the tree once for all of them, so it is fast when they run side by side; every answer is a function of its own ray
    alone.  Measured on an MI355X on 1 M faces (scripts/bench_meshrays.py): 1 M rays from inside in random directions and random
    order 9.9 ms in ``ray_order`` (2.5 ms of it the order itself) with the way back, 26 ms as given; the 2 M rays of a 1080p camera
    2.3 ms as given, in row-major pixel order, and 6.3 ms ordered -- the order costs more than it saves when the rays come side by
    side already, hence ``first_hits(..., sort=False)``.  Returns ``face_idx``, ``t``, ``bary`` (None unless wanted)."""
    n, dev = int(origins.shape[0]), origins.device
    face_idx = torch.empty(n, dtype=torch.int64, device=dev)
    t = torch.empty(n, dtype=torch.float32, device=dev)
    bary = torch.empty((n, 3), dtype=torch.float32, device=dev) if return_bary else None
    _ask("gsr_ray_first_hit", (origins, dirs), tree, (face_idx, t, bary), order)
    return face_idx, t, bary


def _as_tensor(x, device, dtype):
    return torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x).to(device, dtype)


class Scene:
    """A mesh to ask closest points and first hits of, for code written against ``open3d.t.geometry.RaycastingScene``: the plan is
    built once, here.  ``verts``, ``faces``: numpy arrays or tensors (moved to ``device``, default the current GPU)."""

    def __init__(self, verts, faces, device=None):
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.verts = torch.as_tensor(np.asarray(verts) if not isinstance(verts, torch.Tensor) else verts).to(dev, torch.float32).contiguous()
        self.faces = torch.as_tensor(np.asarray(faces) if not isinstance(faces, torch.Tensor) else faces).to(dev, torch.int64).contiguous()
        self.plan = plan(self.verts, self.faces)

    def compute_closest_points(self, points) -> dict:
        """``points``: ``[n, 3]``, numpy or torch, any float dtype.  Returns device tensors: ``primitive_ids`` int64 ``[n]`` (-1: no
        answer), ``points`` float32 ``[n, 3]``, ``distances`` float32 ``[n]`` (Euclidean) and ``squared_distances``."""
        pts = torch.as_tensor(np.asarray(points) if not isinstance(points, torch.Tensor) else points)
        pts = pts.to(self.verts.device, torch.float32).reshape(-1, 3)
        face_idx, sq_dist, closest = closest_triangles(pts, self.verts, self.faces, plan=self.plan, return_points=True)
        return {"primitive_ids": face_idx, "points": closest, "distances": torch.sqrt(sq_dist), "squared_distances": sq_dist}

    def cast_rays(self, rays) -> dict:
        """``rays``: ``[n, 6]`` (origin, direction; the direction is not normalised and ``t_hit`` is in its units, as in Open3D),
        numpy or torch, any float dtype.  Returns device tensors: ``t_hit`` float32 ``[n]`` (+inf: no hit), ``primitive_ids`` int64
        ``[n]`` and ``primitive_uvs`` float32 ``[n, 2]`` (the weights of the face's second and third corner; zeros on a miss).
        Unlike Open3D, whose ``primitive_ids`` are uint32 with 4294967295 for no hit, a miss is -1 here.  ``geometry_ids`` and
        ``primitive_normals`` are not returned."""
        r = _as_tensor(rays, self.verts.device, torch.float32).reshape(-1, 6)
        face_idx, t, bary = first_hits(r[:, :3], r[:, 3:], self.verts, self.faces, plan=self.plan, return_bary=True)
        return {"t_hit": t, "primitive_ids": face_idx, "primitive_uvs": bary[:, 1:].contiguous()}


class RayIntersector:
    """The first-hit questions of ``trimesh``'s ``mesh.ray`` on the GPU, numpy in and numpy out: ``RayIntersector(mesh.vertices,
    mesh.faces)`` where the caller wrote ``mesh.ray``.  The answers follow this library's contract, whose choices at
    ties and at grazing rays need not be trimesh's; locations are float32."""

    def __init__(self, verts, faces, device=None):
        self.scene = Scene(verts, faces, device=device)

    def _ask(self, ray_origins, ray_directions, points: bool = False):
        dev = self.scene.verts.device
        o = _as_tensor(ray_origins, dev, torch.float32).reshape(-1, 3)
        d = _as_tensor(ray_directions, dev, torch.float32).reshape(-1, 3)
        return first_hits(o, d, self.scene.verts, self.scene.faces, plan=self.scene.plan, return_points=points)

    def intersects_first(self, ray_origins, ray_directions) -> np.ndarray:
        """The first face every ray hits, ``[n]`` int64, -1 for none."""
        return self._ask(ray_origins, ray_directions)[0].cpu().numpy()

    def intersects_any(self, ray_origins, ray_directions) -> np.ndarray:
        """Whether every ray hits anything, ``[n]`` bool."""
        return (self._ask(ray_origins, ray_directions)[0] >= 0).cpu().numpy()

    def intersects_location(self, ray_origins, ray_directions, multiple_hits: bool = False):
        """``(locations [m, 3] float32, index_ray [m] int64, index_tri [m] int64)`` of the rays that hit, in ray order: the first
        hit of each.  ``multiple_hits=True`` (all hits of every ray) is not provided and raises ``NotImplementedError``."""
        if multiple_hits:
            raise NotImplementedError("RayIntersector.intersects_location: only the first hit of a ray is computed (multiple_hits=False)")
        face_idx, _, points = self._ask(ray_origins, ray_directions, points=True)
        index_ray = torch.nonzero(face_idx >= 0).reshape(-1)
        return points[index_ray].cpu().numpy(), index_ray.cpu().numpy(), face_idx[index_ray].cpu().numpy()
