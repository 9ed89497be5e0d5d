"""Shared by tests/test_meshraster.py and tests/test_meshraster_gpu.py: the scene builder, hand-built faces, and the float64 truth of the
mesh rasterizer's contract (the module docstring of autovfx_amd/meshraster.py), evaluated by brute force, face by face.

Bars.  ``HOST_ERR_*`` are the largest absolute errors of the fp32 numpy restatement against this truth on the decided pixels
of the four ``SCENES`` at K = 10, with ``perspective_correct`` on and off; ``BAR_*`` = 4 x those, the margin for another platform's
differently vectorised numpy.  ``dists`` is compared absolutely: relatively it is off by up to a percent where the distance is tiny.
"""
from __future__ import annotations

import functools

import numpy as np

F = np.float32
SCENES = ((37, 53, 300, 1), (53, 37, 300, 2), (32, 32, 600, 3), (64, 48, 1000, 4))     # H, W, faces, seed
UNDECIDED_W = 1e-5          # a pixel this close (in barycentric units) to an edge of a face that passes the culls is undecided
UNDECIDED_Z = 1e-5          # ... and one whose K + 1 nearest hold two depths closer than this times max(1, |z|)
MAX_UNDECIDED = 0.01        # at most this share of a scene's pixels may be set aside

# measured with tests/test_meshraster.py::test_host_restatement_against_truth (it prints them) on x86-64 numpy: z is worst with
# perspective_correct off on the 1000-face scene (8.0e-6 with it on), the barycentrics on the same scene either way
HOST_ERR_Z, HOST_ERR_BARY, HOST_ERR_DIST = 3.42e-5, 2.45e-5, 8.57e-7
BAR_Z, BAR_BARY, BAR_DIST = 4 * HOST_ERR_Z, 4 * HOST_ERR_BARY, 4 * HOST_ERR_DIST


def scene(n_faces: int, seed: int) -> np.ndarray:
    """``[n_faces, 3, 3]`` float32: triangles of very different sizes over and around the image, at overlapping depths, behind two
    screen-filling ones."""
    g = np.random.default_rng(seed)
    centres = g.uniform(-1.5, 1.5, (n_faces, 1, 2))
    radii = np.exp(g.uniform(np.log(0.03), np.log(0.6), (n_faces, 1, 1)))
    xy = centres + radii * g.standard_normal((n_faces, 3, 2))
    z = g.uniform(0.5, 10.0, (n_faces, 1)) + g.uniform(-0.3, 0.3, (n_faces, 3))
    big = np.array([(-3.0, -3.0), (3.0, -3.0), (0.0, 4.0)])
    xy[0] = big
    xy[1] = big * (1.0, 1.01)
    return np.ascontiguousarray(np.concatenate([xy, z[:, :, None]], axis=2), dtype=F)


def one_mesh(fv: np.ndarray):
    """The three index arguments for a single mesh without clipped faces."""
    n = len(fv)
    return np.array([0], np.int64), np.array([n], np.int64), np.full(n, -1, np.int64)


def tri_around(x: float, y: float, z=1.0, r: float = 0.1) -> np.ndarray:
    """A small upright triangle whose inside holds (x, y)."""
    zs = np.broadcast_to(np.asarray(z, np.float64), (3,))
    return np.array([(x - r, y - r, zs[0]), (x + r, y - r, zs[1]), (x, y + r, zs[2])], F)


def _ndc64(i, S1, S2):
    rng = 2.0 * S1 / S2 if S1 > S2 else 2.0
    return -rng / 2.0 + (rng * i + rng / 2.0) / S1


def _edge64(p, a, b):
    return (p[0] - a[0]) * (b[1] - a[1]) - (p[1] - a[1]) * (b[0] - a[0])


def truth(face_verts, first, num, nbr, image_size, K, perspective_correct=False, clip_barycentric_coords=False, cull_backfaces=False):
    """The contract in float64, one face at a time over the whole pixel grid.  Returns ``pix_to_face``, ``zbuf``, ``bary_coords``,
    ``dists`` as the operator shapes them, and ``undecided [N, H, W]``."""
    fv = np.asarray(face_verts, np.float64)
    H, W = image_size
    N, n_faces = len(first), len(fv)
    X, Y = np.meshgrid(_ndc64(W - 1 - np.arange(W), W, H), _ndc64(H - 1 - np.arange(H), H, W))
    p = (X, Y)
    out_face = np.full((N, H, W, K), -1, np.int64)
    out_z, out_d, out_b = np.full((N, H, W, K), -1.0), np.full((N, H, W, K), -1.0), np.full((N, H, W, K, 3), -1.0)
    undecided = np.zeros((N, H, W), bool)
    for n in range(N):
        faces = [f for f in range(max(int(first[n]), 0), min(int(first[n]) + int(num[n]), n_faces))
                 if not any(int(first[m]) <= f < int(first[m]) + int(num[m]) for m in range(n))]
        kept, depth, dist, bary = {}, {}, {}, {}
        for f in faces:
            v0, v1, v2 = fv[f, 0], fv[f, 1], fv[f, 2]
            area = _edge64(v0, v1, v2)
            if max(v0[2], v1[2], v2[2]) < 1e-8 or abs(area) <= 1e-8 or (cull_backfaces and area < 0):
                continue
            den = _edge64(v2, v0, v1) + 1e-8
            w = np.stack([_edge64(p, v1, v2) / den, _edge64(p, v2, v0) / den, _edge64(p, v0, v1) / den])
            undecided[n] |= np.abs(w).min(0) < UNDECIDED_W
            box = (X >= fv[f, :, 0].min()) & (X <= fv[f, :, 0].max()) & (Y >= fv[f, :, 1].min()) & (Y <= fv[f, :, 1].max())
            b = w
            if perspective_correct:
                t = np.stack([w[0] * v1[2] * v2[2], v0[2] * w[1] * v2[2], v0[2] * v1[2] * w[2]])
                b = t / np.maximum(t.sum(0), 1e-8)
            if clip_barycentric_coords:
                c = np.clip(b, 0.0, 1.0)
                b = c / np.maximum(c.sum(0), 1e-5)
            pz = b[0] * v0[2] + b[1] * v1[2] + b[2] * v2[2]
            kept[f] = box & (w > 0).all(0) & ~(pz < 0)
            depth[f], bary[f] = pz, b
            dist[f] = np.minimum(_seg_grid(p, v0, v1), np.minimum(_seg_grid(p, v0, v2), _seg_grid(p, v1, v2)))
        final = {}
        for f in kept:
            g = int(nbr[f])
            final[f] = kept[f]
            if g >= 0 and g != f and g in kept:
                final[f] = kept[f] & ~(kept[g] & ((dist[g] < dist[f]) | ((dist[g] == dist[f]) & (g < f))))
        order = sorted(final)
        if not order:
            continue
        keys = np.stack([np.where(final[f], depth[f], np.inf) for f in order])           # [faces, H, W], faces ascending
        rank = np.argsort(keys, axis=0, kind="stable")[:K + 1]
        near = np.take_along_axis(keys, rank, axis=0)
        with np.errstate(invalid="ignore"):
            gap = near[1:] - near[:-1]
            close = np.isfinite(near[1:]) & (gap < UNDECIDED_Z * np.maximum(1.0, np.abs(near[:-1])))
        undecided[n] |= close.any(0)
        for k in range(min(K, len(order))):
            found = np.isfinite(near[k])
            which = np.asarray(order)[rank[k]]
            out_face[n, :, :, k] = np.where(found, which, -1)
            for f in np.unique(which[found]):
                at = found & (which == f)
                out_z[n, :, :, k][at] = depth[f][at]
                out_d[n, :, :, k][at] = -dist[f][at]
                out_b[n, :, :, k][at] = np.moveaxis(bary[f], 0, -1)[at]
    return out_face, out_z, out_b, out_d, undecided


def _seg_grid(p, a, b):
    u = b[:2] - a[:2]
    l2 = float(u @ u)
    if l2 <= 1e-8:
        return (p[0] - b[0]) ** 2 + (p[1] - b[1]) ** 2
    t = np.clip((u[0] * (p[0] - a[0]) + u[1] * (p[1] - a[1])) / l2, 0.0, 1.0)
    return (p[0] - (a[0] + t * u[0])) ** 2 + (p[1] - (a[1] + t * u[1])) ** 2


@functools.lru_cache(maxsize=None)
def scene_truth(index: int, K: int = 10, perspective_correct: bool = True):
    """``(face_verts, truth(...))`` of ``SCENES[index]``, computed once per process and shared (read-only) by the tests."""
    H, W, n_faces, seed = SCENES[index]
    fv = scene(n_faces, seed)
    out = truth(fv, *one_mesh(fv), (H, W), K, perspective_correct=perspective_correct)
    for a in out:
        a.setflags(write=False)
    fv.setflags(write=False)
    return fv, out


def against_truth(got, want, label: str = ""):
    """The comparison both test files use: identical ``pix_to_face`` and the bars on the three float outputs, on the decided pixels; at
    most ``MAX_UNDECIDED`` of the pixels set aside.  Returns the largest errors (z, bary, dist) for the caller to print."""
    face, z, b, d, undecided = want
    share = undecided.mean()
    assert share <= MAX_UNDECIDED, f"{label}: {share:.3%} of the pixels undecided"
    ok = ~undecided
    assert np.array_equal(np.asarray(got[0])[ok], face[ok]), f"{label}: pix_to_face differs on decided pixels"
    errs = tuple(float(np.abs(np.asarray(g, np.float64)[ok] - t[ok]).max()) for g, t in zip(got[1:], (z, b, d)))
    print(f"{label}: undecided {share:.3%}, max abs error z {errs[0]:.2e} bary {errs[1]:.2e} dists {errs[2]:.2e}")
    return errs
