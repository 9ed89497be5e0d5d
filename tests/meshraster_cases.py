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
# the same on the two NEAR_PLANE scenes (tests/test_meshraster.py::test_near_plane_restatement_against_truth prints them), flags off and
# perspective_correct with clip_barycentric_coords: z is worst with the flags off on seed 102, the barycentrics likewise
NEAR_HOST_ERR_Z, NEAR_HOST_ERR_BARY, NEAR_HOST_ERR_DIST = 4.30e-5, 1.27e-5, 8.58e-7
NEAR_BAR_Z, NEAR_BAR_BARY, NEAR_BAR_DIST = 4 * NEAR_HOST_ERR_Z, 4 * NEAR_HOST_ERR_BARY, 4 * NEAR_HOST_ERR_DIST


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


def near_plane_scene(n_faces: int, seed: int) -> np.ndarray:
    """``scene()`` with the z of faces 2.. drawn per vertex from [-1, 3]: faces that straddle the camera plane (the barycentric clip and the
    ``pz < 0`` skip do something), faces wholly behind it (culled) and perspective denominators around zero (the eps clamp)."""
    fv = scene(n_faces, seed)
    fv[2:, :, 2] = np.random.default_rng((seed, 7)).uniform(-1.0, 3.0, (n_faces - 2, 3))
    return fv


FLT_MAX = float(np.finfo(F).max)


def scaled_scene(n_faces: int, seed: int, z_scale: float = 1.0, xy_scale: float = 1.0) -> np.ndarray:
    """``scene()`` with z and xy multiplied in float64 and brought back to the largest finite float32 where the product exceeds it: every
    input stays finite, the intermediates overflow."""
    fv = scene(n_faces, seed).astype(np.float64)
    fv[:, :, 2] *= z_scale
    fv[:, :, :2] *= xy_scale
    return np.ascontiguousarray(np.clip(fv, -FLT_MAX, FLT_MAX), dtype=F)


def non_finite_scene(n_faces: int, seed: int, every: int = 7):
    """``(broken, finite_only, is_broken)``: ``scene()`` with NaN, +inf and -inf scattered over x, y and z of every ``every``-th face from
    face 3 on (one to three coordinates each, all nine in turn; face 3 itself fills the screen with one depth +inf), and the same scene with those faces put wholly behind the camera
    (culled: the indices of the others stay)."""
    fv = scene(n_faces, seed)
    g = np.random.default_rng((seed, 11))
    is_broken = np.zeros(n_faces, bool)
    is_broken[3::every] = True
    broken, finite_only = fv.copy(), fv.copy()
    values = (np.nan, np.inf, -np.inf)
    for i, f in enumerate(np.nonzero(is_broken)[0]):
        coords = broken[f].reshape(-1)
        coords[i % 9] = values[(i + i // 9) % 3]                       # every coordinate with every value in turn ...
        for at in g.choice(9, size=g.integers(0, 3), replace=False): # ... and up to two more anywhere
            coords[at] = values[g.integers(0, 3)]
    broken[3] = flat(BIG * 1.02, (np.inf, 5.0, 5.0))                 # over every pixel at depth +inf (perspective_correct: NaN)
    finite_only[is_broken, :, 2] = -1.0
    assert np.isfinite(broken[~is_broken]).all() and not np.isfinite(broken[is_broken]).all(axis=(1, 2)).any()
    return broken, finite_only, is_broken


def one_mesh(fv: np.ndarray):
    """The three index arguments for a single mesh without clipped faces."""
    n = len(fv)
    return np.array([0], np.int64), np.array([n], np.int64), np.full(n, -1, np.int64)


def tri_around(x: float, y: float, z=1.0, r: float = 0.1) -> np.ndarray:
    """A small upright triangle whose inside holds (x, y)."""
    zs = np.broadcast_to(np.asarray(z, np.float64), (3,))
    return np.array([(x - r, y - r, zs[0]), (x + r, y - r, zs[1]), (x, y + r, zs[2])], F)


CHUNK = 256                 # faces per LDS chunk of the raster kernel (gsr_meshraster.hip: kMeshChunk)
SCAN_ROUND = 256 * 16       # tiles per round of the scan kernel (kMeshThreads * kScanPerLane)
WAVE_RECT = 64              # a rectangle of more tiles than this is walked by the wave (kWaveRect)
BIG = np.array([(-3.0, -3.0), (3.0, -3.0), (0.0, 4.0)])    # holds [-1, 1]^2: every pixel of a square image


def flat(xy, z) -> np.ndarray:
    """One face from three (x, y) and a depth (or three)."""
    return np.concatenate([np.asarray(xy, np.float64), np.broadcast_to(np.asarray(z, np.float64), (3,))[:, None]], axis=1).astype(F)


@functools.lru_cache(maxsize=None)
def many_small_meshes(n_meshes: int, seed: int = 21):
    """``n_meshes`` meshes of three faces each for 17 x 17 images (4 tiles each): 1024 of them fill one round of the scan exactly, 1025 need
    a second.  The first meshes of a longer batch are those of a shorter one."""
    g = np.random.default_rng(seed)
    n = 3 * 1025
    assert n_meshes <= 1025
    x, y, z, r = g.uniform(-1, 1, n), g.uniform(-1, 1, n), g.uniform(1, 2, n), g.uniform(0.2, 1.5, n)
    fv = np.stack([tri_around(*a) for a in zip(x, y, z, r)])[:3 * n_meshes]
    return fv, 3 * np.arange(n_meshes, dtype=np.int64), np.full(n_meshes, 3, np.int64), np.full(3 * n_meshes, -1, np.int64)


def large_image_faces(side: int = 1041) -> np.ndarray:
    """14 faces for one ``side x side`` image (1041: 66 x 66 = 4356 tiles, the last row and column of tiles one pixel wide): two that fill
    the screen, so that one wave-walked rectangle spans every tile of both scan rounds, faces 2..7 small ones along the last pixel row and
    faces 8..13 along the last pixel column (the centre of column W - 1 is at x = -1 + 1 / W, of row H - 1 at y = -1 + 1 / H).  The
    restatement's time goes with pixels times faces: 14 keep it near three seconds."""
    px = 2.0 / side
    edge = -1.0 + px / 2
    along = np.linspace(-0.999, 0.95, 6)
    faces = [flat(BIG, 5.0), flat(BIG * (1.0, 1.01), 6.0)]
    faces += [tri_around(x, edge, 1.0 + 0.1 * i, r=3 * px) for i, x in enumerate(along)]
    faces += [tri_around(edge, y, 2.5 + 0.1 * i, r=3 * px) for i, y in enumerate(along)]
    return np.stack(faces)


def mixed_wave_kind(f):
    """Of face ``f`` of mesh 1 in ``mixed_waves_two_meshes``: 0 fills the screen, 1 lies behind the camera, 2 and 3 off the image, 4..7 are
    ordinary.  The kinds move on by one lane from wave to wave, so lane 0 of a wave -- and every other lane -- is of another kind in each."""
    return (f + f // 64) % 8


def mixed_waves_two_meshes(n_faces: int = 700, first1: int = 160, seed: int = 12):
    """Two meshes for 150 x 140 (10 x 9 tiles).  Mesh 0 is ``scene()``'s first ``first1`` faces, with one more screen-filling face at 130; in
    mesh 1 every eighth face fills the screen (a wave-walked rectangle with ``base != 0``), every eighth lies behind the camera (culled), two
    in eight lie off the image, the rest are ordinary: each of its waves holds all four kinds.  700 faces are two workgroups and 188 lanes
    of a third; wave 2 (faces 128..191) holds faces, and wave-walked rectangles, of both meshes."""
    fv = scene(n_faces, seed)
    g = np.random.default_rng((seed, 3))
    fv[130, :, :2] = BIG * (1.0, 1.003)
    for f in range(first1, n_faces):
        kind = mixed_wave_kind(f)
        if kind == 0:
            fv[f, :, :2] = BIG * (1.0, 1.0 + 0.001 * (f % 5))
            fv[f, :, 2] = g.uniform(0.5, 10.0) + g.uniform(-0.3, 0.3, 3)
        elif kind == 1:
            fv[f, :, 2] = -g.uniform(0.1, 2.0, 3)
        elif kind == 2:
            fv[f, :, 0] += 10.0
        elif kind == 3:
            fv[f, :, 1] -= 10.0
    return (fv, np.array([0, first1], np.int64), np.array([first1, n_faces - first1], np.int64), np.full(n_faces, -1, np.int64))


# On 160 x 160 (10 x 10 tiles) a pixel is 1 / 80 wide and the binning's span of [lo, hi] is pixel indices
# floor((lo + 1) * 80 - 0.5) - 1 .. ceil((hi + 1) * 80 - 0.5) + 1 (index i is column or row 159 - i):
#   [-0.775, 0.775]   -> floor(17.5) - 1 = 16 .. ceil(141.5) + 1 = 143: columns 16..143, tiles 1..8, 8 tiles
#   [-0.775, 0.7875]  -> 16 .. ceil(142.5) + 1 = 144: columns 15..143, tiles 0..8, 9 tiles
RECT_LO, RECT_HI8, RECT_HI9 = -0.775, 0.775, 0.7875


def rect_bound_faces() -> np.ndarray:
    """Three faces for 160 x 160 whose padded boxes land on 8 x 8 = 64 tiles (walked by its lane), 9 x 8 = 72 and 8 x 9 = 72 (by the wave)."""
    tri = lambda hx, hy, z: flat([(RECT_LO, RECT_LO), (hx, RECT_LO), (0.0, hy)], z)
    return np.stack([tri(RECT_HI8, RECT_HI8, 1.0), tri(RECT_HI9, RECT_HI8, 2.0), tri(RECT_HI8, RECT_HI9, 3.0)])


def rect_bound_scene(seed: int = 13) -> np.ndarray:
    """``scene()`` with the three faces of ``rect_bound_faces`` in two different waves."""
    fv = scene(130, seed)
    fv[[7, 8, 100]] = rect_bound_faces()
    return fv


TIE = tri_around(0.75, 0.75, 2.0, r=0.15)                    # on 64 x 64: columns and rows 3..12, inside tile 0 with its padding
N_TIES = 2 * CHUNK + 40


def long_tie(interleaved: bool):
    """``(face_verts, expected faces of the covered pixels at K = 16)``: ``N_TIES`` coincident faces in one tile of 64 x 64, more than two LDS
    chunks whose order in the tile's list is whatever the fill's atomics gave.  ``interleaved``: every fifth index holds a farther face of
    a depth of its own, and five indices spread over the range hold nearer ones, nearest last."""
    if not interleaved:
        return np.stack([TIE] * N_TIES), np.arange(16)
    near_at = (7, 130, 300, 420, 640)
    faces, ties, near = [], [], []
    while len(ties) < N_TIES:
        i = len(faces)
        depth = 2.0
        if i in near_at:
            depth = 1.5 - 0.1 * near_at.index(i)
            near.append(i)
        elif i % 5 == 1:
            depth = 3.0 + 0.01 * i
        else:
            ties.append(i)
        faces.append(tri_around(0.75, 0.75, depth, r=0.15))
    assert len(near) == 5
    return np.stack(faces), np.array(near[::-1] + ties[:11])


def tie_of_two_walks():
    """``(face_verts, (H, W), both, wide_only)`` -- ``N_TIES`` faces of exactly equal depth in two shapes, alternating by index, on a 16 x 1040 strip
    (1 x 65 tiles): the even ones span all 65 tiles and are listed by the wave, the odd ones touch at most 10 and are listed by their
    lane, *before* the even ones of the same wave -- a list order that is certainly not the index order.  ``both`` marks the columns both
    shapes cover, ``wide_only`` those only the even ones do.  The depth is exactly 2 on every pixel: the strip's pixel centres are odd multiples of 1 / 16, the vertices integers and
    the doubled areas (8192 and 128) powers of two above 1 (so ``+ eps`` changes nothing), hence every barycentric is a dyadic rational
    computed without rounding and the three sum to exactly 1."""
    wide = flat([(-128, -2), (896, -2), (-128, 6)], 2.0)         # x + 128 (y + 2) <= 896: holds the strip |x| <= 65, |y| <= 1
    narrow = flat([(-8, -2), (8, -2), (-8, 6)], 2.0)             # x + 2 (y + 2) <= 8: holds -8 < x < 2 on every row
    fv = np.stack([wide if i % 2 == 0 else narrow for i in range(N_TIES)])
    H, W = 16, 1040
    x = -65.0 + (2 * (W - 1 - np.arange(W)) + 1) / 16.0
    return fv, (H, W), (x > -8) & (x < 2), (x < -8) | (x > 8)


# The neighbour rule's guards: A, B, C overlap around the centre (A is nearest and widest); each case is (face_verts, first, num, nbr).
_A, _B, _C = tri_around(0, 0, 1, r=0.95), tri_around(0.25, 0.25, 2, r=0.6), tri_around(0, 0, 3, r=0.9)


def _mesh(faces, nbr, first=None, num=None):
    fv = np.stack(faces)
    return (fv, np.array([0] if first is None else first, np.int64), np.array([len(fv)] if num is None else num, np.int64),
            np.asarray(nbr, np.int64))


def neighbour_names_itself():
    return _mesh([_A, _B, _C], [0, 1, 2])


def neighbour_is_culled():
    """A names a back face (B's twin, wound the other way), B names a face behind the camera: with ``cull_backfaces`` neither exists."""
    front = lambda t: t[::-1].copy()                                # tri_around winds its faces backwards: edge(v0, v1, v2) < 0
    return _mesh([front(_A), front(_B), _B, tri_around(0.25, 0.25, -1.0, r=0.6)], [2, 3, -1, -1])


def neighbour_in_the_other_mesh():
    """Mesh 0 is A, B; mesh 1 is A, B, C (faces 2, 3, 4).  Face 0 names face 3 and face 4 names face 1: the other mesh, ahead and behind.
    Faces 2 and 3 name each other: a pair inside mesh 1, whose first face is not 0."""
    return _mesh([_A, _B, _A, _B, _C], [3, -1, 3, 2, 1], first=[0, 2], num=[2, 3])


def neighbour_out_of_range():
    """``F``, ``2^31``, ``2^40`` and ``-2``: no face."""
    return _mesh([_A, _B, _C, _B], [4, 2 ** 31, 2 ** 40, -2])


def neighbour_is_a_twin():
    """Two identical triangles that name each other, in front of C."""
    return _mesh([_B, _B, _C], [1, 0, -1])


def neighbour_across_chunks(seed: int = 8):
    """A pair at the two ends of a tile's list of ``CHUNK + 42`` faces (64 x 64, tile 0): face 0 is listed by the first workgroup of the fill
    and the last face by the second."""
    g = np.random.default_rng(seed)
    n = CHUNK + 40
    between = [tri_around(x, y, z, r=0.03) for x, y, z in zip(g.uniform(0.55, 0.95, n), g.uniform(0.55, 0.95, n), g.uniform(2, 3, n))]
    faces = [tri_around(0.75, 0.75, 1.0, r=0.2)] + between + [tri_around(0.78, 0.78, 1.5, r=0.15)]
    nbr = np.full(len(faces), -1, np.int64)
    nbr[0], nbr[-1] = len(faces) - 1, 0
    return _mesh(faces, nbr)


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


NEAR_PLANE = ((37, 53, 300, 101), (37, 53, 300, 102))          # H, W, faces, seed: the near-plane scenes held against the truth


@functools.lru_cache(maxsize=None)
def near_plane_truth(index: int, perspective_correct: bool, clip_barycentric_coords: bool, K: int = 10):
    """``(face_verts, truth(...))`` of ``NEAR_PLANE[index]``, computed once per process and shared (read-only)."""
    H, W, n_faces, seed = NEAR_PLANE[index]
    fv = near_plane_scene(n_faces, seed)
    out = truth(fv, *one_mesh(fv), (H, W), K, perspective_correct=perspective_correct, clip_barycentric_coords=clip_barycentric_coords)
    for a in out:
        a.setflags(write=False)
    fv.setflags(write=False)
    return fv, out


def finite_faces_are_a_prefix(got, finite_only, is_broken, label: str = ""):
    """What holds for a scene with non-finite faces (``is_broken``): per pixel, the listed faces with the broken ones taken out are the first
    of the finite-only scene's list, with its ``zbuf``, ``bary_coords`` and ``dists`` bit for bit; and the list stops short of the
    finite-only one only where broken faces took the slots.  Returns how many slots broken faces hold."""
    face, want = np.asarray(got[0]), np.asarray(finite_only[0])
    K = face.shape[-1]
    listed = face >= 0
    assert (listed[..., :-1] >= listed[..., 1:]).all(), f"{label}: an empty slot before a filled one"
    keep = listed & ~is_broken[np.clip(face, 0, None)]
    order = np.argsort(~keep, axis=-1, kind="stable")               # the kept slots first, in their order
    n_kept, n_want = keep.sum(-1), (want >= 0).sum(-1)
    prefix = np.arange(K) < n_kept[..., None]
    assert (n_kept <= n_want).all(), f"{label}: more finite faces than the finite-only scene lists"
    assert (listed.sum(-1)[n_kept < n_want] == K).all(), f"{label}: a finite face is missing though a slot is free"
    bits = lambda a: a.view(np.int32) if a.dtype == F else a
    for name, g, w in zip(("pix_to_face", "zbuf", "bary_coords", "dists"), got, finite_only):
        g, w = bits(np.asarray(g)), bits(np.asarray(w))
        at = order if g.ndim == face.ndim else order[..., None]
        mask = prefix if g.ndim == face.ndim else prefix[..., None]
        differ = (np.take_along_axis(g, at, axis=face.ndim - 1) != w) & mask
        assert not differ.any(), f"{label}: {name} of the finite faces differs in {int(differ.sum())} elements, first at {tuple(np.argwhere(differ)[0])}"
    return int((listed & ~keep).sum())


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
