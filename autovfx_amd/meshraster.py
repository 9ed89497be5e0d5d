"""A z-buffer over triangle meshes on the GPU: the forward of pytorch3d's ``_C.rasterize_meshes`` at ``blur_radius == 0``.

SuGaR's coarse mesh extraction rasterizes its splatted diamond mesh once per training camera (``sugar_extractors/coarse_mesh.py:216-227``
builds the ``MeshRasterizer`` with ``faces_per_pixel=10``; ``sugar_scene/sugar_model.py:1341``, ``:1568``, ``:1798`` call it, the texture
extraction at ``:2541-2598`` and ``metrics.py:283-290`` with ``faces_per_pixel=1``).  Underneath sits ``pytorch3d._C.rasterize_meshes``, a
CUDA kernel that a pytorch3d built against torch-ROCm does not have.  :func:`rasterize_face_verts` runs the HIP kernels of
``gsr_meshraster.hip`` (C ABI ``gsr_mesh_raster_count``, ``gsr_mesh_raster``) behind that argument list; :func:`drop_in` is what
``autovfx_amd.install()`` puts in place of pytorch3d's operator; :func:`rasterize_face_verts_host` restates the contract in numpy.

The contract is pytorch3d's published forward kernel as recalled, pinned here; the tests hold the code to this text.

**Inputs.**  ``face_verts [F, 3, 3]`` float32, finite: x, y in NDC with +x left and +y up, z the view depth.  ``mesh_to_face_first_idx [N]``,
``num_faces_per_mesh [N]``, ``clipped_faces_neighbor_idx [F]`` int64.  ``image_size = (H, W)``, ``blur_radius``, ``faces_per_pixel`` K,
``bin_size``, ``max_faces_per_bin``, ``perspective_correct``, ``clip_barycentric_coords``, ``cull_backfaces``.  Face f belongs to the lowest
mesh n with ``first[n] <= f < first[n] + num[n]`` (the ranges of a packed batch do not overlap) and lands only in image n; a face in no
range lands nowhere.

**Outputs.**  ``pix_to_face [N, H, W, K]`` int64 (the packed face index), ``zbuf [N, H, W, K]``, ``bary_coords [N, H, W, K, 3]``,
``dists [N, H, W, K]`` float32.  An empty slot holds -1 in all four.

**Pixel centre.**  Output row r, column c has ``x = ndc(W - 1 - c, W, H)``, ``y = ndc(H - 1 - r, H, W)`` with
``ndc(i, S1, S2) = -off + (range * i + off) / S1``, ``range = (2 * S1) / S2 if S1 > S2 else 2``, ``off = range / 2``.

**Per face**, every operation an fp32 one in the order written, nothing contracted; ``eps = 1e-8``,
``edge(p, a, b) = (p.x - a.x) * (b.y - a.y) - (p.y - a.y) * (b.x - a.x)``.  The face is skipped when

* ``max(z0, z1, z2) < eps``, or ``|edge(v0, v1, v2)| <= eps``, or ``cull_backfaces`` and ``edge(v0, v1, v2) < 0``;
* the pixel lies outside the xy bounding box: ``x < xmin or x > xmax or y < ymin or y > ymax``.

Otherwise ``w = (edge(p, v1, v2), edge(p, v2, v0), edge(p, v0, v1))``, each divided by ``edge(v2, v0, v1) + eps``;
``inside = w0 > 0 and w1 > 0 and w2 > 0`` (strict).  ``b = w``; with ``perspective_correct``
``t = ((w0 * z1) * z2, (z0 * w1) * z2, (z0 * z1) * w2)`` and ``b = t / max((t0 + t1) + t2, eps)``; then with ``clip_barycentric_coords``
``c_i = max(0, min(1, b_i))`` and ``b = c / max((c0 + c1) + c2, 1e-5)``.  ``pz = (b0 * z0 + b1 * z1) + b2 * z2``; the face is skipped when
``pz < 0``.  ``dist = min(d(v0, v1), min(d(v0, v2), d(v1, v2)))`` with the squared distance to a segment
``d(a, b)``: ``u = b - a``, ``l2 = u.x * u.x + u.y * u.y``; if ``l2 <= eps`` it is ``|p - b|^2``; else ``t = (u.x * (p.x - a.x) + u.y * (p.y - a.y)) / l2``,
``q = a + min(max(t, 0), 1) * u`` and it is ``|p - q|^2`` (``|e|^2 = e.x * e.x + e.y * e.y``).  With ``blur_radius == 0`` only ``inside`` pixels
are kept; they carry ``zbuf = pz``, ``bary_coords = b``, ``dists = -dist``.

**Overflow.**  Every finite input is admitted, and huge finite coordinates overflow the intermediates to infinities and, through
``inf - inf`` and ``inf / inf``, to NaN.  Every ``min`` and ``max`` above is C's ``fminf`` / ``fmaxf`` (numpy's ``fmin`` / ``fmax``, not its
``minimum`` / ``maximum``): of a NaN and a number the number is returned, a NaN operand loses, so ``max(NaN, eps) = eps``,
``max(0, min(1, NaN)) = 1`` and ``min(max(NaN, 0), 1) = 0``.  Every comparison with a NaN is false: a NaN ``w`` is not inside, a NaN ``pz`` is
not ``< 0`` (the face counts as kept for a neighbour that names it) but orders before nothing, so such a face is never listed; a kept face
with ``pz = +inf`` is listed behind every finite depth, the lower index first.  A face with a NaN or infinite coordinate is outside the
contract: what that face itself receives, and whether it is listed, is unspecified; the code only promises that it finishes and that the
finite faces of every pixel come out among each other as if it were not there, as far as the K slots it may occupy leave room.

**Per pixel.**  The K kept faces smallest in ``(pz, packed face index)`` order, compared lexicographically, ascending: the result does not
depend on the order the faces are visited in.  pytorch3d leaves equal depths in whatever order its bins produced; here the lower face
index comes first (difference 1).  The neighbour rule: a kept face f with ``g = clipped_faces_neighbor_idx[f] >= 0``, g another face of the
same mesh, gives way when g is kept at the pixel too (by the rules above) and ``dist_g < dist_f``, or ``dist_g == dist_f`` and ``g < f``.
pytorch3d's ``clip_faces`` makes the two parts of a clipped triangle name each other, so of such a pair exactly one stays, the one nearer to
its own edges, as in pytorch3d's "already listed" test; stated like this the rule needs no visiting order either.

``bin_size`` and ``max_faces_per_bin`` are accepted and ignored: a tile's list has no maximum length and nothing is ever dropped, where
pytorch3d drops the faces of a bin past ``max_faces_per_bin`` with a warning (difference 2).

The backward stays pytorch3d's: a call whose ``face_verts`` requires a gradient is not taken.
"""
from __future__ import annotations

import ctypes
from typing import Callable, Optional, Tuple

import numpy as np
import torch

from . import _takes

MAX_K = 16
MAX_SIDE = 16384
MAX_FACES = (1 << 31) - 2
_F = np.float32
EPS = _F(1e-8)
BARY_CLIP_EPS = _F(1e-5)


class TooManyPairs(ValueError):
    """The tile lists of a call would hold 2^31 entries or more; only known once the count kernel has run."""


def _image_size(image_size) -> Optional[Tuple[int, int]]:
    try:
        h, w = image_size
    except (TypeError, ValueError):
        return None
    if type(h) is not int or type(w) is not int:
        return None
    return h, w


def _why_not(face_verts, mesh_to_face_first_idx, num_faces_per_mesh, clipped_faces_neighbor_idx, image_size, blur_radius,
             faces_per_pixel) -> Optional[str]:
    """None when the kernels take the call, else the reason they do not."""
    index = (("mesh_to_face_first_idx", mesh_to_face_first_idx, torch.int64), ("num_faces_per_mesh", num_faces_per_mesh, torch.int64),
             ("clipped_faces_neighbor_idx", clipped_faces_neighbor_idx, torch.int64))
    why = (_takes.tensors((("face_verts", face_verts, torch.float32),) + index, host="rasterize_face_verts_host")
           or _takes.shaped("face_verts", face_verts, "[F, 3, 3]", face_verts.dim() == 3 and tuple(face_verts.shape[1:]) == (3, 3)))
    if why is not None:
        return why
    if not face_verts.is_contiguous():
        return "face_verts must be contiguous"
    if face_verts.shape[0] > MAX_FACES:
        return f"{face_verts.shape[0]} faces: at most 2^31 - 2"
    for name, t, _ in index:
        if t.dim() != 1 or not t.is_contiguous():
            return _takes.shaped(name, t, "contiguous and 1-D", False)
    if mesh_to_face_first_idx.shape[0] != num_faces_per_mesh.shape[0]:
        return f"mesh_to_face_first_idx and num_faces_per_mesh must have one length (got {mesh_to_face_first_idx.shape[0]} and {num_faces_per_mesh.shape[0]})"
    if clipped_faces_neighbor_idx.shape[0] != face_verts.shape[0]:
        return f"clipped_faces_neighbor_idx must have one entry per face (got {clipped_faces_neighbor_idx.shape[0]} for {face_verts.shape[0]} faces)"
    size = _image_size(image_size)
    if size is None or not all(1 <= s <= MAX_SIDE for s in size):
        return f"image_size must be (H, W), two ints in 1..{MAX_SIDE} (got {image_size!r})"
    if isinstance(blur_radius, bool) or not isinstance(blur_radius, (int, float)) or blur_radius != 0.0:
        return f"blur_radius must be 0.0 (got {blur_radius!r})"
    if type(faces_per_pixel) is not int or not 1 <= faces_per_pixel <= MAX_K:
        return f"faces_per_pixel must be an int in 1..{MAX_K} (got {faces_per_pixel!r})"
    if face_verts.requires_grad:   # (also inside pytorch3d's autograd.Function.forward, where the operator is called with grad mode off)
        return "face_verts requires a gradient (the backward stays pytorch3d's, which needs its own forward)"
    return _takes.capturing("the call reads the pair total back and allocates its scratch")


def rasterize_takes(face_verts, mesh_to_face_first_idx, num_faces_per_mesh, clipped_faces_neighbor_idx, image_size, blur_radius,
                    faces_per_pixel, bin_size=None, max_faces_per_bin=None, perspective_correct=False, clip_barycentric_coords=False,
                    cull_backfaces=False) -> bool:
    """Whether :func:`rasterize_face_verts` runs this call: CUDA float32 contiguous ``[F, 3, 3]`` faces that need no gradient, contiguous
    1-D int64 index tensors on the same device (``[N]``, ``[N]``, ``[F]``), ``image_size`` two ints in 1..16384, ``blur_radius == 0.0``,
    ``1 <= faces_per_pixel <= 16``, not under graph capture."""
    return _why_not(face_verts, mesh_to_face_first_idx, num_faces_per_mesh, clipped_faces_neighbor_idx, image_size, blur_radius,
                    faces_per_pixel) is None


def _taken(face_verts, first_idx, num_faces, neighbours, image_size, K: int, perspective_correct, clip_barycentric_coords, cull_backfaces):
    """A call ``_why_not`` let through."""
    from . import _lib

    fv = face_verts.detach()
    dev = fv.device
    F, N = int(fv.shape[0]), int(first_idx.shape[0])
    H, W = image_size
    flags = (int(bool(perspective_correct)), int(bool(clip_barycentric_coords)), int(bool(cull_backfaces)))
    pix_to_face = torch.empty((N, H, W, K), dtype=torch.int64, device=dev)
    zbuf = torch.empty((N, H, W, K), dtype=torch.float32, device=dev)
    bary = torch.empty((N, H, W, K, 3), dtype=torch.float32, device=dev)
    dists = torch.empty((N, H, W, K), dtype=torch.float32, device=dev)
    if N == 0:
        return pix_to_face, zbuf, bary, dists
    outputs = (pix_to_face.data_ptr(), zbuf.data_ptr(), bary.data_ptr(), dists.data_ptr())
    with torch.cuda.device(dev):
        if F == 0:
            _lib.call("gsr_mesh_raster", 0, N, None, None, None, None, H, W, 0.0, K, *flags, None, 0, 0, None, 0, *outputs, device=dev)
            return pix_to_face, zbuf, bary, dists
        plan, plan_bytes = _lib.scratch("gsr_mesh_raster_plan_bytes", F, N, H, W, device=dev)
        total = ctypes.c_int64(0)
        _lib.call("gsr_mesh_raster_count", F, N, fv.data_ptr(), first_idx.data_ptr(), num_faces.data_ptr(), H, W, flags[2], plan.data_ptr(),
                  plan_bytes, ctypes.byref(total), device=dev)           # (the one host read of the call)
        if total.value >= 1 << 31:
            raise TooManyPairs(f"rasterize_meshes: {total.value} (tile, face) pairs, at most 2^31 - 1 (faces times the 16x16 tiles each touches)")
        pairs, pair_bytes = _lib.scratch("gsr_mesh_raster_pair_bytes", total.value, device=dev)
        _lib.call("gsr_mesh_raster", F, N, fv.data_ptr(), first_idx.data_ptr(), num_faces.data_ptr(), neighbours.data_ptr(), H, W, 0.0, K,
                  *flags, plan.data_ptr(), plan_bytes, total.value, pairs.data_ptr(), pair_bytes, *outputs, device=dev)
    return pix_to_face, zbuf, bary, dists


def rasterize_face_verts(face_verts, mesh_to_face_first_idx, num_faces_per_mesh, clipped_faces_neighbor_idx, image_size, blur_radius,
                         faces_per_pixel, bin_size=None, max_faces_per_bin=None, perspective_correct=False, clip_barycentric_coords=False,
                         cull_backfaces=False):
    """``pytorch3d._C.rasterize_meshes`` (its positional order) -> ``(pix_to_face, zbuf, bary_coords, dists)`` by the module's contract,
    queued on the current stream; the call waits once for the device (the total length of the tile lists sizes its scratch).
    ``bin_size`` and ``max_faces_per_bin`` are ignored.  A call :func:`rasterize_takes` rejects raises ``ValueError`` with the reason, and so does
    one whose tile lists would hold 2^31 entries or more (:class:`TooManyPairs`, after the count step)."""
    _takes.refuse("rasterize_meshes", _why_not(face_verts, mesh_to_face_first_idx, num_faces_per_mesh, clipped_faces_neighbor_idx, image_size,
                                               blur_radius, faces_per_pixel))
    return _taken(face_verts, mesh_to_face_first_idx, num_faces_per_mesh, clipped_faces_neighbor_idx, _image_size(image_size), faces_per_pixel,
                  perspective_correct, clip_barycentric_coords, cull_backfaces)


def drop_in(original: Callable) -> Callable:
    """A ``rasterize_meshes`` that runs the kernels for the calls :func:`rasterize_takes` accepts and ``original`` (pytorch3d's operator,
    same positional arguments) for every other: CPU tensors, ``blur_radius > 0``, more than 16 faces per pixel, faces that need a gradient,
    graph capture, and a call whose tile lists turn out to need 2^31 entries or more (:class:`TooManyPairs`, found by the count step).
    ``autovfx_amd.install()`` builds it around ``pytorch3d._C.rasterize_meshes``; pytorch3d's Python looks the operator up on ``_C`` at every
    call, so its ``clip_faces``, bin heuristics and ``convert_clipped_rasterization_to_original_faces`` run as they are around it."""
    def rasterize_meshes_drop_in(face_verts, mesh_to_face_first_idx, num_faces_per_mesh, clipped_faces_neighbor_idx, image_size, blur_radius,
                                 faces_per_pixel, bin_size, max_faces_per_bin, perspective_correct, clip_barycentric_coords, cull_backfaces):
        if _why_not(face_verts, mesh_to_face_first_idx, num_faces_per_mesh, clipped_faces_neighbor_idx, image_size, blur_radius,
                    faces_per_pixel) is None:
            try:
                return _taken(face_verts, mesh_to_face_first_idx, num_faces_per_mesh, clipped_faces_neighbor_idx, _image_size(image_size),
                              faces_per_pixel, perspective_correct, clip_barycentric_coords, cull_backfaces)
            except TooManyPairs:      # known only after the count: nothing has been written yet, the call is the original's after all
                pass
        return original(face_verts, mesh_to_face_first_idx, num_faces_per_mesh, clipped_faces_neighbor_idx, image_size, blur_radius,
                        faces_per_pixel, bin_size, max_faces_per_bin, perspective_correct, clip_barycentric_coords, cull_backfaces)

    return _takes.dressed(rasterize_meshes_drop_in, "rasterize_meshes", original, "pytorch3d._C.rasterize_meshes", "meshraster")


# ---- the contract in numpy ------------------------------------------------------------------------------------------------------------

def _ndc(i: np.ndarray, S1: int, S2: int) -> np.ndarray:
    rng = (_F(2.0) * _F(S1)) / _F(S2) if S1 > S2 else _F(2.0)
    off = rng / _F(2.0)
    return -off + (rng * i.astype(_F) + off) / _F(S1)


def _edge(px, py, ax, ay, bx, by):
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax)


def _segment_dist2(px, py, ax, ay, bx, by):
    dx, dy = bx - ax, by - ay
    l2 = dx * dx + dy * dy
    ex, ey = px - bx, py - by
    at_end = ex * ex + ey * ey
    t = (dx * (px - ax) + dy * (py - ay)) / l2
    tt = np.fmin(np.fmax(t, _F(0.0)), _F(1.0))
    qx, qy = ax + tt * dx, ay + tt * dy
    ex, ey = px - qx, py - qy
    return np.where(l2 <= EPS, at_end, ex * ex + ey * ey)


def rasterize_face_verts_host(face_verts, mesh_to_face_first_idx, num_faces_per_mesh, clipped_faces_neighbor_idx, image_size, blur_radius,
                              faces_per_pixel, bin_size=None, max_faces_per_bin=None, perspective_correct=False,
                              clip_barycentric_coords=False, cull_backfaces=False, chunk_elems: int = 1 << 21):
    """The module's contract restated in numpy: every operation an fp32 elementwise one in the contract's order (no fused multiply-add),
    brute force over all faces of a mesh for a chunk of pixels at a time, a stable sort on ``pz`` over the faces in index order.  Arguments
    as :func:`rasterize_face_verts`, anything ``np.asarray`` takes; ``blur_radius`` must be 0.  Returns the four arrays."""
    if blur_radius != 0.0:
        raise ValueError(f"blur_radius must be 0.0 (got {blur_radius!r})")
    fv = np.ascontiguousarray(np.asarray(face_verts, dtype=_F).reshape(-1, 3, 3))
    first = np.asarray(mesh_to_face_first_idx, dtype=np.int64).reshape(-1)
    count = np.asarray(num_faces_per_mesh, dtype=np.int64).reshape(-1)
    nbr = np.asarray(clipped_faces_neighbor_idx, dtype=np.int64).reshape(-1)
    H, W = image_size
    K, F, N = int(faces_per_pixel), fv.shape[0], first.shape[0]
    pix_to_face = np.full((N, H * W, K), -1, np.int64)
    zbuf = np.full((N, H * W, K), -1, _F)
    bary = np.full((N, H * W, K, 3), -1, _F)
    dists = np.full((N, H * W, K), -1, _F)
    shape = lambda a, *tail: a.reshape(N, H, W, K, *tail)
    if F == 0 or N == 0:
        return shape(pix_to_face), shape(zbuf), shape(bary, 3), shape(dists)

    x0, y0, z0, x1, y1, z1, x2, y2, z2 = (fv[:, i, j] for i in range(3) for j in range(3))
    with np.errstate(all="ignore"):
        area = _edge(x0, y0, x1, y1, x2, y2)
        culled = (np.fmax(z0, np.fmax(z1, z2)) < EPS) | (np.abs(area) <= EPS)
        if cull_backfaces:
            culled |= area < _F(0.0)
    mesh_of = np.full(F, -1, np.int64)
    for n in range(N - 1, -1, -1):                                   # the lowest mesh whose range holds the face wins
        mesh_of[max(int(first[n]), 0):max(int(first[n]) + int(count[n]), 0)] = n
    cols = _ndc(W - 1 - np.arange(W), W, H)
    rows = _ndc(H - 1 - np.arange(H), H, W)
    px_all = np.broadcast_to(cols[None, :], (H, W)).reshape(-1, 1)
    py_all = np.broadcast_to(rows[:, None], (H, W)).reshape(-1, 1)

    for n in range(N):
        idx = np.nonzero((mesh_of == n) & ~culled)[0]
        if idx.size == 0:
            continue
        ax, ay, az, bx, by, bz, cx, cy, cz = (v[idx][None, :] for v in (x0, y0, z0, x1, y1, z1, x2, y2, z2))
        with np.errstate(all="ignore"):
            denom = _edge(cx, cy, ax, ay, bx, by) + EPS
        xmin, xmax = np.fmin(ax, np.fmin(bx, cx)), np.fmax(ax, np.fmax(bx, cx))
        ymin, ymax = np.fmin(ay, np.fmin(by, cy)), np.fmax(ay, np.fmax(by, cy))
        # the neighbour of every listed face as a column of this mesh's list (-1: none, culled, itself or in another mesh)
        column_of = np.full(F, -1, np.int64)
        column_of[idx] = np.arange(idx.size)
        g = nbr[idx]
        g_ok = (g >= 0) & (g < F) & (g != idx)
        g_col = np.where(g_ok, column_of[np.clip(g, 0, F - 1)], -1)
        has_g = np.nonzero(g_col >= 0)[0]
        step = max(1, chunk_elems // idx.size)
        for a in range(0, H * W, step):
            b = min(H * W, a + step)
            px, py = px_all[a:b], py_all[a:b]
            with np.errstate(all="ignore"):
                outside = (px < xmin) | (px > xmax) | (py < ymin) | (py > ymax)
                w0 = _edge(px, py, bx, by, cx, cy) / denom
                w1 = _edge(px, py, cx, cy, ax, ay) / denom
                w2 = _edge(px, py, ax, ay, bx, by) / denom
                inside = (w0 > _F(0.0)) & (w1 > _F(0.0)) & (w2 > _F(0.0))
                b0, b1, b2 = w0, w1, w2
                if perspective_correct:
                    t0, t1, t2 = (w0 * bz) * cz, (az * w1) * cz, (az * bz) * w2
                    d = np.fmax((t0 + t1) + t2, EPS)
                    b0, b1, b2 = t0 / d, t1 / d, t2 / d
                if clip_barycentric_coords:
                    c0, c1, c2 = (np.fmax(_F(0.0), np.fmin(_F(1.0), v)) for v in (b0, b1, b2))
                    d = np.fmax((c0 + c1) + c2, BARY_CLIP_EPS)
                    b0, b1, b2 = c0 / d, c1 / d, c2 / d
                pz = (b0 * az + b1 * bz) + b2 * cz
                kept = ~outside & inside & ~(pz < _F(0.0))
                dist = np.fmin(_segment_dist2(px, py, ax, ay, bx, by),
                               np.fmin(_segment_dist2(px, py, ax, ay, cx, cy), _segment_dist2(px, py, bx, by, cx, cy)))
            final = kept & ~np.isnan(pz)                             # a NaN depth is nearer than nothing: never listed (a neighbour still sees it kept)
            if has_g.size:                                           # the neighbour rule, on the faces that name a listed one
                theirs, mine = dist[:, g_col[has_g]], dist[:, has_g]
                gives_way = kept[:, g_col[has_g]] & ((theirs < mine) | ((theirs == mine) & (idx[g_col[has_g]] < idx[has_g])[None, :]))
                final[:, has_g] &= ~gives_way
            key = np.where(final, pz, _F(np.nan))                    # numpy sorts NaN behind +inf: a listed face of infinite depth comes before the unlisted
            order = np.argsort(key, axis=1, kind="stable")[:, :K]   # the faces are in index order: equal depths go by the lower index
            k = order.shape[1]
            found = np.take_along_axis(final, order, axis=1)
            take = lambda v: np.take_along_axis(np.broadcast_to(v, final.shape), order, axis=1)
            pix_to_face[n, a:b, :k] = np.where(found, idx[order], -1)
            zbuf[n, a:b, :k] = np.where(found, take(pz), _F(-1.0))
            dists[n, a:b, :k] = np.where(found, -take(dist), _F(-1.0))
            for i, v in enumerate((b0, b1, b2)):
                bary[n, a:b, :k, i] = np.where(found, take(v), _F(-1.0))
    return shape(pix_to_face), shape(zbuf), shape(bary, 3), shape(dists)
