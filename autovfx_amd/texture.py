"""The texture of SuGaR's refined mesh, baked on the GPU: ``extract_texture_image_and_uv_from_gaussians``
(``sugar/sugar_scene/sugar_model.py:2398-2614``, called by ``sugar_extractors/refined_mesh.py:195``).

The reference gives every pair of faces an ``S x S`` square of a ``T x T`` atlas (``T = S A``), fills each face's texels from the
nearest of the face's Gaussians, and then, per training camera, renders the Gaussians, rasterizes the mesh, runs pytorch3d's whole
``SoftPhongShader`` over an index map only to learn which texel each pixel sees, and scatters the colours with six boolean-mask
``index_put``s.  Here :func:`atlas` builds the UV layout and two small tables with the reference's values, :func:`fill` is one pass
over (face, texel of the face), and :func:`bake_view` is two launches per camera over the rasterizer's fragments (C ABI
``gsr_texture_fill``, ``gsr_texture_bake_view``, ``gsr_texture_texels`` in ``gsr_texture.hip``).  The contract,
plain fp32 in the order written, nothing contracted, division correctly rounded:

**The atlas** (``:2420-2424``, ``:2436-2469``, ``:2476-2514``).  ``A = int(sqrt(F // 2 + 1) + 1)``, ``T = S A``.  Square ``s`` sits at
``(a, b) = (s // A, s % A)`` and holds faces ``2 s`` ("bottom") and ``2 s + 1`` ("top").  ``verts_uv [6 A A, 2]``: rows ``6 s .. 6 s + 5``
are ``S (a + 1, b) + (-2, 1)``, ``S (a, b) + (2, 1)``, ``S (a + 1, b + 1) + (-2, -3)``, ``S (a, b + 1) + (1, -1)``, ``S (a, b) + (1, 3)``,
``S (a + 1, b + 1) + (-3, -1)``, each divided by ``T``; ``faces_uv = arange(3 F).view(F, 3)``.  ``texel_offset [2, n, 2]`` int32,
``n = S (S - 1) / 2``: row 0 the ``(i, j)`` with ``0 <= j <= i <= S - 2``, row 1 those with ``0 <= i < j <= S - 1``, ``i`` outermost.
``texel_bary [2, n, 3]``: with ``(c_0, c_1) = (S - 2 - i, j - 1) / (S - 3)`` in row 0 and ``(i - 1, S - 1 - j) / (S - 3)`` in row 1 it
is ``(1 - (c_0 + c_1), c_0, c_1)``.  (The tables' unit barycentrics sit one texel off the UV corners, and row 1 weighs the face's
second and third vertices where the UV layout has the third and second: the reference's values, kept.)

**A pixel's texel** (``TexturesUV.sample_textures`` with ``align_corners=True``, ``padding_mode="border"``, ``sampling_mode="nearest"``
on the flipped map, as recalled; this text is the contract).  Pixel ``p`` with ``f = pix_to_face[p]`` is valid iff ``0 <= f < F`` and
``zbuf[p] > 0`` (a NaN ``zbuf`` is invalid).  Then for ``c = 0, 1``: ``uv_c = (b_0 uv[f,0,c] + b_1 uv[f,1,c]) + b_2 uv[f,2,c]``;
``g_c = uv_c * 2 - 1``; ``x_c = ((g_c + 1) / 2) * (T - 1)``, a NaN ``x_c`` makes the pixel invalid;
``i_c = rintf(fminf(T - 1, fmaxf(x_c, 0)))`` (half to even); the texel is ``(row, col) = (T - 1 - i_1, i_0)``.

**One view.**  *claim*: every valid pixel does ``atomicMin(owner[texel], p)`` on a ``[T T]`` buffer of 32-bit words that holds
``0xFFFFFFFF`` everywhere (an int32 tensor of ``-1``, :func:`new_owner`).  *accumulate*: the pixel that finds its own index there writes
``tex[texel] = rgb[p] if count[texel] == 0 else tex[texel] + rgb[p]``, ``count[texel] += 1`` and ``0xFFFFFFFF`` back; the others read
the winner's index or ``0xFFFFFFFF``, never their own, so the buffer is clean for the next view.  No host read, no float atomics:
the sum runs in camera order and is the same bits on every run.  Limits: ``H W <= 2^32 - 2``, ``T T < 2^31``.

**The fill** (``:2473-2539``).  For face ``f`` and texel ``t`` of its table (row ``f & 1``): ``x = (bary_0 v_0 + bary_1 v_1) + bary_2 v_2``;
per Gaussian ``g < G`` of the face ``q_g`` is the density field's ``q`` (field.py: ``s = x - c``, ``w = M^T s``, the square sum, the
clamp to ``[0, 1e8]``); the first NaN ``q``, else the first smallest, chooses ``g``; ``features[f G + g] * 0.28209479177387814f + 0.5f``
goes to texel ``(T - 1 - (b S + o_1), a S + o_0)`` (the reference's ``transpose(0, 1).flip(0)``).  Texels no face owns are ``0.5``.
``1 <= G <= 8``, ``4 <= S <= 32``.  A face with a vertex index outside ``[0, V)`` writes nothing.

**Stated differences from the reference.**

1. Among several pixels of one camera on one texel the lowest pixel index is taken; the reference's ``index_put`` with repeated indices
   leaves that open.
2. The shader's soft blend is not applied.  It is the identity after ``.round()`` unless ``zbuf`` is within about 0.12 % of ``zfar`` or
   beyond it (with ``zfar = 100`` and ``T <= 32768``: from about 99.88), where the reference sends the pixel's colour to a lower,
   unrelated texel.  Here such a pixel votes for its own texel.
3. The fill picks the smallest ``q``; the reference picks the largest ``exp(-q / 2)``, so Gaussians whose weights round equal or
   underflow to 0 go to index 0.  It matters only for texels no camera sees.
4. A non-finite initial value is dropped on a texel's first visit, where the reference's ``0 * x`` keeps NaN.
5. Faces with a vertex index outside ``[0, V)`` are skipped by the fill.

:func:`atlas_host`, :func:`fill_host`, :func:`texels_of_pixels_host` and :func:`bake_view_host` restate the contract in numpy fp32, the
checkers of the tests; :func:`drop_in` is what ``autovfx_amd.install()`` puts in the reference's module.
"""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np
import torch

from . import _mesh_host, _takes

MAX_G = 8
MIN_S, MAX_S = 4, 32
MAX_T = 46340                     # T * T < 2^31
MAX_PIXELS = (1 << 32) - 2
MAX_FACES = (1 << 28) - 1
SH_C0 = 0.28209479177387814
Q_MAX = 1e8
_F = np.float32

# per corner of a square's six UV vertices: which corner of the square, and the shift in texels (:2454-2468)
_CORNER = ((1, 0), (0, 0), (1, 1), (0, 1), (0, 0), (1, 1))
_SHIFT = ((-2, 1), (2, 1), (-2, -3), (1, -1), (1, 3), (-3, -1))


def squares_per_axis(n_faces: int) -> int:
    return int(np.sqrt(n_faces // 2 + 1) + 1)


def _table_offsets(S: int) -> np.ndarray:
    bottom = [(i, j) for i in range(S - 1) for j in range(i + 1)]
    top = [(i, j) for i in range(S) for j in range(i + 1, S)]
    return np.asarray([bottom, top], np.int32)


# ---- the atlas ----
def atlas(n_faces: int, square_size: int, device):
    """``(verts_uv [6 A A, 2] fp32, faces_uv [F, 3] int64, texture_size, A, texel_offset [2, n, 2] int32, texel_bary [2, n, 3] fp32)``
    on ``device``, the reference's values (module docstring)."""
    F, S = int(n_faces), int(square_size)
    if F < 0 or not MIN_S <= S <= MAX_S:
        raise ValueError(f"atlas: n_faces = {F}, square_size = {S} (n_faces >= 0, square_size in {MIN_S}..{MAX_S})")
    A = squares_per_axis(F)
    T = S * A
    if T > MAX_T:
        raise ValueError(f"atlas: texture_size {T} exceeds {MAX_T}")
    grid = torch.cartesian_prod(torch.arange(A, device=device), torch.arange(A, device=device))            # [A A, 2] int64: (a, b)
    corner = torch.tensor(_CORNER, dtype=torch.int64, device=device)
    shift = torch.tensor(_SHIFT, dtype=torch.int64, device=device)
    verts_uv = ((grid[:, None, :] + corner[None]) * S + shift[None]).reshape(-1, 2) / T                     # int64 / int: fp32 division
    faces_uv = torch.arange(3 * F, device=device).view(F, 3)
    offs = torch.from_numpy(_table_offsets(S)).to(device)
    ij = offs.float()
    c = torch.stack([torch.stack([-(ij[0, :, 0] - (S - 2)), ij[0, :, 1] - 1], dim=-1),
                     torch.stack([ij[1, :, 0] - 1, -(ij[1, :, 1] - (S - 1))], dim=-1)]) / (S - 3)
    bary = torch.cat([1.0 - c.sum(dim=-1, keepdim=True), c], dim=-1)
    return verts_uv, faces_uv, T, A, offs.contiguous(), bary.contiguous()


def atlas_host(n_faces: int, square_size: int):
    """:func:`atlas` in numpy."""
    F, S = int(n_faces), int(square_size)
    A = squares_per_axis(F)
    T = S * A
    a, b = np.divmod(np.arange(A * A, dtype=np.int64), A)
    grid = np.stack([a, b], axis=-1)
    texels = (grid[:, None, :] + np.asarray(_CORNER, np.int64)[None]) * S + np.asarray(_SHIFT, np.int64)[None]
    verts_uv = texels.reshape(-1, 2).astype(_F) / _F(T)
    faces_uv = np.arange(3 * F, dtype=np.int64).reshape(F, 3)
    offs = _table_offsets(S)
    ij = offs.astype(_F)
    c = np.stack([np.stack([-(ij[0, :, 0] - _F(S - 2)), ij[0, :, 1] - _F(1)], axis=-1),
                  np.stack([ij[1, :, 0] - _F(1), -(ij[1, :, 1] - _F(S - 1))], axis=-1)]) / _F(S - 3)
    bary = np.concatenate([_F(1) - (c[..., 0:1] + c[..., 1:2]), c], axis=-1).astype(_F)
    return verts_uv, faces_uv, T, A, offs, bary


# ---- the contract in numpy ----
def texels_of_pixels_host(pix_to_face, bary, zbuf, face_uvs, texture_size: int) -> np.ndarray:
    """``[P]`` int32: ``row * T + col`` of the texel each pixel sees, -1 for an invalid pixel."""
    pix = np.asarray(pix_to_face, np.int64).reshape(-1)
    w = np.asarray(bary, _F).reshape(-1, 3)
    z = np.asarray(zbuf, _F).reshape(-1)
    uv = np.asarray(face_uvs, _F).reshape(-1, 3, 2)
    T = int(texture_size)
    last = _F(T - 1)
    with np.errstate(over="ignore", invalid="ignore"):
        valid = (pix >= 0) & (pix < uv.shape[0]) & (z > 0)
        u = uv[np.where(valid, pix, 0)] if uv.shape[0] else np.zeros((pix.shape[0], 3, 2), _F)
        ic = []
        for c in range(2):
            uvc = (w[:, 0] * u[:, 0, c] + w[:, 1] * u[:, 1, c]) + w[:, 2] * u[:, 2, c]
            g = uvc * _F(2) - _F(1)
            x = ((g + _F(1)) / _F(2)) * last
            valid = valid & ~np.isnan(x)
            ic.append(np.rint(np.fmin(last, np.fmax(np.where(np.isnan(x), _F(0), x), _F(0)))).astype(np.int64))
    return np.where(valid, (T - 1 - ic[1]) * T + ic[0], -1).astype(np.int32)


def bake_view_host(tex, count, rgb, pix_to_face, bary, zbuf, face_uvs):
    """One view into copies of ``tex [T, T, 3]`` and ``count [T, T]``: ``(tex, count)``."""
    tex = np.array(tex, _F)
    T = tex.shape[0]
    tex = tex.reshape(T * T, 3)
    count = np.array(count, _F).reshape(T * T)
    colours = np.asarray(rgb, _F).reshape(-1, 3)
    texel = texels_of_pixels_host(pix_to_face, bary, zbuf, face_uvs, T)
    seen = np.nonzero(texel >= 0)[0]
    hit, first = np.unique(texel[seen], return_index=True)      # (seen ascends: the first occurrence is the lowest pixel)
    winner = seen[first]
    fresh = count[hit] == 0
    with np.errstate(over="ignore", invalid="ignore"):
        tex[hit] = np.where(fresh[:, None], colours[winner], tex[hit] + colours[winner])
        count[hit] = count[hit] + _F(1)
    return tex.reshape(T, T, 3), count.reshape(T, T)


def _q_host(x, centers, M):
    """``q [..., G]`` of points ``x [..., 1, 3]`` against ``centers [..., G, 3]``, ``M [..., G, 3, 3]``: field.py's order."""
    s = x - centers
    w = (M[..., 0, :] * s[..., 0:1] + M[..., 1, :] * s[..., 1:2]) + M[..., 2, :] * s[..., 2:3]
    q = (w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1]) + w[..., 2] * w[..., 2]
    return np.where(q < 0, _F(0), np.where(q > _F(Q_MAX), _F(Q_MAX), q))


def fill_host(verts, faces, centers, inv_scaled_rot, features, texel_offset, texel_bary, A: int, S: int, return_q: bool = False):
    """The initial atlas ``[T, T, 3]`` (with ``return_q`` also ``q [F, n, G]``)."""
    verts, faces = _mesh_host.verts_faces(verts, faces)
    F = faces.shape[0]
    offs = np.asarray(texel_offset, np.int32)
    bary = np.asarray(texel_bary, _F)
    n = offs.shape[1]
    G = np.asarray(centers).size // (3 * F) if F else 1
    c = np.asarray(centers, _F).reshape(F, 1, G, 3)
    M = np.asarray(inv_scaled_rot, _F).reshape(F, 1, G, 3, 3)
    feat = np.asarray(features, _F).reshape(F, G, 3)
    T = A * S
    tex = np.full((T, T, 3), _F(0.5), _F)
    ok, v0, v1, v2 = _mesh_host.face_corners(verts, faces)
    parity = np.arange(F) & 1
    w = bary[parity]                                                                   # [F, n, 3]
    with np.errstate(over="ignore", invalid="ignore"):
        x = (w[..., 0:1] * v0[:, None] + w[..., 1:2] * v1[:, None]) + w[..., 2:3] * v2[:, None]              # [F, n, 3]
        q = _q_host(x[:, :, None, :], c, M)                                            # [F, n, G]
        nan = np.isnan(q)
        best = np.where(nan.any(axis=-1), nan.argmax(axis=-1), np.where(nan, _F(np.inf), q).argmin(axis=-1))
        value = np.take_along_axis(feat[:, None], best[..., None, None], axis=2)[:, :, 0, :] * _F(SH_C0) + _F(0.5)
    sq = np.arange(F) >> 1
    a, b = sq // A, sq % A
    o = offs[parity]                                                                   # [F, n, 2]
    row = (T - 1) - (b[:, None] * S + o[..., 1])
    col = a[:, None] * S + o[..., 0]
    tex[row[ok], col[ok]] = value[ok]
    return (tex, q) if return_q else tex


# ---- the kernels ----
def new_owner(texture_size: int, device) -> torch.Tensor:
    """The claim buffer of :func:`bake_view`: ``[T T]`` 32-bit words of ``0xFFFFFFFF``, allocated once for all views."""
    return torch.full((int(texture_size) ** 2,), -1, dtype=torch.int32, device=device)


ALLOCATES = "the call allocates its outputs or copies of its inputs"


def _view_why_not(pix_to_face, bary, zbuf, face_uvs) -> Optional[str]:
    why = _takes.tensors((("pix_to_face", pix_to_face, torch.int64), ("bary", bary, torch.float32), ("zbuf", zbuf, torch.float32),
                          ("face_uvs", face_uvs, torch.float32)))
    if why is not None:
        return why
    P = pix_to_face.numel()
    if bary.dim() < 1 or bary.shape[-1] != 3 or bary.numel() != 3 * P:
        return f"bary must hold three values per pixel of pix_to_face {list(pix_to_face.shape)} (got {list(bary.shape)})"
    if zbuf.numel() != P:
        return f"zbuf must hold one value per pixel of pix_to_face {list(pix_to_face.shape)} (got {list(zbuf.shape)})"
    if face_uvs.dim() != 3 or tuple(face_uvs.shape[1:]) != (3, 2):
        return _takes.shaped("face_uvs", face_uvs, "[F, 3, 2]", False)
    if P > MAX_PIXELS:
        return f"{P} pixels: at most 2^32 - 2"
    return None


def texels_of_pixels(pix_to_face, bary, zbuf, face_uvs, texture_size: int) -> torch.Tensor:
    """int32, the shape of ``pix_to_face``: ``row * T + col`` of the texel each pixel sees, -1 for an invalid pixel.  On the current
    stream, no host synchronisation.  A call the kernel does not take raises ``ValueError`` with the reason."""
    why = _view_why_not(pix_to_face, bary, zbuf, face_uvs)
    if why is None and not (type(texture_size) is int and 1 <= texture_size <= MAX_T):
        why = f"texture_size must be an int in 1..{MAX_T} (got {texture_size!r})"
    _takes.refuse("texels_of_pixels", why or _takes.capturing(ALLOCATES))
    from . import _lib

    pix, w, z, uv = _takes.cs(pix_to_face, bary, zbuf, face_uvs)
    out = torch.empty(pix.shape, dtype=torch.int32, device=pix.device)
    with torch.cuda.device(pix.device):
        _lib.call("gsr_texture_texels", pix.numel(), uv.shape[0], texture_size, _lib.ptr(pix), _lib.ptr(w), _lib.ptr(z), _lib.ptr(uv),
                  _lib.ptr(out), device=pix.device)
    return out


def _pixel_rows(rgb: torch.Tensor):
    """``rgb [..., 3]`` as (tensor to keep alive, floats between two pixels): a ``[..., :3]`` view of a contiguous ``[..., C]`` image is
    taken as it is."""
    strides, shape = rgb.stride(), rgb.shape
    uniform = strides[-1] == 1 and all(strides[i] == strides[i + 1] * shape[i + 1] for i in range(rgb.dim() - 2))
    if rgb.dim() >= 2 and uniform and strides[-2] >= 3:
        return rgb, strides[-2]
    return rgb.contiguous(), 3


def bake_view(tex, count, owner, rgb, pix_to_face, bary, zbuf, face_uvs) -> None:
    """One camera into the atlas, in place: ``tex [T, T, 3]`` and ``count [T, T]`` (or ``[T, T, 1]``) fp32 contiguous, ``owner`` from
    :func:`new_owner`, ``rgb [..., 3]`` fp32 with one colour per pixel of ``pix_to_face`` (a ``[..., :3]`` view of an RGBA image is read in
    place), the rasterizer's fragments, ``face_uvs [F, 3, 2]``.  Two launches on the current stream, no host synchronisation.  A call the
    kernels do not take raises ``ValueError`` with the reason."""
    why = _view_why_not(pix_to_face, bary, zbuf, face_uvs)
    if why is None:
        why = _takes.tensors((("tex", tex, torch.float32), ("count", count, torch.float32), ("owner", owner, torch.int32),
                              ("rgb", rgb, torch.float32)), like=pix_to_face)
    if why is None:
        T = tex.shape[0] if tex.dim() == 3 else 0
        if tex.dim() != 3 or tuple(tex.shape) != (T, T, 3) or not 1 <= T <= MAX_T:
            why = f"tex must be [T, T, 3] with T in 1..{MAX_T} (got {list(tex.shape)})"
        elif tuple(count.shape) not in ((T, T), (T, T, 1)):
            why = f"count must be [T, T] or [T, T, 1] with T = {T} (got {list(count.shape)})"
        elif tuple(owner.shape) != (T * T,):
            why = f"owner must be [T * T] with T = {T} (got {list(owner.shape)})"
        elif not (tex.is_contiguous() and count.is_contiguous() and owner.is_contiguous()):
            why = "tex, count and owner are written in place and must be contiguous"
        elif rgb.dim() < 1 or rgb.shape[-1] != 3 or rgb.numel() != 3 * pix_to_face.numel():
            why = f"rgb must hold three values per pixel of pix_to_face {list(pix_to_face.shape)} (got {list(rgb.shape)})"
    _takes.refuse("bake_view", why or _takes.capturing(ALLOCATES))
    from . import _lib

    pix, w, z, uv = _takes.cs(pix_to_face, bary, zbuf, face_uvs)
    colours, stride = _pixel_rows(rgb.detach())
    with torch.cuda.device(pix.device):
        _lib.call("gsr_texture_bake_view", pix.numel(), uv.shape[0], T, _lib.ptr(pix), _lib.ptr(w), _lib.ptr(z), _lib.ptr(uv),
                  _lib.ptr(colours), stride, tex.data_ptr(), count.data_ptr(), owner.data_ptr(), device=pix.device)


def fill(verts, faces, centers, inv_scaled_rot, features, texel_offset, texel_bary, A: int, S: int) -> torch.Tensor:
    """The initial atlas ``[T, T, 3]``, ``T = A S``: ``verts [V, 3]``, ``faces [F, 3]`` int64, ``centers [F G, 3]``, ``inv_scaled_rot
    [F G, 3, 3]``, ``features [F G, 3]``, the two tables of :func:`atlas`.  On the current stream, no host synchronisation.  A call the
    kernels do not take raises ``ValueError`` with the reason."""
    why = _takes.mesh(verts, faces) or _takes.tensors((
        ("centers", centers, torch.float32), ("inv_scaled_rot", inv_scaled_rot, torch.float32), ("features", features, torch.float32),
        ("texel_offset", texel_offset, torch.int32), ("texel_bary", texel_bary, torch.float32)), like=verts)
    if why is None:
        F = faces.shape[0]
        n = texel_offset.shape[1] if texel_offset.dim() == 3 else 0
        G = centers.shape[0] // F if centers.dim() == 2 and F else 1
        if type(A) is not int or type(S) is not int or not MIN_S <= S <= MAX_S or A < 1 or A * S > MAX_T:
            why = f"A and S must be ints with S in {MIN_S}..{MAX_S}, A >= 1 and A * S <= {MAX_T} (got A = {A!r}, S = {S!r})"
        elif F > MAX_FACES or (F + 1) // 2 > A * A:
            why = f"{F} faces: at most 2^28 - 1, and two per square of the {A} x {A} atlas"
        elif centers.dim() != 2 or centers.shape[1] != 3 or centers.shape[0] != F * G:
            why = f"centers must be [F G, 3] with F = {F} (got {list(centers.shape)})"
        elif not 1 <= G <= MAX_G:
            why = f"G must be in 1..{MAX_G} (got {G})"
        elif tuple(inv_scaled_rot.shape) != (F * G, 3, 3):
            why = f"inv_scaled_rot must be [F G, 3, 3] with F G = {F * G} (got {list(inv_scaled_rot.shape)})"
        elif tuple(features.shape) != (F * G, 3):
            why = f"features must be [F G, 3] with F G = {F * G} (got {list(features.shape)})"
        elif tuple(texel_offset.shape) != (2, n, 2) or tuple(texel_bary.shape) != (2, n, 3) or not 1 <= n <= S * S:
            why = (f"texel_offset must be [2, n, 2] and texel_bary [2, n, 3] with 1 <= n <= S S (got {list(texel_offset.shape)}, "
                   f"{list(texel_bary.shape)})")
    _takes.refuse("fill", why or _takes.capturing(ALLOCATES))
    from . import _lib

    v, fc, c, M, ft, off, wt = _takes.cs(verts, faces, centers, inv_scaled_rot, features, texel_offset, texel_bary)
    T = A * S
    tex = torch.empty((T, T, 3), dtype=torch.float32, device=v.device)
    with torch.cuda.device(v.device):
        _lib.call("gsr_texture_fill", v.shape[0], F, G, A, S, n, _lib.ptr(v), _lib.ptr(fc), _lib.ptr(c), _lib.ptr(M), _lib.ptr(ft),
                  off.data_ptr(), wt.data_ptr(), tex.data_ptr(), device=v.device)
    return tex


# ---- what install() puts in the reference's module ----
def drop_in(original: Callable) -> Callable:
    """``extract_texture_image_and_uv_from_gaussians(rc, square_size=10, n_sh=-1, texture_with_gaussian_renders=True)`` ->
    ``(verts_uv, faces_uv, texture_img)``.  Takes the call when ``texture_with_gaussian_renders`` is true, the model is on the GPU in fp32,
    ``4 <= square_size <= 32``, at most 8 Gaussians per triangle, autograd is off and no graph is being captured; every other call --
    ``square_size < 3`` and its ``ValueError`` among them -- runs ``original`` with the caller's arguments, decided before anything is
    consumed.  ``MeshRasterizer``, ``RasterizationSettings`` and ``Meshes`` are the reference module's own; no shader is built."""
    names = getattr(original, "__globals__", {})

    def takes(rc, square_size, n_sh, texture_with_gaussian_renders) -> bool:
        if not texture_with_gaussian_renders or torch.is_grad_enabled() or _takes.capturing(ALLOCATES):
            return False
        if type(square_size) is not int or not MIN_S <= square_size <= MAX_S or type(n_sh) is not int:
            return False
        if not all(callable(names.get(k)) for k in ("MeshRasterizer", "RasterizationSettings", "Meshes")):
            return False
        try:
            G = rc.n_gaussians_per_surface_triangle
            verts, faces = rc.surface_mesh.verts_list()[0], rc.surface_mesh.faces_list()[0]
            points, sh = rc.points, rc.sh_coordinates
            pixels = int(rc.image_height) * int(rc.image_width)
        except (AttributeError, IndexError, TypeError, ValueError):
            return False
        if type(G) is not int or not 1 <= G <= MAX_G:
            return False
        tensors = (verts, faces, points, sh)
        if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.device == verts.device for t in tensors):
            return False
        if verts.dtype != torch.float32 or points.dtype != torch.float32 or sh.dtype != torch.float32 or faces.dtype != torch.int64:
            return False
        F = faces.shape[0]
        if faces.dim() != 2 or F == 0 or F > MAX_FACES or points.shape[0] != F * G or sh.dim() != 3 or sh.shape[0] != F * G or sh.shape[2] != 3:
            return False
        if (n_sh if n_sh != -1 else sh.shape[1]) < 1 or square_size * squares_per_axis(F) > MAX_T:
            return False
        return 0 < pixels <= MAX_PIXELS

    def extract_texture_image_and_uv_from_gaussians(rc, square_size=10, n_sh=-1, texture_with_gaussian_renders=True):
        if not takes(rc, square_size, n_sh, texture_with_gaussian_renders):
            return original(rc, square_size=square_size, n_sh=n_sh, texture_with_gaussian_renders=texture_with_gaussian_renders)
        verts, faces = rc.surface_mesh.verts_list()[0], rc.surface_mesh.faces_list()[0]
        F, G, device = faces.shape[0], rc.n_gaussians_per_surface_triangle, verts.device
        if n_sh == -1:
            n_sh = rc.sh_coordinates.shape[1]
        verts_uv, faces_uv, T, A, offsets, barys = atlas(F, square_size, device)
        features = rc.sh_coordinates[:, :n_sh].reshape(F * G, n_sh * 3)[:, :3]
        tex = fill(verts, faces, rc.points.reshape(F * G, 3),
                   rc.get_covariance(return_full_matrix=True, return_sqrt=True, inverse_scales=True).reshape(F * G, 3, 3), features,
                   offsets, barys, A, square_size)
        count = torch.zeros((T, T, 1), dtype=torch.float32, device=device)
        owner = new_owner(T, device)
        face_uvs = verts_uv[faces_uv]
        cameras = rc.nerfmodel.training_cameras
        settings = names["RasterizationSettings"](image_size=(rc.image_height, rc.image_width), blur_radius=0.0, faces_per_pixel=1)
        rasterizer = names["MeshRasterizer"](cameras=cameras.p3d_cameras[0], raster_settings=settings)
        mesh = names["Meshes"](verts=[verts], faces=[faces])
        for cam_idx in range(len(cameras)):
            rgb_img = rc.render_image_gaussian_rasterizer(camera_indices=cam_idx, sh_deg=0, compute_color_in_rasterizer=True).clamp(min=0, max=1)
            fragments = rasterizer(mesh, cameras=cameras.p3d_cameras[cam_idx])
            bake_view(tex, count, owner, rgb_img[..., :3], fragments.pix_to_face, fragments.bary_coords, fragments.zbuf, face_uvs)
        return verts_uv, faces_uv, tex / count.clamp(min=1)

    return _takes.dressed(extract_texture_image_and_uv_from_gaussians, "extract_texture_image_and_uv_from_gaussians", original,
                          "extract_texture_image_and_uv_from_gaussians", "texture")
