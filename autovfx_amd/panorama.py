"""Panoramas on the GPU: a drop-in for the reference's ``render_panorama`` (``sugar/gaussian_splatting/render_panorama.py:100-145``).

What the reference does, on one host thread: six blocking ``render()`` calls for the faces of a cube map around ``center``
(``create_cube_map_views``, ``:77-97``), each face written with ``torchvision.utils.save_image`` and copied to the host, then
``c2e(faces, pano_h, pano_w, mode='bilinear', cube_format='dict')`` in numpy / scipy (``utils/py360_utils.py:7-65``) and the
panorama saved through PIL as ``pano_ldr.png``.

Here:
* the six faces are rendered IN FLIGHT (``renderer.render_begin`` / ``finish`` on the side streams the frame loop uses); their
  images are those of six blocking ``render()`` calls, bit for bit;
* the cube-to-equirect resample is one HIP kernel (``gsr_cube_to_equirect``, ``csrc/gsr_panorama.hip``) that reproduces ``c2e``:
  face type, fp32 face coordinates, seam padding, bilinear weights ("Panoramas", states the parity contract);
* the seven files are built as FILE IMAGES on the GPU (``gsr_pack_rgba8`` with save_image's rounding for the faces, the kernel's
  fused truncating quantisation for the panorama, ``gsr_png_encode_deflate`` for all seven), leave through ONE device-to-host copy
  and are written by host threads.

``c2e_host`` restates ``c2e`` in numpy: the checker for sizes the reference's own function would take seconds over, and the
reference-shaped side of ``scripts/bench_panorama.py``.  It is not on the product path: there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import math
import os
import threading
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, Mapping, Optional, Sequence, Union

import numpy as np
import torch

from .cameras import Camera

FACE_ORDER = ("front", "right", "back", "left", "up", "down")     # c2e's dict order (cube_dict2h): the kernel's face index
VIEW_ORDER = ("front", "back", "left", "right", "up", "down")     # create_cube_map_views' order: the reference renders and saves in it
# lookat, up per view (render_panorama.py:87-94)
_VIEWS = {"front": ((1, 0, 0), (0, 0, 1)), "back": ((-1, 0, 0), (0, 0, 1)), "left": ((0, 1, 0), (0, 0, 1)),
          "right": ((0, -1, 0), (0, 0, 1)), "up": ((0, 0, 1), (-1, 0, 0)), "down": ((0, 0, -1), (1, 0, 0))}
FOV = math.pi / 2
ZNEAR, ZFAR = 0.01, 100.0


# ------------------------------------------------------------------------------------------------------------------------------------
# cameras
# ------------------------------------------------------------------------------------------------------------------------------------
def cube_map_cameras(center, size: int = 1024) -> Dict[str, Camera]:
    """The six cameras ``create_cube_map_views(center, size)`` builds (``render_panorama.py:27-38,77-97``), in its order:
    ``right = lookat x up``, ``down = lookat x right``, c2w columns (right, down, lookat) at ``center``, ``w2c = inv(c2w)``; 90-degree
    field of view, znear 0.01, zfar 100.  Host tensors (``Camera.batch_to`` moves them)."""
    center = np.asarray(center, dtype=np.float64).reshape(3)
    cams = {}
    for name in VIEW_ORDER:
        lookat, up = (np.array(a) for a in _VIEWS[name])
        right = np.cross(lookat, up)
        down = np.cross(lookat, right)
        c2w = np.eye(4)
        c2w[:3, :3] = np.array([right, down, lookat]).T
        c2w[:3, 3] = center
        w2c = np.linalg.inv(c2w)
        cams[name] = Camera.from_Rt(w2c[:3, :3].T, w2c[:3, 3], FOV, FOV, size, size, name, znear=ZNEAR, zfar=ZFAR)
    return cams


# ------------------------------------------------------------------------------------------------------------------------------------
# the equirectangular grid: face type per pixel and the angles, in numpy's arithmetic
# ------------------------------------------------------------------------------------------------------------------------------------
def _check_size(h: int, w: int) -> None:
    if w % 8 != 0 or w <= 0:
        raise ValueError(f"the panorama's width ({w}) must be a positive multiple of 8")
    if h < 2:
        raise ValueError(f"the panorama's height ({h}) must be at least 2")


def equirect_grid(h: int, w: int):
    """``(u, v, ceil)``: the fp32 longitude of every column and latitude of every row (``equirect_uvgrid``), and the int32 height of
    the up face above each column of a quarter of the width (``equirect_facetype``'s ceiling mask; the down face mirrors it)."""
    _check_size(h, w)
    u = np.linspace(-np.pi, np.pi, num=w, dtype=np.float32)
    v = np.linspace(np.pi, -np.pi, num=h, dtype=np.float32) / 2
    lon = np.linspace(-np.pi, np.pi, w // 4) / 4
    ceil = (h // 2 - np.round(np.arctan(np.cos(lon)) * h / np.pi).astype(np.int64)).astype(np.int32)
    if ceil.min() < 0:
        raise ValueError(f"no ceiling for a {h}x{w} panorama")
    return u, v, ceil


def face_type(h: int, w: int) -> np.ndarray:
    """int32 ``[h, w]``: the face each pixel samples (0 front, 1 right, 2 back, 3 left, 4 up, 5 down) -- ``equirect_facetype``, from
    the same ceilings the kernel reads and by the kernel's rule."""
    _u, _v, ceil = equirect_grid(h, w)
    q = w // 4
    src = (np.arange(w) + w - 3 * (w // 8)) % w               # the column of the unrolled map: a roll right by 3w/8
    c = ceil[src % q][None, :]
    rows = np.arange(h)[:, None]
    tp = np.broadcast_to(src // q, (h, w)).astype(np.int32)
    tp = np.where(rows < c, 4, tp)
    tp = np.where(h - 1 - rows < c, 5, tp)
    return tp.astype(np.int32)


def pad_source(S: int):
    """``(face, row, col)``, int64 ``[6, S+2, S+2]`` each: the texel of the six ``S x S`` faces that the reference's padded cube
    (``sample_cubefaces``: two rows, then two columns from the row-padded neighbours) holds at every position; face -1 where it
    holds a zero.  The same mapping as ``pad_source`` in ``csrc/gsr_panorama.hip``."""
    m = S - 1
    k, r, c = (a.astype(np.int64) for a in np.meshgrid(np.arange(6), np.arange(S + 2), np.arange(S + 2), indexing="ij"))
    k, r, c = k.copy(), r.copy(), c.copy()
    zero = np.zeros_like(k, dtype=bool)
    # column pads first (they may resolve to a neighbour's row pad)
    first, second = c == S, c == S + 1
    side = k < 4
    colpad = first | second
    sel = colpad & side
    k[sel] = np.where(first[sel], (k[sel] + 1) % 4, (k[sel] + 3) % 4)
    c[sel] = np.where(first[sel], 0, m)
    ud = colpad & ~side
    zero |= ud & ((r == 0) | (r == S + 1))
    ud &= ~zero
    up = ud & (k == 4)
    dn = ud & (k == 5)
    c[up] = np.where(first[up], S - r[up], r[up] - 1)
    c[dn] = np.where(first[dn], r[dn] - 1, S - r[dn])
    r[up], r[dn] = 0, S
    k[ud] = np.where(first[ud], 1, 3)
    # then row pads
    rowpad = (r >= S) & ~zero
    fr = r == S
    table = {  # face: (first row pad, second row pad) as (face, row, col) functions of the column
        0: ((5, lambda c: 0, lambda c: c), (4, lambda c: m, lambda c: c)),
        1: ((5, lambda c: c, lambda c: m), (4, lambda c: m - c, lambda c: m)),
        2: ((5, lambda c: m, lambda c: m - c), (4, lambda c: 0, lambda c: m - c)),
        3: ((5, lambda c: m - c, lambda c: 0), (4, lambda c: c, lambda c: 0)),
        4: ((0, lambda c: 0, lambda c: c), (2, lambda c: 0, lambda c: m - c)),
        5: ((2, lambda c: m, lambda c: m - c), (0, lambda c: m, lambda c: c)),
    }
    k0 = k.copy()
    nk, nr, nc = k.copy(), r.copy(), c.copy()
    for face, pads in table.items():
        for which, (to, row_of, col_of) in enumerate(pads):
            sel = rowpad & (k0 == face) & (fr if which == 0 else ~fr)
            nk[sel], nr[sel], nc[sel] = to, row_of(c[sel]), col_of(c[sel])
    nk[zero] = -1
    nr[zero] = nc[zero] = 0
    return nk, nr, nc


def _face_coordinates(tp: np.ndarray, u: np.ndarray, v: np.ndarray, S: int):
    """``c2e``'s face coordinates: fp32 in its operation order, renormalised in fp64 to ``0 .. S``."""
    h, w = tp.shape
    U = np.broadcast_to(u[None, :], (h, w))
    V = np.broadcast_to(v[:, None], (h, w))
    cx = np.zeros((h, w))
    cy = np.zeros((h, w))
    for i in range(4):
        sel = tp == i
        a = U[sel] - np.float32(np.pi * i / 2)
        cx[sel] = np.float32(0.5) * np.tan(a)
        cy[sel] = (np.float32(-0.5) * np.tan(V[sel])) / np.cos(a)
    for i in (4, 5):
        sel = tp == i
        lat = V[sel] if i == 4 else np.abs(V[sel])
        c = np.float32(0.5) * np.tan(np.float32(np.pi / 2) - lat)
        cx[sel] = c * np.sin(U[sel])
        cy[sel] = c * np.cos(U[sel]) if i == 4 else -c * np.cos(U[sel])
    return (np.clip(cx, -0.5, 0.5) + 0.5) * S, (np.clip(cy, -0.5, 0.5) + 0.5) * S


def _as_face_list(faces) -> list:
    if isinstance(faces, Mapping):
        return [faces[k] for k in FACE_ORDER]
    faces = list(faces)
    if len(faces) != 6:
        raise ValueError("a cube map has six faces")
    return faces


def c2e_host(faces, h: int, w: int) -> np.ndarray:
    """numpy restatement of the reference's ``c2e(faces, h, w, mode='bilinear', cube_format='dict')``: ``faces`` is a dict with the
    reference's keys or a sequence of six ``[S, S, C]`` arrays in ``FACE_ORDER``; returns float64 ``[h, w, C]``."""
    F = np.stack([np.asarray(f, dtype=np.float64) for f in _as_face_list(faces)])     # [6, S, S, C]
    if F.ndim != 4 or F.shape[1] != F.shape[2]:
        raise ValueError("faces must be six [S, S, C] arrays")
    S = F.shape[1]
    u, v, _ceil = equirect_grid(h, w)
    tp = face_type(h, w)
    x, y = _face_coordinates(tp, u, v, S)
    nk, nr, nc = pad_source(S)
    padded = np.where((nk >= 0)[..., None], F[np.maximum(nk, 0), nr, nc], 0.0)        # [6, S+2, S+2, C]
    x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    wx0, wy0 = 1.0 - (x - x0), 1.0 - (y - y0)
    wx, wy = (wx0, 1.0 - wx0), (wy0, 1.0 - wy0)                                          # map_coordinates' order-1 weights
    out = np.zeros((h, w, F.shape[3]))
    for t in range(4):
        a, b = t >> 1, t & 1
        out += padded[tp, y0 + a, x0 + b] * wy[a][..., None] * wx[b][..., None]
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# the kernel
# ------------------------------------------------------------------------------------------------------------------------------------
_GRIDS: dict = {}
_GRIDS_LOCK = threading.Lock()


def _device_grid(h: int, w: int, device):
    key = (h, w, str(device))
    with _GRIDS_LOCK:
        got = _GRIDS.get(key)
        if got is None:
            u, v, ceil = equirect_grid(h, w)
            got = tuple(torch.from_numpy(a).to(device) for a in (u, v, ceil))
            _GRIDS[key] = got
    return got


def _face_tensors(faces, what: str, depth: bool = False):
    faces = _as_face_list(faces)
    out = []
    for i, f in enumerate(faces):
        if not isinstance(f, torch.Tensor) or not f.is_cuda:
            raise RuntimeError(f"cube_to_equirect: {what} must live on a HIP device (there is no CPU fallback)")
        if f.dtype != torch.float32:
            raise ValueError(f"cube_to_equirect: {what} must be float32")
        if depth and f.dim() == 3:
            f = f.reshape(f.shape[-2], f.shape[-1])
        if f.dim() != (2 if depth else 3) or f.shape[-1] != f.shape[-2]:
            raise ValueError(f"cube_to_equirect: {what} must be {'[S, S] or [1, S, S]' if depth else '[C, S, S]'}")
        out.append(f.contiguous())
    if len({tuple(f.shape) for f in out}) != 1 or len({f.device for f in out}) != 1:
        raise ValueError(f"cube_to_equirect: the six {what} must have one shape and one device")
    return out


def cube_to_equirect(faces, h: int, w: int, depth=None, out_uint8: bool = False, *, out=None, out_depth=None):
    """``c2e`` of the reference on the GPU (``gsr_cube_to_equirect``).  ``faces``: six planar float32 ``[C, S, S]`` device tensors
    (``render()["render"]``) in ``FACE_ORDER``, or a dict with the reference's keys.  Returns the float32 ``[h, w, C]`` panorama, or with
    ``out_uint8`` the bytes the reference saves, ``uint8(clip(x * 255, 0, 255))`` (truncation) of it, ``[h, w, C]``.  With ``depth``
    (six ``[S, S]`` / ``[1, S, S]`` depth planes, same order) returns ``(panorama, radial)``: ``radial`` the float32 ``[h, w]`` distance
    from the cube's centre ("Panoramas").  ``out`` / ``out_depth``: tensors to write into.  Queued on the current stream."""
    from . import _lib
    _check_size(h, w)
    F = _face_tensors(faces, "faces")
    C, S = int(F[0].shape[0]), int(F[0].shape[-1])
    dev = F[0].device
    D = _face_tensors(depth, "depth planes", depth=True) if depth is not None else None
    if D is not None and (D[0].device != dev or int(D[0].shape[-1]) != S):
        raise ValueError("cube_to_equirect: the depth planes must match the faces' size and device")
    dtype = torch.uint8 if out_uint8 else torch.float32
    if out is None:
        out = torch.empty((h, w, C), dtype=dtype, device=dev)
    if not (out.is_contiguous() and out.dtype == dtype and out.device == dev and tuple(out.shape) == (h, w, C)):
        raise ValueError(f"cube_to_equirect: out must be a contiguous {dtype} tensor [{h}, {w}, {C}] on {dev}")
    if D is not None:
        if out_depth is None:
            out_depth = torch.empty((h, w), dtype=torch.float32, device=dev)
        if not (out_depth.is_contiguous() and out_depth.dtype == torch.float32 and out_depth.device == dev and tuple(out_depth.shape) == (h, w)):
            raise ValueError(f"cube_to_equirect: out_depth must be a contiguous float32 tensor [{h}, {w}] on {dev}")
    gu, gv, gc = _device_grid(h, w, dev)
    ptrs = (ctypes.c_void_p * 6)(*[f.data_ptr() for f in F])
    dptrs = (ctypes.c_void_p * 6)(*[f.data_ptr() for f in D]) if D is not None else None
    with torch.cuda.device(dev):
        _lib.call("gsr_cube_to_equirect", ptrs, S, C, dptrs, gu.data_ptr(), gv.data_ptr(), gc.data_ptr(), h, w,
                  None if out_uint8 else out.data_ptr(), out.data_ptr() if out_uint8 else None,
                  None if D is None else out_depth.data_ptr(), device=dev)
    return out if D is None else (out, out_depth)


# ------------------------------------------------------------------------------------------------------------------------------------
# the faces, in flight
# ------------------------------------------------------------------------------------------------------------------------------------
def render_cube_faces(gaussians, pipeline, background, center, size: int = 1024, streams: Optional[int] = None) -> Dict[str, dict]:
    """The six ``render()`` results of the cube map around ``center`` (``VIEW_ORDER``), rendered in flight by the frame loop's
    driver (``frame_loop._frames_in_flight``): ``render_begin`` on side streams, ``finish`` oldest first, at most ``streams`` faces
    queued.  The images are those of six blocking ``render()`` calls, bit for bit; the caller's stream is ordered behind them when
    this returns.  A model / pipeline the split path does not take gets blocking ``render()`` calls instead (same kernels)."""
    from . import frame_loop
    device = background.device
    if device.type != "cuda":
        raise RuntimeError("render_cube_faces: the background must live on a HIP device (there is no CPU fallback)")
    cams = cube_map_cameras(center, size)
    views = dict(zip(VIEW_ORDER, Camera.batch_to([cams[n] for n in VIEW_ORDER], device)))
    S = max(1, int(frame_loop.DEFAULT_STREAMS if streams is None else streams))
    main = torch.cuda.current_stream(device)
    results: Dict[str, dict] = {}
    with torch.no_grad():
        frame_loop._frames_in_flight(device, S, VIEW_ORDER, lambda name, slot: (views[name], gaussians), pipeline, background,
                                     results.__setitem__)
        for res in results.values():       # made on a side stream, read on the caller's: keep the memory until that stream is done
            for t in res.values():
                if isinstance(t, torch.Tensor) and t.is_cuda:
                    t.record_stream(main)
    return {name: results[name] for name in VIEW_ORDER}


# ------------------------------------------------------------------------------------------------------------------------------------
# the drop-in
# ------------------------------------------------------------------------------------------------------------------------------------
_PINNED: dict = {}          # page-locked staging per byte count (pinning megabytes costs milliseconds per call)
_PINNED_LOCK = threading.Lock()


def _pinned(nbytes: int) -> torch.Tensor:
    buf = _PINNED.get(nbytes)
    if buf is None:
        _PINNED.clear()
        buf = _PINNED[nbytes] = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    return buf


def _align(n: int, a: int = 256) -> int:
    return (n + a - 1) // a * a


def render_panorama(gaussians, pipeline, background, center, output_dir, pano_h: int = 1024, pano_w: int = 2048, *,
                    face_size: int = 1024, return_depth: bool = False):
    """The reference's ``render_panorama`` (same arguments, same files, same return value: the path of ``pano_ldr.png``):
    ``<view>.png`` for the six faces (RGBA, ``save_image``'s rounding) and ``pano_ldr.png`` (RGBA, ``uint8(clip(x * 255, 0, 255))``).
    ``face_size``: the faces' side (the reference's 1024).  ``return_depth``: also return the radial-distance panorama, float32
    ``[pano_h, pano_w]`` on the GPU -- the reference's TODO at ``render_panorama.py:127`` -- as ``(path, radial)``."""
    from . import _lib
    from .frame_io import png_deflate_max_size, png_deflate_room, png_deflate_scratch
    from .frame_parallel import pack_rgba8
    _check_size(pano_h, pano_w)
    os.makedirs(output_dir, exist_ok=True)
    device = background.device
    S = int(face_size)
    with torch.no_grad():
        faces = render_cube_faces(gaussians, pipeline, background, center, S)
        images = {n: faces[n]["render"] for n in VIEW_ORDER}
        depth = [faces[n]["depth"] for n in FACE_ORDER] if return_depth else None
        C = int(images["front"].shape[0])
        if C != 4:
            raise RuntimeError(f"render_panorama: render() returned {C} channels, the files are RGBA")
        res = cube_to_equirect([images[n] for n in FACE_ORDER], pano_h, pano_w, depth=depth, out_uint8=True)
        pano_u8, radial = res if return_depth else (res, None)

        # seven file images in one device buffer: [face PNGs in VIEW_ORDER, panorama PNG, lengths int64[7]]
        jobs = [(images[n], S, S, True) for n in VIEW_ORDER] + [(pano_u8, pano_w, pano_h, False)]
        rooms = [_align(png_deflate_room(w_, h_, 4)) for _img, w_, h_, _p in jobs]
        offsets = np.concatenate(([0], np.cumsum(rooms))).astype(np.int64)
        total = int(offsets[-1]) + 8 * len(jobs)
        staging = torch.empty(total, dtype=torch.uint8, device=device)
        lengths = staging[int(offsets[-1]):].view(torch.int64)
        scratch = torch.empty(max(png_deflate_scratch(w_, h_, 4) for _img, w_, h_, _p in jobs), dtype=torch.uint8, device=device)
        packed = torch.empty((4, S, S), dtype=torch.uint8, device=device)
        for j, (img, w_, h_, planar) in enumerate(jobs):
            src = pack_rgba8(img[:3], img[3:], out=packed) if planar else img
            with torch.cuda.device(device):
                _lib.call("gsr_png_encode_deflate", src.data_ptr(), w_, h_, 4, 1 if planar else 0, staging.data_ptr() + int(offsets[j]),
                          scratch.data_ptr(), lengths.data_ptr() + 8 * j, device=device)
        with _PINNED_LOCK:
            host = _pinned(total)
            host.copy_(staging, non_blocking=True)
            torch.cuda.current_stream(device).synchronize()
            data = host.numpy()
            lens = data[int(offsets[-1]):].view(np.int64).copy()
            names = [n + ".png" for n in VIEW_ORDER] + ["pano_ldr.png"]

            def write(j):
                n = int(lens[j])
                w_, h_ = jobs[j][1], jobs[j][2]
                if not 0 < n <= png_deflate_max_size(w_, h_, 4):
                    raise RuntimeError(f"{names[j]}: the GPU encoder reported {n} bytes")
                with open(os.path.join(output_dir, names[j]), "wb") as f:
                    f.write(memoryview(data)[int(offsets[j]):int(offsets[j]) + n])

            with ThreadPoolExecutor(max_workers=4) as pool:
                list(pool.map(write, range(len(jobs))))
    path = os.path.join(output_dir, "pano_ldr.png")
    return (path, radial) if return_depth else path
