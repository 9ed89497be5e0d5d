"""What the numpy restatements of the mesh kernels share (``meshattrs.py``, ``meshloss.py``, ``bound.py``, ``texture.py``): 3-vector
arithmetic over the last axis, the checked gather of a face's corners, and the face normal of DESIGN.md 7j with its backward -- the host
side of ``csrc/gsr_vec3.h``, with the same operation order.  Every operation is an fp32 elementwise one; nothing here calls the library.
Callers wrap their arithmetic in ``np.errstate(all="ignore")``.
"""
from __future__ import annotations

import numpy as np

_F = np.float32
FACE_NORMAL_EPS = _F(1e-6)


def dot(u: np.ndarray, w: np.ndarray) -> np.ndarray:
    """``((u0 w0 + u1 w1) + u2 w2) + ...`` over the last axis."""
    acc = u[..., 0] * w[..., 0]
    for i in range(1, u.shape[-1]):
        acc = acc + u[..., i] * w[..., i]
    return acc


def norm(w: np.ndarray) -> np.ndarray:
    return np.sqrt(dot(w, w))


def cross(u: np.ndarray, w: np.ndarray) -> np.ndarray:
    return np.stack((u[..., 1] * w[..., 2] - u[..., 2] * w[..., 1], u[..., 2] * w[..., 0] - u[..., 0] * w[..., 2],
                     u[..., 0] * w[..., 1] - u[..., 1] * w[..., 0]), axis=-1)


def verts_faces(verts, faces):
    """``verts [V, 3]`` float32 and ``faces [F, 3]`` int64, contiguous."""
    return (np.ascontiguousarray(np.asarray(verts, dtype=_F).reshape(-1, 3)), np.ascontiguousarray(np.asarray(faces, dtype=np.int64).reshape(-1, 3)))


def face_corners(verts: np.ndarray, faces: np.ndarray):
    """``valid [F]`` (every index inside ``[0, V)``) and ``v0, v1, v2 [F, 3]``: zeros for the faces that are not valid, which read nothing."""
    V = verts.shape[0]
    valid = ((faces >= 0) & (faces < V)).all(axis=1)
    if V == 0:
        zero = np.zeros((faces.shape[0], 3), _F)
        return valid, zero, zero.copy(), zero.copy()
    idx = np.where(valid[:, None], faces, 0)
    v0, v1, v2 = (np.where(valid[:, None], verts[idx[:, i]], _F(0.0)) for i in range(3))
    return valid, v0, v1, v2


def face_cross(v0: np.ndarray, v1: np.ndarray, v2: np.ndarray):
    """``a = v1 - v0``, ``b = v2 - v0``, ``c = a x b``, ``n = |c|``."""
    a, b = v1 - v0, v2 - v0
    c = cross(a, b)
    return a, b, c, norm(c)


def normal_backward(c: np.ndarray, n: np.ndarray, gn: np.ndarray) -> np.ndarray:
    """``g_c`` of ``normal = c / max(n, 1e-6)`` from the normal's gradient: the projection off ``m = c / n``, over ``n``; below the clamp
    (and for a NaN ``n``) the forward is ``c / 1e-6``."""
    m = c / n[:, None]
    return np.where((n >= FACE_NORMAL_EPS)[:, None], (gn - m * dot(m, gn)[:, None]) / n[:, None], gn / FACE_NORMAL_EPS)
