"""Inputs, the per-pixel bound and the comparison for the cube-to-equirect kernel (tests/test_panorama_seams.py on the CPU,
tests/test_panorama_seams_gpu.py on the MI355X; DESIGN.md 7a states the bound).

The kernel and ``c2e_host`` read the same host tables (face type, fp32 angles) and differ only in the fp32 ``tan`` / ``cos`` / ``sin``
behind the face coordinates.  ``truth_coordinates`` takes those functions, the products and the quotient in float64 from the same
fp32 inputs; ``E(S, h, w)`` is how far the reference's own coordinates lie from that truth, in face-coordinate units (before the
multiplication by S).  The kernel is allowed ``4 E`` against the truth -- four times the original's own error, the yardstick of the
mesh-loss and bound-Gaussian tests -- so its coordinates lie within ``5 E S`` texels of the reference's.  The bilinear interpolant over
a padded face is continuous across cell borders and across the clip, and its slope along either axis is at most the spread of the
padded values, so per pixel and channel

    |got - c2e_host| <= 5 E S * 2 * (max - min of the padded cube's channel) + 2^-24 |c2e_host|

(one x step and one y step; the last term is the fp32 rounding of the output).  Nothing here is measured on the kernel.
"""
import functools

import numpy as np

from autovfx_amd import panorama as pano

ULP = 2.0 ** -24
FACE_NAMES = pano.FACE_ORDER

# (S, h, w, C) of the noise cases: an odd S and an odd h whose second workgroup has 8 live lanes; two workgroups of full rows; one
# channel on a width that is no multiple of 16; the smallest golden size
TAP_CASES = ((7, 65, 264, 3), (16, 256, 512, 4), (8, 33, 72, 1), (5, 8, 16, 3))
COORDINATE_CASE = (64, 128, 256)
SMALLEST_CASE = (2, 2, 8)
SIZES = tuple(c[:3] for c in TAP_CASES) + (COORDINATE_CASE, SMALLEST_CASE)


def noise_faces(S: int, C: int, seed: int, lo: float = 0.0, hi: float = 1.0) -> list:
    """Six float32 ``[S, S, C]`` faces of uniform noise in ``[lo, hi)``."""
    rng = np.random.default_rng(seed)
    return [(np.float32(lo) + np.float32(hi - lo) * rng.random((S, S, C), dtype=np.float32)).astype(np.float32) for _ in range(6)]


def ramp_faces(S: int) -> list:
    """Channel 0 holds the column index and channel 1 the row index: away from the pads the resample returns its own (x, y)."""
    ramp = np.zeros((S, S, 2), np.float32)
    ramp[..., 0] = np.arange(S, dtype=np.float32)[None, :]
    ramp[..., 1] = np.arange(S, dtype=np.float32)[:, None]
    return [ramp.copy() for _ in range(6)]


def radial_planes(depth: list) -> list:
    """``depth * sqrt(1 + x x + y y)`` per texel in fp32, in the kernel's operation order (``radial_factor``; no contraction):
    ``x = float32(2 c + 1 - S) / float32(S)``.  Six ``[S, S]`` planes in, six ``[S, S, 1]`` faces out."""
    S = depth[0].shape[0]
    x = (2 * np.arange(S) + 1 - S).astype(np.float32) / np.float32(S)
    xx = x * x
    factor = np.sqrt((np.float32(1.0) + xx[None, :]) + xx[:, None])                   # [row, col]
    assert factor.dtype == np.float32
    return [(np.asarray(d, np.float32) * factor)[..., None] for d in depth]


def grid(h: int, w: int):
    """``(tp, u, v)``: the face type of every pixel and the fp32 angles, as both sides read them."""
    u, v, _ceil = pano.equirect_grid(h, w)
    return pano.face_type(h, w), u, v


def truth_coordinates(tp: np.ndarray, u: np.ndarray, v: np.ndarray, S: int):
    """``_face_coordinates`` from the same fp32 inputs with every ``tan``, ``cos``, ``sin``, product and quotient in float64.  What stays
    fp32: the subtraction ``u - fp32(pi i / 2)``, the fp32 ``pi / 2`` and ``fp32(pi / 2) - lat``.  The clip and the scale are unchanged."""
    assert u.dtype == v.dtype == np.float32
    h, w = tp.shape
    U = np.broadcast_to(u[None, :], (h, w))
    V = np.broadcast_to(v[:, None], (h, w))
    cx = np.zeros((h, w))
    cy = np.zeros((h, w))
    for i in range(4):
        sel = tp == i
        a32 = U[sel] - np.float32(np.pi * i / 2)
        assert a32.dtype == np.float32
        a = a32.astype(np.float64)
        cx[sel] = 0.5 * np.tan(a)
        cy[sel] = (-0.5 * np.tan(V[sel].astype(np.float64))) / np.cos(a)
    for i in (4, 5):
        sel = tp == i
        lat = V[sel] if i == 4 else np.abs(V[sel])
        t32 = np.float32(np.pi / 2) - lat
        assert t32.dtype == np.float32
        c = 0.5 * np.tan(t32.astype(np.float64))
        Ud = U[sel].astype(np.float64)
        cx[sel] = c * np.sin(Ud)
        cy[sel] = c * np.cos(Ud) if i == 4 else -c * np.cos(Ud)
    return (np.clip(cx, -0.5, 0.5) + 0.5) * S, (np.clip(cy, -0.5, 0.5) + 0.5) * S


@functools.lru_cache(maxsize=None)
def E(S: int, h: int, w: int) -> float:
    """The largest distance, in face-coordinate units, between ``c2e_host``'s coordinates and the truth over all pixels."""
    tp, u, v = grid(h, w)
    rx, ry = pano._face_coordinates(tp, u, v, S)
    tx, ty = truth_coordinates(tp, u, v, S)
    return float(max(np.abs(rx - tx).max(), np.abs(ry - ty).max())) / S


def taps(S: int, h: int, w: int):
    """The reference's four taps per pixel: ``(tp [h, w], rows [4, h, w], cols [4, h, w], weights [4, h, w])`` in the padded face."""
    tp, u, v = grid(h, w)
    x, y = pano._face_coordinates(tp, u, v, S)
    x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    wx0, wy0 = 1.0 - (x - x0), 1.0 - (y - y0)
    wx, wy = (wx0, 1.0 - wx0), (wy0, 1.0 - wy0)
    rows = np.stack([y0 + (t >> 1) for t in range(4)])
    cols = np.stack([x0 + (t & 1) for t in range(4)])
    weights = np.stack([wy[t >> 1] * wx[t & 1] for t in range(4)])
    return tp, rows, cols, weights


def value_spread(faces) -> np.ndarray:
    """max - min per channel of what the padded cube holds: the six faces' values and the zeros of the up / down corners."""
    F = np.stack([np.asarray(f, np.float64) for f in faces])
    return np.maximum(F.max(axis=(0, 1, 2)), 0.0) - np.minimum(F.min(axis=(0, 1, 2)), 0.0)


def bound(faces, h: int, w: int, ref: np.ndarray) -> np.ndarray:
    S = np.asarray(faces[0]).shape[0]
    return 5.0 * E(S, h, w) * S * 2.0 * value_spread(faces)[None, None, :] + ULP * np.abs(ref)


def _describe(faces, h, w, row, col, ch) -> str:
    S = np.asarray(faces[0]).shape[0]
    tp, rows, cols, weights = taps(S, h, w)
    nk, nr, nc = pano.pad_source(S)
    k = int(tp[row, col])
    lines = [f"pixel ({row}, {col}) channel {ch}, face type {k} ({FACE_NAMES[k]})"]
    for t in range(4):
        r, c = int(rows[t, row, col]), int(cols[t, row, col])
        f, sr, sc = int(nk[k, r, c]), int(nr[k, r, c]), int(nc[k, r, c])
        src = "zero" if f < 0 else f"{FACE_NAMES[f]}[{sr}, {sc}] = {float(np.asarray(faces[f])[sr, sc, ch])!r}"
        lines.append(f"  padded ({r}, {c}) weight {weights[t, row, col]:.6f} <- {src}")
    return "\n".join(lines)


def check(got, faces, h: int, w: int, what: str = "") -> float:
    """Assert the per-pixel bound of the module docstring on ``got`` (float32 ``[h, w, C]``) against ``c2e_host(faces, h, w)``;
    prints ``E``, the largest bound and the worst observed ratio, and returns that ratio."""
    faces = [np.asarray(f) for f in faces]
    S, C = faces[0].shape[0], faces[0].shape[2]
    got = np.asarray(got)
    assert got.shape == (h, w, C) and got.dtype == np.float32, (got.shape, got.dtype)
    assert np.isfinite(got).all()
    ref = pano.c2e_host(faces, h, w)
    lim = bound(faces, h, w, ref)
    err = np.abs(got.astype(np.float64) - ref)
    ratio = err / np.maximum(lim, np.finfo(np.float64).tiny)
    worst = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    e = E(S, h, w)
    print(f"{what or 'c2e'} S {S} {h}x{w} C {C}: E {e / ULP:.3f} x 2^-24, bound <= {lim.max():.3e}, max-abs {err.max():.3e}, "
          f"worst error / bound {ratio[worst]:.4f}")
    if not (err <= lim).all():
        row, col, ch = (int(i) for i in worst)
        raise AssertionError(f"{int((err > lim).sum())} of {err.size} elements beyond the bound; worst: got {float(got[worst])!r}, "
                             f"reference {float(ref[worst])!r}, error {err[worst]:.3e} > bound {lim[worst]:.3e}\n"
                             + _describe(faces, h, w, row, col, ch))
    return float(ratio[worst])
