"""Numpy fp32 restatements of the quadrant reach test (gsr_device.h: splat_reaches_rect), operation for operation: the four-edge
form the library had (copied from scripts/blend_subblock_census.py as it stood) and the two-line form it has now.  Shared by
tests/test_reach_lines_host.py and tests/test_reach_lines_gpu.py.  fminf / fmaxf are np.fmin / np.fmax (a NaN operand gives the
other one); 1 / x stands for the hardware reciprocal (1 ulp: it moves a line's minimiser, and q only to second order)."""
import numpy as np

F = np.float32
INF = F(np.inf)


def f32(*arrays):
    return tuple(np.asarray(a, F) for a in arrays)


def skip_below_of(opacity):
    """blend_skip_below: -logf(255 o) - 1e-4 in fp32."""
    with np.errstate(all="ignore"):
        return (-np.log(F(255.0) * np.asarray(opacity, F)) - F(1.0e-4)).astype(F)


def _edge_q(A, B, C, dx, dy):
    return F(0.5) * (A * dx * dx + C * dy * dy) + B * dx * dy


def _clamp(lo, hi, v):
    return np.fmin(hi, np.fmax(lo, v))


def _setup(A, B, C, skip, cx, cy, x0, y0, w, h):
    A, B, C, skip, cx, cy = f32(A, B, C, skip, cx, cy)
    x_first, x_last, y_first, y_last = f32(x0, np.asarray(x0) + w - 1, y0, np.asarray(y0) + h - 1)
    irregular = ~(A > 0) | ~(C > 0) | ~((B * B) < F(0.99) * (A * C))
    budget = -skip - F(1.0e-4)
    x_lo, x_hi, y_lo, y_hi = cx - x_last, cx - x_first, cy - y_last, cy - y_first
    nb_c, nb_a = -B * (F(1.0) / C), -B * (F(1.0) / A)
    return A, B, C, irregular, budget, x_lo, x_hi, y_lo, y_hi, nb_c, nb_a


def reach_edges(A, B, C, skip, cx, cy, x0, y0, w=8, h=8):
    """The parent's predicate: centre-inside test, then the minimum over the four edges.  Returns (keeps, qmin, centre inside)."""
    with np.errstate(all="ignore"):
        A, B, C, irregular, budget, x_lo, x_hi, y_lo, y_hi, nb_c, nb_a = _setup(A, B, C, skip, cx, cy, x0, y0, w, h)
        inside = (x_lo <= 0) & (x_hi >= 0) & (y_lo <= 0) & (y_hi >= 0)
        qmin = _edge_q(A, B, C, x_lo, _clamp(y_lo, y_hi, nb_c * x_lo))
        qmin = np.fmin(qmin, _edge_q(A, B, C, x_hi, _clamp(y_lo, y_hi, nb_c * x_hi)))
        qmin = np.fmin(qmin, _edge_q(A, B, C, _clamp(x_lo, x_hi, nb_a * y_lo), y_lo))
        qmin = np.fmin(qmin, _edge_q(A, B, C, _clamp(x_lo, x_hi, nb_a * y_hi), y_hi))
        return irregular | inside | ~(qmin * F(0.998) - F(1.0e-3) > budget), qmin, inside


def reach_lines(A, B, C, skip, cx, cy, x0, y0, w=8, h=8):
    """The library's predicate: the minimum over the two lines through the rectangle's point nearest the centre.  Returns
    (keeps, qmin)."""
    with np.errstate(all="ignore"):
        A, B, C, irregular, budget, x_lo, x_hi, y_lo, y_hi, nb_c, nb_a = _setup(A, B, C, skip, cx, cy, x0, y0, w, h)
        x_e, y_e = _clamp(x_lo, x_hi, F(0.0)), _clamp(y_lo, y_hi, F(0.0))
        qmin = _edge_q(A, B, C, x_e, _clamp(y_lo, y_hi, nb_c * x_e))
        qmin = np.fmin(qmin, _edge_q(A, B, C, _clamp(x_lo, x_hi, nb_a * y_e), y_e))
        return irregular | ~(qmin * F(0.998) - F(1.0e-3) > budget) | ~(budget + x_lo > -INF), qmin


def line_minima(A, B, C, cx, cy, x0, y0, w=8, h=8):
    """The two-line form's minimum on the vertical and on the horizontal line, separately (fp32)."""
    with np.errstate(all="ignore"):
        A, B, C, _, _, x_lo, x_hi, y_lo, y_hi, nb_c, nb_a = _setup(A, B, C, np.zeros_like(np.asarray(A, F)), cx, cy, x0, y0, w, h)
        x_e, y_e = _clamp(x_lo, x_hi, F(0.0)), _clamp(y_lo, y_hi, F(0.0))
        return _edge_q(A, B, C, x_e, _clamp(y_lo, y_hi, nb_c * x_e)), _edge_q(A, B, C, _clamp(x_lo, x_hi, nb_a * y_e), y_e)


def conic_of(sigma_major, sigma_minor, angle):
    """The conic the projection gives a splat with these standard deviations (pixels) along and across `angle`: the inverse of
    the 2D covariance with the reference's 0.3 added to its diagonal (forward.cu:110-136), in fp64, rounded to fp32."""
    s1, s2, t = (np.asarray(a, np.float64) for a in (sigma_major, sigma_minor, angle))
    c, s = np.cos(t), np.sin(t)
    a = c * c * s1 * s1 + s * s * s2 * s2 + 0.3
    b = c * s * (s1 * s1 - s2 * s2)
    d = s * s * s1 * s1 + c * c * s2 * s2 + 0.3
    det = a * d - b * b
    return f32(d / det, -b / det, a / det)


def q64(A, B, C, cx, cy, x0, y0, w=8, h=8):
    """q at the w x h pixel centres of the rectangle in fp64 from the fp32 operands: [cases, h * w]."""
    A, B, C, cx, cy = (np.asarray(v, np.float64)[:, None] for v in f32(A, B, C, cx, cy))
    ys, xs = (g.reshape(1, -1).astype(np.float64) for g in np.mgrid[0:h, 0:w])
    dx = cx - (np.asarray(x0, np.float64).reshape(-1, 1) + xs)
    dy = cy - (np.asarray(y0, np.float64).reshape(-1, 1) + ys)
    return 0.5 * (A * dx * dx + C * dy * dy) + B * dx * dy
