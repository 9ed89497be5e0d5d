"""The fp32 contract of gsr_field.hip as checks without a fitted tolerance, numpy only.

The contract is an exact fp32 operation sequence around one ``expf``.  ``expf`` is the only operation whose bits may differ between a
device and numpy, so it alone gets a window: ``U = 2`` steps on the fp32 number line around ``e0 = fl32(exp(-0.5 q))`` evaluated in
float64 (7g's allowance for the device ``expf``; a condition, not a measurement).  Everything around it is held exactly:

1. opacities: every stored ``o[i, k]`` equals, as bits, ``fl(A step(e0, d))`` for some ``d`` in ``-U .. U`` (``A = fl(density_factor)
   sigma_j``); a slot outside ``[0, P)`` holds ``+0.0``;
2. ``density[i]`` equals, as bits, the k-ascending fp32 sum of the stored opacities' own row; ``beta`` equals ``field_values_host``'s bits;
3. a density without stored opacities (and the march's ``densities [n, S]``) lies in ``[sum_asc(o_lo), sum_asc(o_hi)]`` with ``o_lo``,
   ``o_hi`` the ends of the window: fp32 addition and multiplication round monotonically, so the k-ascending sum is non-decreasing in
   every term, and so is the ``d >= 1 -> d / (d + 1e-12f)`` step;
4. ``hit``, ``t`` and the points equal, as bits, ``crossing_host`` and ``fl(origin + fl(t dir))`` on the densities the kernel itself stored,
   on every ray;
5. a normal lies in the float64 interval image of ``-g / max(|g|, 1e-12f)`` over the box ``[g_lo, g_hi]`` that the window gives at the
   stored point, widened by ``8 2^-24`` of the interval's largest magnitude: seven fp32 roundings lie between ``g`` and a component (three
   squares, two additions, the root, the quotient; the root halves what precedes it, so 3.5 would do).  A hit whose box contains ``g = 0``
   has no direction to hold and is skipped, at most ``SKIP_CAP`` of a case's hits;
6. a pair with a NaN ``q`` is outside the window checks (its opacity must be a NaN); the exact parts hold on every element, a NaN
   matching any NaN.

Every check raises ``AssertionError``; :func:`check_field` and :func:`check_march` return what they observed (the histogram of the
matching ``d``, the widths of the enclosures, the skipped hits)."""
import numpy as np

from autovfx_amd.field import _host_inputs, _host_pairs, field_values_host
from autovfx_amd.levelset import crossing_host

F = np.float32
U = 2
EPS = 2.0 ** -24
SKIP_CAP = 0.01
_ORDER = (0, -1, 1, -2, 2)             # the histogram counts the nearest matching step


def step(v, d: int):
    """``v`` (fp32, >= 0) moved ``d`` steps along the fp32 number line: integer arithmetic on the bit pattern, clamped at 0 and +inf.
    A NaN stays a NaN."""
    v = np.asarray(v, F)
    bits = v.view(np.int32).astype(np.int64)
    moved = np.clip(bits + d, 0, 0x7F800000).astype(np.int32).view(F)
    return np.where(np.isnan(v), v, moved).astype(F)


def same(a, b):
    """Elementwise: the same bits, or a NaN on both sides."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def sum_asc(a):
    """The fp32 sum over the last axis from 0, index ascending."""
    a = np.asarray(a, F)
    out = np.zeros(a.shape[:-1], F)
    for k in range(a.shape[-1]):
        out = out + a[..., k]
    return out


def renorm(d):
    return np.where(d >= 1, d / (d + F(1e-12)), d).astype(F)


def _where(mask):
    at = np.argwhere(mask)
    return f"{int(mask.sum())} of {mask.size}, first at {at[0].tolist() if len(at) else None}"


class Pairs:
    """The expf-free quantities of every (point, slot) pair in the host code's own expressions, and the window around ``e0``."""

    def __init__(self, x, idx, c):
        x, idx, cs, M, sg, _, self.valid, j = _host_inputs(x, idx, c["centers"], c["M"], c["strengths"], None)
        with np.errstate(all="ignore"):
            _, self.w, q_raw, _, self.Mj = _host_pairs(x, cs, M, j)
            # the host's clamp, restated because _host_pairs returns q only before it
            self.q = np.where(q_raw < 0, F(0), np.where(q_raw > F(1e8), F(1e8), q_raw))
            self.e0 = np.exp(-0.5 * self.q.astype(np.float64)).astype(F)
            self.A = F(c["density_factor"]) * sg[j]
            self.finite = self.valid & np.isfinite(self.q)
            self.window = np.stack([(self.A * step(self.e0, d)).astype(F) for d in range(-U, U + 1)])
            lo, hi = np.minimum(self.window[0], self.window[-1]), np.maximum(self.window[0], self.window[-1])
        zero = F(0)
        self.o_lo, self.o_hi = np.where(self.valid, lo, zero), np.where(self.valid, hi, zero)
        self.rows_finite = (self.finite | ~self.valid).all(axis=1)        # rows whose every live pair has a finite q

    def density_bounds(self):
        with np.errstate(all="ignore"):
            return sum_asc(self.o_lo), sum_asc(self.o_hi)

    def Mw(self):
        Mj, w = self.Mj, self.w
        with np.errstate(all="ignore"):
            return (Mj[..., :, 0] * w[..., 0:1] + Mj[..., :, 1] * w[..., 1:2]) + Mj[..., :, 2] * w[..., 2:3]


def check_opacities(o, p: Pairs, label=""):
    """Check 1; the histogram ``{d: pairs}`` of the nearest matching step."""
    o = np.asarray(o, F)
    assert o.shape == p.valid.shape, f"{label}: opacities {o.shape}"
    dead = ~p.valid & (o.view(np.uint32) != 0)
    assert not dead.any(), f"{label}: a slot outside [0, P) does not hold +0.0: {_where(dead)}"
    lost = p.valid & ~p.finite & ~np.isnan(o)
    assert not lost.any(), f"{label}: a NaN q gave an opacity that is no NaN: {_where(lost)}"
    found = np.full(o.shape, 99, np.int64)
    for d in reversed(_ORDER):
        found[same(o, p.window[d + U])] = d
    out = p.finite & (found == 99)
    if out.any():
        i, k = np.argwhere(out)[0]
        off = int(o[i, k].view(np.int32)) - int(p.window[U][i, k].view(np.int32))
        raise AssertionError(f"{label}: opacity outside the {U}-step window of expf: {_where(out)}; there o = {o[i, k]!r}, "
                             f"A e0 = {p.window[U][i, k]!r} ({off:+d} steps of o), q = {p.q[i, k]!r}, e0 = {p.e0[i, k]!r}")
    return {d: int((p.finite & (found == d)).sum()) for d in range(-U, U + 1)}


def _check_enclosed(d, lo, hi, rows, label, what):
    d = np.asarray(d, F)
    with np.errstate(invalid="ignore"):
        out = rows & ~((lo <= d) & (d <= hi))
    if out.any():
        at = tuple(np.argwhere(out)[0])
        raise AssertionError(f"{label}: {what} outside its enclosure: {_where(out)}; there {d[at]!r} not in [{lo[at]!r}, {hi[at]!r}]")
    width = hi.astype(np.float64) - lo.astype(np.float64)
    pos = rows & (d > 0)
    return {"widest": float(width[rows].max()) if rows.any() else 0.0,
            "median_relative": float(np.median(width[pos] / d[pos])) if pos.any() else 0.0, "elements": int(rows.sum())}


def check_field(c, got, label="") -> dict:
    """Checks 1, 2, 3 and 6 on ``got = {"density", "opacities" or None, "beta" or None}`` of the case ``c`` (``x, idx, centers, M,
    strengths, min_scaling, density_factor``)."""
    p = Pairs(c["x"], c["idx"], c)
    density = np.asarray(got["density"], F)
    assert density.shape == (p.valid.shape[0],), f"{label}: density {density.shape}"
    stats = {}
    if got.get("opacities") is not None:
        stats["steps"] = check_opacities(got["opacities"], p, label)
        with np.errstate(all="ignore"):
            own = sum_asc(got["opacities"])
        bad = ~same(density, own)
        assert not bad.any(), f"{label}: density is not the k-ascending fp32 sum of its own opacities: {_where(bad)}"
    lo, hi = p.density_bounds()
    stats["density"] = _check_enclosed(density, lo, hi, p.rows_finite, label, "density")
    if got.get("beta") is not None:
        want = field_values_host(c["x"], c["idx"], c["centers"], c["M"], c["strengths"], c["min_scaling"], c["density_factor"])[2]
        bad = ~same(got["beta"], want)
        assert not bad.any(), f"{label}: beta differs from the host restatement's bits: {_where(bad)}"
    return stats


def _unit_range(lo, hi, r_lo, r_hi):
    """The range of ``g / max(sqrt(g^2 + r^2), 1e-12f)`` over ``g in [lo, hi]``, ``r in [r_lo, r_hi]``, float64: increasing in ``g``,
    and in ``r`` decreasing where ``g > 0`` and increasing where ``g < 0``, so two corners of the box give it."""
    floor = float(F(1e-12))
    f = lambda g, r: g / np.maximum(np.sqrt(g * g + r * r), floor)
    return f(lo, np.where(lo > 0, r_hi, r_lo)), f(hi, np.where(hi > 0, r_lo, r_hi))


def check_normals(normals, points, hit, idx, c, label="") -> dict:
    """Check 5 for one level: ``normals [n, 3]`` at the kernel's own ``points [n, 3]``."""
    normals, hit = np.asarray(normals, F), np.asarray(hit, bool)
    empty = ~hit[:, None] & (normals.view(np.uint32) != 0)
    assert not empty.any(), f"{label}: the normal of an empty ray is not +0.0: {_where(empty)}"
    p = Pairs(points, idx, c)
    Mw = p.Mw()
    with np.errstate(all="ignore"):
        a, b = (p.o_lo[..., None] * Mw).astype(F), (p.o_hi[..., None] * Mw).astype(F)
        zero = F(0)
        t_lo, t_hi = np.where(p.valid[..., None], np.minimum(a, b), zero), np.where(p.valid[..., None], np.maximum(a, b), zero)
        g_lo = np.stack([sum_asc(t_lo[..., k]) for k in range(3)], 1).astype(np.float64)
        g_hi = np.stack([sum_asc(t_hi[..., k]) for k in range(3)], 1).astype(np.float64)
    held = hit & p.rows_finite & np.isfinite(g_lo).all(1) & np.isfinite(g_hi).all(1) & np.isfinite(np.where(p.valid[..., None], Mw, zero)).all((1, 2))
    no_direction = held & ((g_lo <= 0) & (g_hi >= 0)).all(1)
    held &= ~no_direction
    least = np.where((g_lo <= 0) & (g_hi >= 0), 0.0, np.minimum(np.abs(g_lo), np.abs(g_hi)))
    most = np.maximum(np.abs(g_lo), np.abs(g_hi))
    width = 0.0
    with np.errstate(all="ignore"):
        for k in range(3):
            u, v = (k + 1) % 3, (k + 2) % 3
            r_lo, r_hi = np.sqrt(least[:, u] ** 2 + least[:, v] ** 2), np.sqrt(most[:, u] ** 2 + most[:, v] ** 2)
            f_lo, f_hi = _unit_range(g_lo[:, k], g_hi[:, k], r_lo, r_hi)
            n_lo, n_hi = -f_hi, -f_lo
            pad = 8 * EPS * np.maximum(np.abs(n_lo), np.abs(n_hi))
            got = normals[:, k].astype(np.float64)
            out = held & ~((n_lo - pad <= got) & (got <= n_hi + pad))
            if out.any():
                i = int(np.argwhere(out)[0, 0])
                raise AssertionError(f"{label}: normal component {k} outside its enclosure: {_where(out)}; there {got[i]!r} not in "
                                     f"[{n_lo[i] - pad[i]!r}, {n_hi[i] + pad[i]!r}]")
            if held.any():
                width = max(width, float((n_hi - n_lo)[held].max()))
    return {"hits": int(hit.sum()), "held": int(held.sum()), "no_direction": int(no_direction.sum()), "widest": width}


def check_march(c, levels, rng, got, label="") -> dict:
    """Checks 3 to 6 on ``got = {"hit", "t", "points", "normals" or None, "densities"}`` of the case ``c`` (``origins, dirs, stds, idx,
    centers, M, strengths, density_factor``); ``rng`` is the fp32 ``range [S]`` the kernel was given."""
    o, v = np.asarray(c["origins"], F).reshape(-1, 3), np.asarray(c["dirs"], F).reshape(-1, 3)
    sd, rng = np.asarray(c["stds"], F).reshape(-1), np.asarray(rng, F).reshape(-1)
    n, S = o.shape[0], rng.shape[0]
    idx = np.asarray(c["idx"], np.int64).reshape(n, -1)
    d = np.asarray(got["densities"], F)
    assert d.shape == (n, S), f"{label}: densities {d.shape}"
    with np.errstate(all="ignore"):
        taus = rng[None, :] * sd[:, None]
        x = o[:, None, :] + taus[..., None] * v[:, None, :]
        p = Pairs(x.reshape(-1, 3), np.repeat(idx, S, axis=0), c)
        lo, hi = p.density_bounds()
        lo, hi = renorm(lo).reshape(n, S), renorm(hi).reshape(n, S)
    stats = {"densities": _check_enclosed(d, lo, hi, p.rows_finite.reshape(n, S), label, "a density of the march"),
             "hits": 0, "held": 0, "no_direction": 0, "normals_widest": 0.0}
    for l, level in enumerate(levels):
        hit, _, t = crossing_host(d, taus, level)
        bad = hit != np.asarray(got["hit"][l], bool)
        assert not bad.any(), f"{label}, level {level}: hit differs from the selection on the kernel's own densities: {_where(bad)}"
        bad = ~same(got["t"][l], t)
        assert not bad.any(), f"{label}, level {level}: t differs from the interpolation on the kernel's own densities: {_where(bad)}"
        with np.errstate(all="ignore"):
            point = np.where(hit[:, None], o + np.asarray(got["t"][l], F)[:, None] * v, F(0)).astype(F)
        bad = ~same(got["points"][l], point)
        assert not bad.any(), f"{label}, level {level}: a point is not fl(origin + fl(t dir)): {_where(bad)}"
        if got.get("normals") is not None:
            s = check_normals(got["normals"][l], got["points"][l], hit, idx, c, f"{label}, level {level}")
            for key in ("hits", "held", "no_direction"):
                stats[key] += s[key]
            stats["normals_widest"] = max(stats["normals_widest"], s["widest"])
    assert stats["no_direction"] <= SKIP_CAP * max(stats["hits"], 1), (
        f"{label}: {stats['no_direction']} of {stats['hits']} hits have a gradient box around 0: more than {SKIP_CAP:.0%} skipped")
    return stats
