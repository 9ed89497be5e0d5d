"""The quadrant reach test as a minimum over two lines (gsr_device.h: splat_reaches_rect), without a GPU.

The four-edge form took the minimum of q over the rectangle's four edges after a separate centre-inside test; the two-line form
takes it over the vertical and the horizontal line through the rectangle's point nearest the centre, the only edges that can hold
it.  tests/reach_lines_model.py restates both in numpy fp32, operation for operation.

  (a) over 1.2 M fixed-seed finite cases and hand-made ones the two predicates agree except where the contract allows it:
        1. the rounding of qmin straddles the threshold: the two minima are the same number up to the fp32 rounding of q,
           8e-7 (1 + |rho|) / (1 - |rho|) relative between the two (the comparison's margin is 2e-3 relative + 1e-3);
        2. the centre is inside the rectangle and the budget ln(255 o) is below -1e-3: alpha < 1/255 even at the centre;
      both are counted and printed;
  (b) soundness against the fp64 truth: wherever one of the rectangle's 64 pixel centres has o exp(-q) >= 1/255, the two-line
      predicate keeps the entry -- no allowance;
  (c) NaN and +-inf in every operand, one at a time and combined: the two-line form keeps every entry the four-edge form kept;
  (d) from the cross-compiled gfx950 assembly: both blend kernels keep <= 64 vector registers, no scratch and their LDS bytes, and
      the vector instructions of a batch's staging (scripts/blend_isa_census.py: staging_census) are at least 25 fewer than the
      155 / 158 the four-edge form compiled to.
"""
import itertools
import os
import sys

import numpy as np

import reach_lines_model as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
ORIGINS = ((0, 0), (8, 8), (1912, 1072))
OPACITIES = (1.0 / 255.0, 1.0, 1.5, np.inf)


def random_cases(n, seed):
    """Conics built the way the projection builds them (isotropic blobs to 1000:1 needles, every angle), centres within 40 pixels
    of an 8 x 8 rectangle (a third of them on integer coordinates), opacities from 1e-3 to 1 and the four special ones."""
    g = np.random.default_rng(seed)
    major = np.exp(g.uniform(np.log(0.3), np.log(300.0), n))
    minor = major * np.exp(-g.uniform(0.0, np.log(1000.0), n) * (g.random(n) < 0.7))
    A, B, C = m.conic_of(major, minor, g.uniform(0.0, np.pi, n))
    o = np.exp(g.uniform(np.log(1.0e-3), 0.0, n))
    pick = g.integers(0, 12, n)
    for k, v in enumerate(OPACITIES):
        o[pick == k] = v
    org = np.asarray(ORIGINS)[g.integers(0, len(ORIGINS), n)]
    cx, cy = org[:, 0] + g.uniform(-40.0, 48.0, n), org[:, 1] + g.uniform(-40.0, 48.0, n)
    snap = g.random(n) < 1.0 / 3.0
    cx[snap], cy[snap] = np.round(cx[snap]), np.round(cy[snap])
    return m.f32(A, B, C, o, cx, cy) + (org[:, 0], org[:, 1])


def hand_made_cases():
    """Every opacity x every centre position x a family of conics, against the rectangle at (8, 8):
    centres on each edge and corner pixel, inside, and in the eight regions outside (near and far);
    conics: isotropic, correlations up to the 0.99 guard on both sides (rho^2 = 0.9899 and 0.9901), 1000:1 needles at +-45 degrees
    (they cross a corner diagonally: the case a single nearest edge gets wrong) and at shallow angles."""
    x0 = y0 = 8
    inside = [(11.0, 12.0), (8.0, 8.0), (15.0, 15.0), (8.0, 15.0), (15.0, 8.0), (8.0, 11.0), (15.0, 11.0), (11.0, 8.0), (11.0, 15.5 - 0.5),
              (11.25, 12.75), (8.0 + 2.0 ** -20, 15.0 - 2.0 ** -20)]
    outside = []
    for dx, dy in itertools.product((-1, 0, 1), repeat=2):
        if dx == dy == 0:
            continue
        for dist in (2.0 ** -18, 0.5, 1.0, 3.25, 9.0, 40.0):
            px = 11.5 if dx == 0 else (8.0 - dist if dx < 0 else 15.0 + dist)
            py = 11.5 if dy == 0 else (8.0 - dist if dy < 0 else 15.0 + dist)
            outside.append((px, py))
    # needles past a corner: the centre diagonal from a corner, shifted along the anti-diagonal so the needle just crosses / misses it
    for corner, sgn in (((8.0, 8.0), 1), ((15.0, 8.0), -1), ((8.0, 15.0), -1), ((15.0, 15.0), 1)):
        for along in (-30.0, -6.0, 6.0, 30.0):
            for off in (0.0, 0.4, 1.0, 2.5):
                outside.append((corner[0] + along + off, corner[1] + sgn * along - sgn * off))
    centres = np.asarray(inside + outside)
    conics = []
    for s in (0.5, 2.0, 8.0, 60.0):
        conics.append(m.conic_of(s, s, 0.0))
    for rho2 in (0.5, 0.9, 0.98, 0.9899, 0.9901):
        for sign in (1.0, -1.0):
            for a, c in ((0.3, 0.3), (2.0, 0.02), (0.01, 0.5)):
                conics.append(m.f32(a, sign * np.sqrt(rho2 * a * c), c))
    for ang in (np.pi / 4, -np.pi / 4, 0.05, np.pi / 2 - 0.05, 1.0):
        for major in (20.0, 300.0, 3000.0):
            conics.append(m.conic_of(major, major / 1000.0, ang))
    conics = np.asarray([[float(v) for v in c] for c in conics], F)
    opac = np.asarray(OPACITIES + (0.004, 0.05, 0.6), F)
    ci, ki, oi = (a.reshape(-1) for a in np.meshgrid(np.arange(len(centres)), np.arange(len(conics)), np.arange(len(opac)), indexing="ij"))
    n = len(ci)
    return (conics[ki, 0], conics[ki, 1], conics[ki, 2], opac[oi], centres[ci, 0].astype(F), centres[ci, 1].astype(F),
            np.full(n, x0), np.full(n, y0))


_FINITE = {}


def finite_cases():
    if not _FINITE:
        parts = [random_cases(1_200_000, 20241), hand_made_cases()]
        _FINITE["cases"] = tuple(np.concatenate([p[i] for p in parts]) for i in range(8))
    return _FINITE["cases"]


def test_two_lines_agree_with_four_edges_except_where_the_contract_allows():
    A, B, C, o, cx, cy, x0, y0 = finite_cases()
    skip = m.skip_below_of(o)
    old, q_old, inside = m.reach_edges(A, B, C, skip, cx, cy, x0, y0)
    new, q_new = m.reach_lines(A, B, C, skip, cx, cy, x0, y0)
    regular = (A > 0) & (C > 0) & ((B * B) < F(0.99) * (A * C))
    assert len(A) >= 1_000_000 and regular.mean() > 0.5 and (~regular).sum() > 1000
    assert (new[~regular] & old[~regular]).all(), "an irregular conic is never culled"
    budget = -skip - F(1.0e-4)
    # The two minima are the same number wherever the centre is outside the rectangle, each within the fp32 rounding of q that
    # gsr_device.h states for the predicate's margin: 4e-7 (1 + |rho|) / (1 - |rho|) relative, |rho| < 0.995 behind the guard.
    out = regular & ~inside
    rho = np.sqrt(np.minimum((B[out].astype(np.float64) ** 2) / (A[out].astype(np.float64) * C[out]), 0.99))
    bound = 2.0 * 4.0e-7 * (1.0 + rho) / (1.0 - rho)
    rel = np.abs(q_new[out].astype(np.float64) - q_old[out]) / np.maximum(q_old[out].astype(np.float64), 1e-30)
    print(f"{int(out.sum())} regular cases with the centre outside: two-line against four-edge minimum, worst relative difference {rel.max():.3g}, "
          f"worst share of the rounding bound {(rel / bound).max():.3g}")
    assert (rel <= bound).all()
    assert (q_new[regular & inside] == 0).all(), "a centre inside the rectangle gives q = 0 on both lines"
    differ = new != old
    allowed_inside = differ & regular & inside & (budget < F(-1.0e-3)) & old & ~new
    straddle = differ & out   # (the minima agree to their rounding, asserted above: only that can separate the predicates)
    print(f"{len(A)} cases, {int(old.sum())} kept by four edges, {int(new.sum())} by two lines; they differ on {int(differ.sum())}: "
          f"{int(straddle.sum())} by the rounding of qmin at the threshold, {int(allowed_inside.sum())} with the centre inside and alpha < 1/255 there")
    assert not (differ & ~allowed_inside & ~straddle).any()
    faint_inside = regular & inside & (budget < F(-1.0e-3))
    assert faint_inside.sum() > 0 and not new[faint_inside].any() and old[faint_inside].all()
    bright_inside = regular & inside & ~(budget < F(-1.0e-3))
    assert bright_inside.sum() > 1000 and new[bright_inside].all()


def test_two_lines_never_drop_an_entry_that_reaches_a_pixel_in_fp64():
    A, B, C, o, cx, cy, x0, y0 = finite_cases()
    new, _ = m.reach_lines(A, B, C, m.skip_below_of(o), cx, cy, x0, y0)
    visible = np.zeros(len(A), bool)
    with np.errstate(all="ignore"):
        for s in range(0, len(A), 100_000):
            sl = slice(s, s + 100_000)
            alpha = o[sl].astype(np.float64)[:, None] * np.exp(-m.q64(A[sl], B[sl], C[sl], cx[sl], cy[sl], x0[sl], y0[sl]))
            visible[sl] = (alpha >= 1.0 / 255.0).any(1)
    print(f"{int(visible.sum())} of {len(A)} cases reach a pixel; the predicate keeps {int(new.sum())}, drops {int((visible & ~new).sum())} of those that reach")
    assert visible.sum() > 100_000 and (~new).sum() > 100_000
    assert not (visible & ~new).any()


def test_non_finite_operands_never_drop_what_four_edges_kept():
    """Fields: centre x, y, conic A, B, C, skip_below itself, and the opacity skip_below is computed from."""
    g = np.random.default_rng(7)
    A, B, C, o, cx, cy, x0, y0 = (v[:4000] for v in random_cases(4000, 99))
    hand = hand_made_cases()
    sel = g.choice(len(hand[0]), 4000, replace=False)
    base = [np.concatenate((a, h[sel])) for a, h in zip((A, B, C, o, cx, cy, x0, y0), hand)]
    n = len(base[0])
    special = (np.nan, np.inf, -np.inf)
    checked = kept_more = 0

    def check(fields, values):
        nonlocal checked, kept_more
        A, B, C, o, cx, cy, x0, y0 = (v.copy() for v in base)
        skip = m.skip_below_of(o)
        arrays = {"cx": cx, "cy": cy, "A": A, "B": B, "C": C, "skip": skip}
        for f, v in zip(fields, values):
            if f == "opacity":
                skip[:] = m.skip_below_of(np.full(n, v, F))
            else:
                arrays[f][:] = v
        old, _, _ = m.reach_edges(A, B, C, skip, cx, cy, x0, y0)
        new, _ = m.reach_lines(A, B, C, skip, cx, cy, x0, y0)
        lost = old & ~new
        assert not lost.any(), (fields, values, int(lost.sum()), [float(a[lost][0]) for a in (A, B, C, skip, cx, cy)])
        checked += n
        kept_more += int((new & ~old).sum())

    names = ("cx", "cy", "A", "B", "C", "skip", "opacity")
    for f in names:
        for v in special + ((0.0, -1.0) if f in ("A", "C", "opacity") else ()):   # (an opacity or a conic diagonal of 0 or below too)
            check((f,), (v,))
    for f1, f2 in itertools.combinations(names, 2):
        for v1, v2 in itertools.product(special, repeat=2):
            check((f1, f2), (v1, v2))
    for k in (3, 4, 5, 6):
        for fields in itertools.combinations(names[:6], k):
            for values in ((np.nan,) * k, (np.inf,) * k, (-np.inf,) * k, tuple(special[i % 3] for i in range(k))):
                check(fields, values)
    print(f"{checked} cases with non-finite operands; two lines keep {kept_more} the four edges dropped, drop none they kept")


def _scripts(name):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        return __import__(name)
    finally:
        sys.path.pop(0)


PARENT_STAGING_VALU = {"blend_quadrant_kernelILb0": 155, "blend_quadrant_kernelILb1": 158}   # the four-edge form, same census


def test_blend_kernels_keep_their_resources_and_stage_a_batch_in_25_fewer_vector_instructions():
    from autovfx_amd import build
    from blend_terms_scenes import SLOTS, SLOTS_EXTRA
    census, blend = _scripts("kernel_isa_census"), _scripts("blend_isa_census")
    asm = census.assembly(build.CSRC, "gsr_blend.hip")
    lds = {"blend_quadrant_kernelILb0": SLOTS * 152 + SLOTS * 4, "blend_quadrant_kernelILb1": SLOTS_EXTRA * 152 + SLOTS_EXTRA * 16}
    for part, before in PARENT_STAGING_VALU.items():
        c = census.census(asm, part)
        staging = blend.staging_census("\n".join(asm), part)
        print(part, {k: c[k] for k in ("vgpr", "sgpr", "lds_bytes", "scratch")}, "staging per batch:", staging)
        assert c["scratch"] == 0 and 0 < c["vgpr"] <= 64 and c["lds_bytes"] == lds[part]
        assert staging["VALU"] <= before - 25, f"{part}: {staging['VALU']} vector instructions per staged batch, {before} before"
