"""Small scenes for the quadrant reach test (gsr_device.h: splat_reaches_rect as a minimum over two lines).  Around each target
quadrant (an 8 x 8 pixel block) of a 32 x 32 or a 37 x 29 image they place
  * isotropic splats with the centre inside the quadrant and in each of the eight regions outside it;
  * splats centred on the quadrant seams, x or y = 7 and 8;
  * 1000:1 needles whose centre lies diagonally off a corner of the quadrant and whose line crosses the quadrant behind that
    corner: the minimum of q is then on ONE of the two visible edges, and the other alone would drop the entry;
  * faint splats diagonally off a corner pixel whose opacity puts the 1/255 contour a few ulps either side of that pixel: the
    opacities come from the fp64 value of q there, computed from the oracle's own projection of the scene (two passes);
  * a few dozen random splats behind and between them.
`coverage` states which of these configurations the projected scene really holds, from the oracle's intermediates and the numpy
restatements of tests/reach_lines_model.py.  Shared by tests/test_reach_lines_gpu.py and tests/reach_lines_unfused_check.py."""
import numpy as np
import torch

from autovfx_amd import scenes
from autovfx_amd.scenes import GaussianCloud
from oracle import cpu_oracle

import reach_lines_model as m
from blend_terms_scenes import BG, splats
from helpers import oracle_kwargs

SIZES = ((32, 32), (37, 29))
TARGETS = {(32, 32): ((8, 8), (16, 16)), (37, 29): ((8, 8), (32, 24))}   # (the second one of 37 x 29 has lanes outside the image)
FAINT_ULPS = (-4, -2, -1, 1, 2, 4)


def _build(cam, parts, seed):
    px, py, vz, major, minor, angle, opac = (np.concatenate([np.asarray(p[i], np.float64).reshape(-1) for p in parts]) for i in range(7))
    P = len(px)
    means, _ = splats(cam, px, py, vz, major)
    focal = cam.image_width / (2.0 * cam.tanfovx)
    scales = np.stack((major * vz / focal, minor * vz / focal, minor * vz / focal), 1).astype(np.float32)
    rot = np.stack((np.cos(angle / 2), np.zeros(P), np.zeros(P), np.sin(angle / 2)), 1).astype(np.float32)   # about the view axis
    g = torch.Generator().manual_seed(seed)
    shs = torch.cat((torch.randn(P, 1, 3, generator=g), 0.2 * torch.randn(P, 15, 3, generator=g)), 1).contiguous()
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float32))
    return GaussianCloud(t(means), t(opac).reshape(P, 1), t(scales), t(rot), shs, None, 3)


def _parts(width, height, seed):
    g = np.random.default_rng(seed)
    parts, faint = [], []
    n = 0

    def add(px, py, major, minor, angle, opac, vz=None):
        nonlocal n
        k = len(np.atleast_1d(px))
        b = lambda a: np.broadcast_to(np.asarray(a, np.float64), (k,)).copy()
        parts.append((b(px), b(py), g.uniform(3.0, 6.0, k) if vz is None else b(vz), b(major), b(minor), b(angle), b(opac)))
        n += k
        return np.arange(n - k, n)

    for x0, y0 in TARGETS[(width, height)]:
        # the nine regions, two sizes each
        rx, ry = np.meshgrid((x0 - 4.7, x0 + 3.4, x0 + 11.6), (y0 - 4.4, y0 + 3.7, y0 + 12.3))
        for s, o in ((1.2, 0.7), (3.0, 0.25)):
            add(rx.reshape(-1), ry.reshape(-1), s, s, 0.0, o)
        # on the seams
        sx, sy = np.meshgrid((x0 - 1.0, x0 + 0.0, x0 + 3.0), (y0 - 1.0, y0 + 0.0, y0 + 3.0))
        add(sx.reshape(-1), sy.reshape(-1), 1.6, 1.6, 0.0, 0.4)
        # needles: the centre diagonally off each corner, the line aimed at a point of the quadrant's boundary behind the corner
        for cx, cy, ox, oy in ((x0, y0, -1, -1), (x0 + 7, y0, 1, -1), (x0, y0 + 7, -1, 1), (x0 + 7, y0 + 7, 1, 1)):
            for off, along in ((3.0, 4.5), (5.0, 2.5), (2.5, 6.0)):
                centre = np.array([cx + ox * off, cy + oy * (off + 1.3)])
                for aim in (np.array([cx - ox * along, cy + oy * 0.2]), np.array([cx + ox * 0.2, cy - oy * along])):
                    d = aim - centre
                    add(centre[0], centre[1], 14.0, 0.014, np.arctan2(d[1], d[0]), 0.8)
        # faint splats diagonally off the far corner pixel (the opacities are set in the second pass)
        for k in FAINT_ULPS:
            ids = add(x0 + 7 + 3.3 + 0.01 * k, y0 + 7 + 3.6, 2.5, 2.5, 0.0, 0.02)
            faint.append((int(ids[0]), x0 + 7, y0 + 7, k))
    add(g.uniform(0.0, width - 1.0, 40), g.uniform(0.0, height - 1.0, 40), g.uniform(0.8, 4.0, 40), g.uniform(0.8, 4.0, 40),
        g.uniform(0.0, np.pi, 40), g.choice([0.04, 0.2, 0.6], 40))
    return parts, faint


_SCENES = {}


def scene(width, height):
    """(cloud, camera, oracle forward with intermediates) of one image size, built once."""
    if (width, height) not in _SCENES:
        cam = scenes.c1_camera(width, height)
        parts, faint = _parts(width, height, seed=width)
        cloud = _build(cam, parts, seed=width)
        first = cpu_oracle.forward(intermediates=True, **oracle_kwargs(cloud, cam, bg=BG))
        for i, cx, cy, k in faint:   # opacity = exp(q at the corner pixel) / 255 in fp64, rounded to fp32, moved k ulps
            A, B, C = (first["conic_opacity"][i, j] for j in range(3))
            q = m.q64([A], [B], [C], [first["means2D"][i, 0]], [first["means2D"][i, 1]], [cx], [cy], 1, 1)[0, 0]
            o = np.float32(np.exp(q) / 255.0)
            for _ in range(abs(k)):
                o = np.nextafter(o, np.float32(2.0 if k > 0 else 0.0), dtype=np.float32)
            cloud.opacities[i, 0] = float(o)
        ref = cpu_oracle.forward(intermediates=True, **oracle_kwargs(cloud, cam, bg=BG))
        _SCENES[(width, height)] = (cloud, cam, ref)
    return _SCENES[(width, height)]


def coverage(width, height):
    """Which configurations the projected scene holds, over every (visible splat, quadrant of the image) pair."""
    cloud, cam, ref = scene(width, height)
    vis = np.nonzero(ref["radii"] > 0)[0]
    qx, qy = np.meshgrid(np.arange(0, width, 8), np.arange(0, height, 8))
    si, qi = (a.reshape(-1) for a in np.meshgrid(vis, np.arange(qx.size), indexing="ij"))
    x0, y0 = qx.reshape(-1)[qi], qy.reshape(-1)[qi]
    A, B, C, o = (ref["conic_opacity"][si, j].astype(np.float32) for j in range(4))
    cx, cy = ref["means2D"][si, 0].astype(np.float32), ref["means2D"][si, 1].astype(np.float32)
    skip = m.skip_below_of(o)
    old, _, inside = m.reach_edges(A, B, C, skip, cx, cy, x0, y0)
    new, _ = m.reach_lines(A, B, C, skip, cx, cy, x0, y0)
    q_vert, q_horz = m.line_minima(A, B, C, cx, cy, x0, y0)
    budget = -skip - np.float32(1.0e-4)
    drops = lambda q: q * np.float32(0.998) - np.float32(1.0e-3) > budget
    regular = (A > 0) & (C > 0) & ((B * B) < np.float32(0.99) * (A * C))
    region = 3 * (np.sign(np.maximum(y0 - cy, 0) - np.maximum(cy - (y0 + 7), 0)).astype(int) + 1) + \
        (np.sign(np.maximum(x0 - cx, 0) - np.maximum(cx - (x0 + 7), 0)).astype(int) + 1)
    corner = np.isin(region, (0, 2, 6, 8))
    with np.errstate(all="ignore"):
        alpha = o.astype(np.float64)[:, None] * np.exp(-m.q64(A, B, C, cx, cy, x0, y0))
    brightest = alpha.max(1) * 255.0
    seam = lambda v: np.abs(v - np.round(v)) < 1.0e-3
    return {
        "pairs": len(si), "kept": int(new.sum()), "dropped": int((~new).sum()), "predicates_differ": int((old != new).sum()),
        "regions_kept": sorted(set(region[new & regular].tolist())), "regions_dropped": sorted(set(region[~new].tolist())),
        "needle_only_horizontal_line_keeps": int((corner & regular & new & drops(q_vert) & ~drops(q_horz)).sum()),
        "needle_only_vertical_line_keeps": int((corner & regular & new & ~drops(q_vert) & drops(q_horz)).sum()),
        "contour_just_includes_a_pixel": int(((brightest >= 1.0) & (brightest < 1.0 + 2.0e-6)).sum()),
        "contour_just_misses_every_pixel": int(((brightest < 1.0) & (brightest > 1.0 - 2.0e-6)).sum()),
        "centres_on_a_seam_x": int((seam(cx) & np.isin(np.round(cx) % 8, (7, 0))).sum()),
        "centres_on_a_seam_y": int((seam(cy) & np.isin(np.round(cy) % 8, (7, 0))).sum()),
        "centre_inside": int(inside.sum()), "reaches_a_pixel_but_dropped": int(((brightest >= 1.0) & ~new).sum()),
    }


def assert_coverage(width, height):
    c = coverage(width, height)
    print(f"{width}x{height}:", c)
    assert c["regions_kept"] == list(range(9)) and len(c["regions_dropped"]) == 8, c   # (a centre inside is never dropped here)
    assert c["needle_only_horizontal_line_keeps"] > 0 and c["needle_only_vertical_line_keeps"] > 0, c
    assert c["contour_just_includes_a_pixel"] > 0 and c["contour_just_misses_every_pixel"] > 0, c
    assert c["centres_on_a_seam_x"] > 0 and c["centres_on_a_seam_y"] > 0 and c["centre_inside"] > 0, c
    assert c["reaches_a_pixel_but_dropped"] == 0 and c["dropped"] > c["kept"] // 4, c
    return c
