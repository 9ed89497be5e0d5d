"""The two Pillow-exact resizes of ``gsr_resample.hip`` restated on the host, and the inputs and sizes they are compared on bit for bit.

``resize_rgba8_host`` and ``resize_depth_host`` follow the contract in the header of ``gsr_resample.hip`` step by step: the per-axis
tables in Python doubles (the doubles Pillow's C code uses), everything per pixel in numpy integers.  Neither imports torch or Pillow:
``test_resample.py`` holds them to Pillow's ``Image.resize`` on the CPU, ``test_resample_gpu.py`` holds the kernels to them.

``wrong_variants()`` are the same restatements with ONE step replaced by a neighbouring rule (the mistakes an edit to the table code or
a rewritten kernel would make).  The CPU tests show that each of them differs from the true restatement on some ``(SIZES entry, input
kind)`` the GPU tests run, so a kernel that followed one of them would be seen.  ``identical_variants()`` holds the one listed variant
that cannot differ on any input, and says why.
"""
from __future__ import annotations

import functools
import math

import numpy as np

BITS = 32 - 8 - 2          # fraction bits of a weight (Resample.c PRECISION_BITS)


# ---- the per-axis tables: Python doubles -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def axis_table(n_in: int, n_out: int, wrong: str | None = None):
    """``(ksize, bounds [n_out, 2] (first input index, tap count), weights [n_out, n_in] int64)`` of one bilinear pass over a whole
    axis (Resample.c precompute_coeffs + normalize_coeffs_8bpc, support 1.0).  The weights are laid out densely over the input axis
    (zero outside an output pixel's taps), which is what a pass multiplies by."""
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    half = 0.0 if wrong == "bounds-no-half" else 0.5
    bounds = np.zeros((n_out, 2), np.int64)
    weights = np.zeros((n_out, n_in), np.int64)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        ss = 1.0 / filterscale
        xmin = max(int(center - support + half), 0)
        count = min(int(center + support + half), n_in) - xmin
        assert count <= ksize
        k, ww = [], 0.0
        for x in range(count):
            t = abs((x + xmin - center + 0.5) * ss)
            w = 1.0 - t if t < 1.0 else 0.0           # the triangle filter: never negative
            k.append(w)
            ww += w
        for x, w in enumerate(k):
            if ww != 0.0 and wrong != "weights-unnormalised":
                w = w / ww
            weights[xx, xmin + x] = int(w * (1 << BITS)) if wrong == "weights-truncated" else int(0.5 + w * (1 << BITS))
        bounds[xx] = (xmin, count)
    return ksize, bounds, weights


@functools.lru_cache(maxsize=None)
def nearest_index(n_in: int, n_out: int, wrong: str | None = None) -> np.ndarray:
    """Source index of every output pixel of a NEAREST resize over a whole axis (Geometry.c ImagingScaleAffine: the source
    coordinate is ACCUMULATED in double, ``xo = a / 2`` then ``xo += a``)."""
    a = n_in / n_out
    index = np.zeros(n_out, np.int64)
    xo = a * 0.5
    for x in range(n_out):
        index[x] = int(math.floor((x + 0.5) * a)) if wrong == "nearest-multiplied" else int(xo)
        xo += a
    assert index.min() >= 0 and index.max() < n_in     # (never outside for a whole-image resize)
    return index


# ---- the per-pixel steps: numpy integers -----------------------------------------------------------------------------------------
def premultiply(c, a):
    """Convert.c MULDIV255."""
    t = c * a + 128
    return ((t >> 8) + t) >> 8


def _pass(pix: np.ndarray, weights: np.ndarray, axis: int, round_to_8_bits: bool = True) -> np.ndarray:
    """One pass along ``axis`` of ``pix`` [H, W, 4] int64: ``clip8((2^21 + sum k_i p_i) >> 22)`` per output pixel and channel."""
    s = np.einsum("ox,yxc->yoc" if axis == 1 else "oy,yxc->oxc", weights, pix)
    if not round_to_8_bits:
        return s
    return np.clip(((1 << (BITS - 1)) + s) >> BITS, 0, 255)


def _resize_rgba8(image: np.ndarray, size_wh, wrong: str | None = None, stats: dict | None = None) -> np.ndarray:
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] == 4
    W, H = int(size_wh[0]), int(size_wh[1])
    Hs, Ws = image.shape[:2]
    assert W > 0 and H > 0 and Hs > 0 and Ws > 0
    if (Hs, Ws) == (H, W):
        return image.copy()                                          # Image.resize returns a copy: no premultiply round trip
    horizontal, vertical = Ws != W, Hs != H
    round_trip = not (wrong == "one-axis-no-premultiply" and horizontal != vertical)
    pix = image.astype(np.int64)
    if round_trip:                                                   # RGBA -> RGBa
        a = pix[..., 3:]
        pix[..., :3] = pix[..., :3] * a // 255 if wrong == "premultiply-div255" else premultiply(pix[..., :3], a)
    tx = axis_table(Ws, W, wrong)[2] if horizontal else None
    ty = axis_table(Hs, H, wrong)[2] if vertical else None
    if horizontal and vertical and wrong == "no-rounding-between-passes":
        s = _pass(_pass(pix, tx, 1, round_to_8_bits=False), ty, 0, round_to_8_bits=False)
        pix = np.clip(((1 << (2 * BITS - 1)) + s) >> (2 * BITS), 0, 255)
    elif horizontal and vertical and wrong == "vertical-first":
        pix = _pass(_pass(pix, ty, 0), tx, 1)
    else:
        if horizontal:                                               # horizontal pass first; a pass whose size stays is skipped
            pix = _pass(pix, tx, 1)
        if vertical:
            pix = _pass(pix, ty, 0)
    if round_trip:                                                   # RGBa -> RGBA
        a = pix[..., 3:]
        straight = (a == 0) if wrong == "unpremultiply-at-255" else (a == 0) | (a == 255)
        safe = np.where(a == 0, 1, a)
        q = (255 * pix[..., :3] + safe // 2) // safe if wrong == "unpremultiply-rounded" else 255 * pix[..., :3] // safe
        if stats is not None:
            divided = np.broadcast_to(~((a == 0) | (a == 255)), q.shape)
            stats["divided"] = stats.get("divided", 0) + int(divided.sum())
            stats["max_quotient"] = max(stats.get("max_quotient", 0), int(q[divided].max()) if divided.any() else 0)
        pix[..., :3] = np.where(straight, pix[..., :3], np.minimum(255, q))
    return pix.astype(np.uint8)


def _resize_depth(depth: np.ndarray, size_wh, wrong: str | None = None) -> np.ndarray:
    depth = np.asarray(depth)
    assert depth.dtype == np.float32 and depth.ndim == 2
    W, H = int(size_wh[0]), int(size_wh[1])
    Hs, Ws = depth.shape
    assert W > 0 and H > 0 and Hs > 0 and Ws > 0
    if (Hs, Ws) == (H, W):
        return depth.copy()
    bits = depth.view(np.uint32)                                     # a gather of 32-bit words: NaN payloads and -0.0 as they are
    return np.ascontiguousarray(bits[nearest_index(Hs, H, wrong)][:, nearest_index(Ws, W, wrong)]).view(np.float32)


def resize_rgba8_host(image: np.ndarray, size_wh, stats: dict | None = None) -> np.ndarray:
    """``np.array(Image.fromarray(image).resize(size_wh, Image.BILINEAR))`` for an RGBA8 ``[H, W, 4]`` array.  ``stats`` collects
    ``divided`` (channels that went through ``255 c / a``) and ``max_quotient`` (the largest such quotient BEFORE the clamp)."""
    return _resize_rgba8(image, size_wh, None, stats)


def resize_depth_host(depth: np.ndarray, size_wh) -> np.ndarray:
    """``np.array(Image.fromarray(depth).resize(size_wh, Image.NEAREST))`` for a float32 ``[H, W]`` array, bit for bit."""
    return _resize_depth(depth, size_wh)


_WRONG_RGBA8 = ("bounds-no-half",                 # xmin / xmax truncated without the + 0.5
                "weights-truncated",              # (int)(w 2^22) without the + 0.5
                "weights-unnormalised",           # an output pixel's weights not divided by their sum
                "premultiply-div255",             # c a / 255 instead of MULDIV255
                "unpremultiply-rounded",          # (255 c + a / 2) / a instead of the truncating division
                "one-axis-no-premultiply",        # the premultiply round trip skipped when only one axis changes
                "vertical-first",                 # the vertical pass before the horizontal one
                "no-rounding-between-passes")     # the horizontal pass's sums handed on at full precision
_WRONG_DEPTH = ("nearest-multiplied",)            # floor((x + 0.5) a) instead of the accumulated coordinate


def wrong_variants() -> dict:
    """``{name: (what, resize)}``: ``what`` is ``"rgba8"`` or ``"depth"``, ``resize(array, size_wh)`` the restatement with that one
    step wrong."""
    out = {name: ("rgba8", functools.partial(_resize_rgba8, wrong=name)) for name in _WRONG_RGBA8}
    out.update({name: ("depth", functools.partial(_resize_depth, wrong=name)) for name in _WRONG_DEPTH})
    return out


def identical_variants() -> dict:
    """A variant of the same form that is NOT wrong: the un-premultiply also applied at ``a == 255`` computes ``255 c / 255``, which is
    ``c`` for every byte, so no input tells it from the contract (``a == 255`` is a shortcut, not a rule; ``a == 0`` is the one that
    guards a division).  It is kept here so that the equality is asserted instead of assumed."""
    return {"unpremultiply-at-255": ("rgba8", functools.partial(_resize_rgba8, wrong="unpremultiply-at-255"))}


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
KINDS = ("noise", "a0", "a255", "a1", "a254", "white", "white_varied_alpha", "checker", "alpha_steps")
ALPHA_STEPS = np.array([0, 1, 2, 127, 128, 253, 254, 255], np.uint8)


def image(kind: str, h: int, w: int, seed: int) -> np.ndarray:
    """An RGBA8 ``[h, w, 4]`` image of a named kind."""
    g = np.random.default_rng(seed)
    img = g.integers(0, 256, (h, w, 4), dtype=np.uint8)
    if kind == "noise":                       # alpha 0 / 255 on about a third of the pixels each
        img[g.random((h, w)) < 0.33, 3] = 0
        img[g.random((h, w)) < 0.33, 3] = 255
    elif kind in ("a0", "a255", "a1", "a254"):
        img[..., 3] = int(kind[1:])
    elif kind == "white":
        img[:] = 255
    elif kind == "white_varied_alpha":
        img[..., :3] = 255
    elif kind == "checker":
        img[:] = (((np.arange(h)[:, None] + np.arange(w)[None, :]) & 1) * 255).astype(np.uint8)[..., None]
    elif kind == "alpha_steps":
        img[..., 3] = ALPHA_STEPS[g.integers(0, len(ALPHA_STEPS), (h, w))]
    else:
        raise KeyError(kind)
    return img


# quiet NaNs with payloads of either sign, both infinities, -0.0, the smallest denormal and the largest negative one
DEPTH_BITS = np.array([0x7fc00001, 0xffc12345, 0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0x807fffff], np.uint32)


def depth(h: int, w: int, seed: int) -> np.ndarray:
    """A float32 ``[h, w]`` map, uniform in 0.5 .. 30, every fifth element replaced in turn by one of ``DEPTH_BITS``."""
    d = np.random.default_rng(seed).uniform(0.5, 30.0, (h, w)).astype(np.float32)
    flat = d.reshape(-1).view(np.uint32)
    at = np.arange(0, flat.size, 5)
    flat[at] = DEPTH_BITS[np.arange(len(at)) % len(DEPTH_BITS)]
    return d


def bits(x: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ---- sizes: (src_hw, dst_hw), the smallest shapes that reach each path -------------------------------------------------------------
SIZES = [
    ((3, 255), (3, 256)), ((3, 256), (3, 255)), ((2, 257), (2, 256)), ((2, 513), (2, 257)),   # the 256-lane x-block edge, horizontal only
    ((2, 600), (2, 1)), ((600, 2), (1, 2)),                                                    # ksize 1201 in each pass alone
    ((1, 1), (7, 300)), ((2, 3), (300, 2)),                                                    # up-scaling: ksize 3, taps cut at the borders
    ((9, 8), (9, 7)), ((9, 8), (7, 8)),                                                        # a ratio just above 1, one axis only
    ((8, 12), (6, 18)), ((12, 9), (18, 11)), ((16, 15), (15, 16)),                             # down on one axis, up on the other
    ((5, 7), (1, 1)), ((1, 1), (4, 6)), ((31, 17), (31, 17)),                                  # to one pixel, from one pixel, the identity
    ((40, 64), (20, 32)), ((45, 96), (15, 32)), ((30, 90), (20, 60)),                          # the exact ratios 2, 3 and 1.5
]
# axis pairs of SIZES on which the accumulated and the multiplied nearest coordinate give different indices
NEAREST_TELLING_PAIRS = [(256, 255), (8, 7), (8, 6), (12, 18), (16, 15)]


def size_id(src_hw, dst_hw) -> str:
    return f"{src_hw[0]}x{src_hw[1]}-{dst_hw[0]}x{dst_hw[1]}"


def case_seed(src_hw, dst_hw, kind: str = "") -> int:
    return (src_hw[0] * 7 + src_hw[1] * 131 + dst_hw[0] * 17 + dst_hw[1] * 1009 + sum(map(ord, kind))) % (1 << 31)


def axis_pairs(src_hw, dst_hw, what: str) -> set:
    """The ``(in, out, kind)`` tables a resize of this size asks the library for (kind 0: bilinear weights, 1: nearest indices)."""
    if tuple(src_hw) == tuple(dst_hw):
        return set()
    pairs = {(src_hw[1], dst_hw[1]), (src_hw[0], dst_hw[0])}
    if what == "rgba8":
        return {(i, o, 0) for i, o in pairs if i != o}
    return {(i, o, 1) for i, o in pairs}


# ---- the GPU sweep: few enough axis pairs that the tables the library keeps for them stay small -----------------------------------
SWEEP_MAX_PAIRS = 150      # every new (in, out, kind) leaves a small device allocation the library never frees
SWEEP_OUT_WIDTHS = (255, 256, 257)


def gpu_sweep(seed: int = 20240613, n: int = SWEEP_MAX_PAIRS):
    """``[(src_hw, dst_hw)]``: ``n`` axis pairs drawn from 1 .. 300 as widths, the output widths 255, 256 and 257 among them, with 2
    or 3 rows on either side."""
    g = np.random.default_rng(seed)
    pairs = [(int(g.integers(1, 301)), w) for w in SWEEP_OUT_WIDTHS]
    while len(pairs) < n:
        p = (int(g.integers(1, 301)), int(g.integers(1, 301)))
        if p not in pairs:
            pairs.append(p)
    return [((int(g.integers(2, 4)), i), (int(g.integers(2, 4)), o)) for i, o in pairs]
