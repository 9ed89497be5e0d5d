"""The host restatements of the two Pillow-exact resizes (resample_cases.py) held to Pillow's Image.resize itself, byte for byte, and
the coverage their cases claim: every deliberately wrong restatement differs from the true one on a case the GPU tests run."""
from __future__ import annotations

import numpy as np
import pytest

import resample_cases as cases
from resample_cases import KINDS, SIZES, bits, case_seed, size_id

Image = pytest.importorskip("PIL.Image")


def pil_rgba8(img, size_wh):
    return np.array(Image.fromarray(img).resize(size_wh, resample=Image.BILINEAR))


def pil_depth(d, size_wh):
    return np.array(Image.fromarray(d).resize(size_wh, Image.NEAREST))


def _wh(hw):
    return (hw[1], hw[0])


@pytest.mark.parametrize("src_hw,dst_hw", SIZES, ids=[size_id(*s) for s in SIZES])
def test_restatements_equal_pillow_on_every_size_and_kind(src_hw, dst_hw):
    for kind in KINDS:
        img = cases.image(kind, *src_hw, case_seed(src_hw, dst_hw, kind))
        got = cases.resize_rgba8_host(img, _wh(dst_hw))
        assert got.dtype == np.uint8 and got.shape == dst_hw + (4,)
        np.testing.assert_array_equal(got, pil_rgba8(img, _wh(dst_hw)), err_msg=kind)
    d = cases.depth(*src_hw, case_seed(src_hw, dst_hw))
    got = cases.resize_depth_host(d, _wh(dst_hw))
    assert got.dtype == np.float32 and got.shape == dst_hw
    np.testing.assert_array_equal(bits(got), bits(pil_depth(d, _wh(dst_hw))))


def test_named_inputs_are_what_they_say():
    img = {k: cases.image(k, 24, 40, 3) for k in KINDS}
    for k, a in (("a0", 0), ("a255", 255), ("a1", 1), ("a254", 254)):
        assert (img[k][..., 3] == a).all() and len(np.unique(img[k][..., :3])) > 200
    assert (img["white"] == 255).all()
    assert (img["white_varied_alpha"][..., :3] == 255).all() and len(np.unique(img["white_varied_alpha"][..., 3])) > 200
    assert set(np.unique(img["checker"])) == {0, 255} and (img["checker"][0, 0] == 0).all() and (img["checker"][0, 1] == 255).all()
    assert (img["checker"] == img["checker"][..., :1]).all()
    assert set(np.unique(img["alpha_steps"][..., 3])) == set(cases.ALPHA_STEPS.tolist())
    frac = [(img["noise"][..., 3] == a).mean() for a in (0, 255)]
    assert all(0.15 < f < 0.5 for f in frac)
    d = cases.depth(9, 11, 5)
    flat = bits(d).reshape(-1)
    assert np.array_equal(flat[::5][:14], np.tile(cases.DEPTH_BITS, 2))
    rest = np.delete(d.reshape(-1), np.arange(0, d.size, 5))
    assert np.isfinite(rest).all() and rest.min() >= 0.5 and rest.max() <= 30.0
    # the smallest image that gets depth() (1 x 1) holds a NaN payload; every 2-row image of the sizes holds all seven patterns
    assert bits(cases.depth(1, 1, 0))[0, 0] == cases.DEPTH_BITS[0]
    assert set(cases.DEPTH_BITS.tolist()) <= set(bits(cases.depth(2, 257, 0)).reshape(-1).tolist())


def test_sizes_reach_the_paths_they_are_listed_for():
    ksize = lambda i, o: cases.axis_table(i, o)[0]
    assert ksize(600, 1) == 1201 and ksize(1, 300) == 3 and ksize(3, 2) == 5 and ksize(8, 7) == 5 and ksize(64, 32) == 5 and ksize(96, 32) == 7
    widths = {dst[1] for _, dst in SIZES}
    assert {255, 256, 257} <= widths                                   # one full x-block less a lane, exactly one, one and a lane
    both = [(s, d) for s, d in SIZES if s[0] != d[0] and s[1] != d[1]]
    one = [(s, d) for s, d in SIZES if (s[0] != d[0]) != (s[1] != d[1])]
    assert len(both) >= 6 and len(one) >= 8 and ((31, 17), (31, 17)) in SIZES
    assert ((16, 15), (15, 16)) in SIZES                               # its vertical table is its horizontal one transposed
    # taps cut at both borders when up-scaling: the first and the last output pixel have fewer taps than the middle ones
    _, bounds, _ = cases.axis_table(2, 300)
    assert bounds[0, 1] < bounds[150, 1] and bounds[-1, 1] < bounds[150, 1]
    # the nearest coordinate: these axis pairs of SIZES tell accumulation from multiplication
    axis = {(s[i], d[i]) for s, d in SIZES for i in (0, 1)}
    for i, o in cases.NEAREST_TELLING_PAIRS:
        assert (i, o) in axis
        assert not np.array_equal(cases.nearest_index(i, o), cases.nearest_index(i, o, "nearest-multiplied")), (i, o)


def test_restatements_equal_pillow_on_a_sweep_of_axis_pairs():
    """Every axis pair ``in, out`` in 1 .. 40, on the horizontal and on the vertical axis, the other axis at random sizes 1 .. 8.

    The un-premultiply's ``min(255, ...)`` is asserted unreachable on the way: a premultiplied channel never exceeds its alpha
    (MULDIV255(c, a) <= a), and both go through the same non-negative weights and the same monotonic rounding, so ``c <= a`` holds
    after every pass and ``255 c / a <= 255``.  No input covers the clamp; none is sought."""
    g = np.random.default_rng(40)
    stats, n = {}, 0
    for n_in in range(1, 41):
        for n_out in range(1, 41):
            for axis in (0, 1):
                r_in, r_out = int(g.integers(1, 9)), int(g.integers(1, 9))
                src_hw, dst_hw = ((r_in, n_in), (r_out, n_out)) if axis else ((n_in, r_in), (n_out, r_out))
                kind = KINDS[n % len(KINDS)]
                img = cases.image(kind, *src_hw, n)
                want = pil_rgba8(img, _wh(dst_hw))
                got = cases.resize_rgba8_host(img, _wh(dst_hw), stats)
                assert np.array_equal(got, want), (src_hw, dst_hw, kind)
                d = cases.depth(*src_hw, n)
                assert np.array_equal(bits(cases.resize_depth_host(d, _wh(dst_hw))), bits(pil_depth(d, _wh(dst_hw)))), (src_hw, dst_hw)
                n += 1
    assert n == 3200 and stats["divided"] > 100_000
    assert stats["max_quotient"] <= 255
    assert stats["max_quotient"] == 255        # (reached, never passed: the sweep does look at the quotients it is asked about)


def test_the_designed_cases_never_reach_the_unpremultiply_clamp():
    stats = {}
    for src_hw, dst_hw in SIZES:
        for kind in KINDS:
            cases.resize_rgba8_host(cases.image(kind, *src_hw, case_seed(src_hw, dst_hw, kind)), _wh(dst_hw), stats)
    assert stats["divided"] > 10_000 and stats["max_quotient"] <= 255


def _tells(name, what, wrong):
    """The ``(size, kind)`` cases of the GPU tests on which ``wrong`` differs from the true restatement."""
    seen = []
    for src_hw, dst_hw in SIZES:
        if what == "depth":
            d = cases.depth(*src_hw, case_seed(src_hw, dst_hw))
            if not np.array_equal(bits(wrong(d, _wh(dst_hw))), bits(cases.resize_depth_host(d, _wh(dst_hw)))):
                seen.append((src_hw, dst_hw, "depth"))
            continue
        for kind in KINDS:
            img = cases.image(kind, *src_hw, case_seed(src_hw, dst_hw, kind))
            if not np.array_equal(wrong(img, _wh(dst_hw)), cases.resize_rgba8_host(img, _wh(dst_hw))):
                seen.append((src_hw, dst_hw, kind))
    return seen


WRONG = cases.wrong_variants()


@pytest.mark.parametrize("name", list(WRONG))
def test_every_wrong_variant_is_caught_by_a_case_the_gpu_tests_run(name):
    what, wrong = WRONG[name]
    seen = _tells(name, what, wrong)
    assert seen, f"{name}: no (SIZES entry, input kind) tells it from the contract"
    if name == "nearest-multiplied":
        told = {(s[i], d[i]) for s, d, _ in seen for i in (0, 1)}
        assert set(cases.NEAREST_TELLING_PAIRS) <= told


def test_the_wrong_variants_are_the_listed_ones():
    assert set(WRONG) == {"nearest-multiplied", "bounds-no-half", "weights-truncated", "weights-unnormalised", "premultiply-div255",
                          "unpremultiply-rounded", "one-axis-no-premultiply", "vertical-first", "no-rounding-between-passes"}
    assert set(cases.identical_variants()) == {"unpremultiply-at-255"}


def test_unpremultiplying_at_full_alpha_is_the_identity():
    """The tenth listed variant, "the un-premultiply also applied at a == 255", is no mistake: 255 c / 255 == c for every byte, so no
    image can tell it from the contract and it cannot stand among the wrong variants.  Asserted for every byte, and on every case."""
    c = np.arange(256)
    assert np.array_equal(255 * c // 255, c)
    what, variant = cases.identical_variants()["unpremultiply-at-255"]
    assert _tells("unpremultiply-at-255", what, variant) == []


def test_the_gpu_sweep_is_capped_and_holds_the_block_edge_widths():
    sweep = cases.gpu_sweep()
    assert sweep == cases.gpu_sweep()                                   # a fixed seed: the same pairs in every process
    axis = [(s[1], d[1]) for s, d in sweep]
    assert len(axis) == len(set(axis)) <= cases.SWEEP_MAX_PAIRS == 150
    assert {255, 256, 257} <= {o for _, o in axis}
    assert all(1 <= i <= 300 and 1 <= o <= 300 for i, o in axis)
    assert all(s[0] in (2, 3) and d[0] in (2, 3) for s, d in sweep)
    for src_hw, dst_hw in sweep[:40]:                                   # (the restatement on these shapes: the first forty)
        img = cases.image("noise", *src_hw, case_seed(src_hw, dst_hw))
        assert np.array_equal(cases.resize_rgba8_host(img, _wh(dst_hw)), pil_rgba8(img, _wh(dst_hw)))
        d = cases.depth(*src_hw, case_seed(src_hw, dst_hw))
        assert np.array_equal(bits(cases.resize_depth_host(d, _wh(dst_hw))), bits(pil_depth(d, _wh(dst_hw))))
