"""What gives tests/test_panorama_seams_gpu.py its teeth, on the CPU (tests/panorama_cases.py holds the bound and the comparison):

* the noise case (S 7, 65 x 264) reaches every class of the padded map -- face type x {row pad, column pad, both} -- and the zero
  corners of the up / down faces with taps that carry weight; the second pads (index S + 1) never carry any, at any case size;
* every single wrong entry of the padded map, 90 of them, is rejected by ``check`` at that case;
* ``check`` passes the reference's own output; ``E`` stays below 2 x 2^-24 at every case size (a guard on the choice of sizes,
  not a limit on the kernel).
"""
import contextlib
import io
from unittest import mock

import numpy as np
import pytest

import panorama_cases as cases
from autovfx_amd import panorama as pano

S7 = cases.TAP_CASES[0]
HEAVY = 1.0 / 8


@pytest.mark.parametrize("S,h,w", cases.SIZES, ids=lambda n: str(n))
def test_reference_coordinates_are_close_to_the_truth(S, h, w):
    e = cases.E(S, h, w)
    print(f"S {S} {h}x{w}: E = {e / cases.ULP:.3f} x 2^-24")
    assert e < 2 * cases.ULP


@pytest.mark.parametrize("S,h,w", cases.SIZES, ids=lambda n: str(n))
def test_second_pads_carry_no_weight(S, h, w):
    """A coordinate is at most S, so a tap at S + 1 has the weight 1 - (1 - 0): exactly 0.  Those pads need no coverage."""
    _tp, rows, cols, weights = cases.taps(S, h, w)
    second = (rows == S + 1) | (cols == S + 1)
    assert rows.min() >= 0 and cols.min() >= 0 and rows.max() <= S + 1 and cols.max() <= S + 1
    assert (weights[second] == 0.0).all()


def test_the_odd_case_reaches_every_padded_class_and_the_zero_corners():
    S, h, w, _C = S7
    tp, rows, cols, weights = cases.taps(S, h, w)
    nk, _nr, _nc = pano.pad_source(S)
    heavy = weights >= HEAVY
    face = np.broadcast_to(tp[None], rows.shape)
    counts = {}
    for k in range(6):
        for name, sel in (("row pad", (rows == S) & (cols < S)), ("column pad", (rows < S) & (cols == S)),
                          ("both", (rows == S) & (cols == S))):
            counts[(cases.FACE_NAMES[k], name)] = int((heavy & (face == k) & sel).sum())
    zeros = int((heavy & (nk[face, rows, cols] < 0)).sum())
    print(counts, "zero corners:", zeros)
    assert len(counts) == 18 and min(counts.values()) >= 8, counts
    assert zeros >= 8


def _mutated(S: int, k: int, r: int, c: int):
    """The padded map with the entry (k, r, c) wrong: a texel's source column shifted by one mod S, a zero turned into texel (1, 0, 0)."""
    nk, nr, nc = (a.copy() for a in pano.pad_source(S))
    if nk[k, r, c] < 0:
        nk[k, r, c], nr[k, r, c], nc[k, r, c] = 1, 0, 0
    else:
        nc[k, r, c] = (nc[k, r, c] + 1) % S
    return nk, nr, nc


def test_check_rejects_every_single_wrong_entry_of_the_padded_map():
    S, h, w, C = S7
    faces = cases.noise_faces(S, C, seed=70)
    entries = [(k, r, c) for k in range(6) for r in range(S + 1) for c in range(S + 1) if r == S or c == S]
    assert len(entries) == 90
    missed = []
    for k, r, c in entries:
        with mock.patch.object(pano, "pad_source", lambda _S, m=_mutated(S, k, r, c): m):
            wrong = pano.c2e_host(faces, h, w).astype(np.float32)
        try:
            with contextlib.redirect_stdout(io.StringIO()):       # ninety report lines say nothing that the assertion below does not
                cases.check(wrong, faces, h, w)
        except AssertionError:
            continue
        missed.append((k, r, c))
    print(f"bound {cases.bound(faces, h, w, pano.c2e_host(faces, h, w)).max():.3e}: {len(missed)} of {len(entries)} wrong entries missed")
    assert not missed, f"{len(missed)} of 90 wrong entries pass the bound: {missed}"


@pytest.mark.parametrize("S,h,w,C", cases.TAP_CASES, ids=lambda n: str(n))
def test_check_passes_the_reference_itself(S, h, w, C):
    faces = cases.noise_faces(S, C, seed=S)
    assert cases.check(pano.c2e_host(faces, h, w).astype(np.float32), faces, h, w) <= 1.0


def test_check_names_the_worst_pixel_and_its_taps():
    S, h, w, C = S7
    faces = cases.noise_faces(S, C, seed=70)
    wrong = pano.c2e_host(faces, h, w).astype(np.float32)
    wrong[0, 5, 1] += np.float32(1e-3)
    with pytest.raises(AssertionError, match=r"pixel \(0, 5\) channel 1, face type 4 \(up\)(.|\n)*padded \(\d+, \d+\) weight"):
        cases.check(wrong, faces, h, w)


def test_truth_coordinates_on_the_smallest_call():
    """S 2, 2 x 8: every pixel is up or down (down where both masks hold) and tan is taken of an exact 0: both sets of coordinates
    are the face centre, which is why the GPU test can ask for equal bits there."""
    S, h, w = cases.SMALLEST_CASE
    tp, u, v = cases.grid(h, w)
    assert np.array_equal(tp, np.repeat([[4], [5]], w, axis=1))
    for x, y in (pano._face_coordinates(tp, u, v, S), cases.truth_coordinates(tp, u, v, S)):
        assert (x == 1.0).all() and (y == 1.0).all()
