"""simple_knn's distCUDA2 without a GPU: the numpy restatement of the contract (autovfx_amd/knn.py: mean_dist3_host) against a float64
truth and against hand-built cases, the C ABI's refusals, the drop-in's import path, and the reference's surface where it is mounted."""
from __future__ import annotations

import contextlib
import importlib
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from autovfx_amd.knn import FLT_MAX, knn_points_host, mean_dist3_host
from shims import reference_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_KNN = os.path.join(reference_env.REF, "sugar", "gaussian_splatting", "submodules", "simple-knn")
F = np.float32


def _truth(pts: np.ndarray) -> np.ndarray:
    """The three nearest by float64 distance of the float32 points, their mean in float64."""
    p = pts.astype(np.float64)
    d = ((p[None, :, :] - p[:, None, :]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    return np.sort(d, axis=1)[:, :3].mean(1)


@pytest.mark.parametrize("kind", ["cube", "clusters", "plane"])
def test_restatement_against_float64_truth(kind):
    g = np.random.default_rng(7)
    if kind == "cube":
        pts = g.uniform(-3, 3, (700, 3))
    elif kind == "clusters":
        pts = np.concatenate([g.normal(c, 0.05, (100, 3)) for c in g.uniform(-10, 10, (6, 3))])
    else:
        pts = np.c_[g.uniform(-1, 1, (600, 2)), np.full(600, 0.25)]
    pts = pts.astype(F)
    got, want = mean_dist3_host(pts).astype(np.float64), _truth(pts)
    assert np.all(np.abs(got - want) <= 16 * 2.0 ** -24 * want)


def test_restatement_is_chunk_independent():
    pts = np.random.default_rng(1).normal(0, 1, (333, 3)).astype(F)
    ref = mean_dist3_host(pts)
    for chunk in (1, 333, 1000, 5 * 333 + 7):
        assert np.array_equal(mean_dist3_host(pts, chunk_elems=chunk), ref)


def test_tiny_inputs():
    inf = np.float32(np.inf)
    assert mean_dist3_host(np.zeros((0, 3), F)).shape == (0,)
    assert np.array_equal(mean_dist3_host([[1, 2, 3]]), [inf])
    assert np.array_equal(mean_dist3_host([[0, 0, 0], [1, 0, 0]]), [inf, inf])
    three = mean_dist3_host([[0, 0, 0], [1, 0, 0], [0, 2, 0]])
    assert np.all(three == np.float32(1.1342745e38)) and np.all(np.isfinite(three))
    assert three[0] == (F(1) + F(4) + F(FLT_MAX)) / F(3)
    four = mean_dist3_host([[0, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 3]])
    assert np.array_equal(four, np.array([(1 + 4 + 9) / 3, (1 + 5 + 10) / 3, (4 + 5 + 13) / 3, (9 + 10 + 13) / 3], F))
    five = mean_dist3_host([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [4, 0, 0]])
    assert np.array_equal(five, np.array([14 / 3, 2, 2, 2, 14 / 3], F))


def test_duplicates_and_identical_points():
    pts = np.array([[0, 0, 0], [0, 0, 0], [1, 1, 1], [5, 5, 5], [1, 1, 1]], F)
    got = mean_dist3_host(pts)
    assert got[0] == got[1] == F(F(F(0) + F(3)) + F(3)) / F(3)
    assert got[2] == got[4] == F(F(F(0) + F(3)) + F(3)) / F(3)
    assert np.array_equal(mean_dist3_host(np.full((17, 3), 2.5, F)), np.zeros(17, F))


def test_non_finite_points_are_nobodys_neighbours():
    pts = np.array([[0, 0, 0], [np.nan, 0, 0], [1, 0, 0], [0, np.inf, 0], [0, 2, 0], [0, 0, -np.inf], [0, 0, 3]], F)
    got = mean_dist3_host(pts)
    assert np.isposinf(got[[1, 3, 5]]).all()
    assert np.array_equal(got[[0, 2, 4, 6]], mean_dist3_host(pts[[0, 2, 4, 6]]))


def test_overflowing_distances_do_not_count():
    # 2e19 apart: the square overflows to inf in fp32, so the far pair are not neighbours of each other
    pts = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [2e19, 0, 0], [2e19, 1, 0]], F)
    got = mean_dist3_host(pts)
    assert np.isposinf(got[3]) and np.isposinf(got[4])   # (1 + FLT_MAX + FLT_MAX) / 3
    assert np.array_equal(got[:3], mean_dist3_host(pts[:3]))


@pytest.mark.parametrize("kind", ["uniform", "repeated", "pairs", "lattice"])
def test_three_slot_mean_is_the_self_query_row_without_its_first_entry(kind):
    """The two restatements answer for each other: for finite points and P >= 4 the self query's row is [0, d1, d2, d3] (the point
    itself, or a duplicate of it, at 0), and d1 <= d2 <= d3 are the three slots of the three-slot search.  Bit for bit."""
    g = np.random.default_rng(21)
    if kind == "uniform":
        pts = g.uniform(-1, 1, (4000, 3))
    elif kind == "repeated":     # every point four times: ties at distance 0 are the rule
        pts = np.repeat(g.uniform(-1, 1, (1000, 3)), 4, axis=0)[g.permutation(4000)]
    elif kind == "pairs":        # every point twice: one tie at 0 and a sum that is not 0
        pts = np.repeat(g.uniform(-1, 1, (2000, 3)), 2, axis=0)[g.permutation(4000)]
    else:                        # 13^3 lattice points: equal distances in every row
        pts = np.stack(np.meshgrid(*[np.arange(13)] * 3, indexing="ij"), -1).reshape(-1, 3) * 0.25
    pts = pts.astype(F)
    d = knn_points_host(pts, pts, 4)[0]
    assert np.all(d[:, 0] == 0)
    want = ((d[:, 1] + d[:, 2]) + d[:, 3]) / F(3.0)
    got = mean_dist3_host(pts)
    assert got.dtype == want.dtype == F and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_cabi_refusals_need_no_device():
    from autovfx_amd import _lib
    L = _lib.lib
    assert L.gsr_knn3_mean_dist(0, None, None, None, 0, None) == 0                      # nothing to do
    assert L.gsr_knn3_scratch_bytes(0) == 0
    assert L.gsr_knn3_mean_dist(5, None, None, None, 1 << 20, None) == -1 and "null" in _lib.last_error()
    assert L.gsr_knn3_mean_dist(5, 4096, None, 8192, 1 << 20, None) == -1 and "null" in _lib.last_error()
    assert L.gsr_knn3_mean_dist(1 << 30, 4096, 4096, 8192, 1 << 40, None) == -1 and "2^30" in _lib.last_error()
    assert L.gsr_knn3_scratch_bytes(1 << 30) == 0
    need = L.gsr_knn3_scratch_bytes(1000)
    assert 0 < need <= 48 * 1000 + 8192
    assert L.gsr_knn3_mean_dist(1000, 4096, 8192, 1 << 20, need - 1, None) == -1 and "scratch" in _lib.last_error()
    assert L.gsr_knn3_mean_dist(1000, 4096, 8192, (1 << 20) + 4, need, None) == -1 and "aligned" in _lib.last_error()
    big = L.gsr_knn3_scratch_bytes((1 << 30) - 1)
    assert 0 < big <= 48 * (1 << 30)


def test_scratch_stays_under_48_bytes_per_point():
    from autovfx_amd import _lib
    for n in (1, 63, 64, 65, 4096, 1_000_000, 3_000_000):
        assert _lib.lib.gsr_knn3_scratch_bytes(n) <= 48 * n + 16384, n


def test_drop_in_import_path_resolves_to_this_repository(tmp_path):
    code = textwrap.dedent(f"""
        import sys
        sys.path.insert(0, {ROOT!r})
        import autovfx_amd
        autovfx_amd.install()
        import simple_knn._C
        print(simple_knn._C.__file__)
        print(callable(simple_knn._C.distCUDA2))
    """)
    r = subprocess.run([sys.executable, "-c", code], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    path, ok = r.stdout.split()
    assert os.path.realpath(path) == os.path.realpath(os.path.join(ROOT, "simple_knn", "_C.py"))
    assert ok == "True"


@contextlib.contextmanager
def drop_in_modules():
    """Other tests register stubs under ``simple_knn`` / ``simple_knn._C`` (and set ``distCUDA2 = None`` on whatever is there):
    take them out, import the drop-in, put everything back afterwards."""
    saved = {k: sys.modules.pop(k) for k in ("simple_knn", "simple_knn._C") if k in sys.modules}
    try:
        pkg = importlib.import_module("simple_knn")
        mod = importlib.import_module("simple_knn._C")
        assert os.path.realpath(mod.__file__) == os.path.realpath(os.path.join(ROOT, "simple_knn", "_C.py"))
        yield pkg, mod
    finally:
        for k in ("simple_knn", "simple_knn._C"):
            sys.modules.pop(k, None)
        sys.modules.update(saved)


def test_drop_in_exposes_the_implementation():
    from autovfx_amd import knn
    with drop_in_modules() as (_pkg, mod):
        assert mod.mean_dist3 is knn.mean_dist3
        with pytest.raises(ValueError):      # a CPU tensor is refused before anything is launched
            import torch
            mod.distCUDA2(torch.zeros(4, 3))


@pytest.mark.skipif(not os.path.isfile(os.path.join(REF_KNN, "ext.cpp")), reason="the reference tree is not mounted")
def test_reference_binds_exactly_distCUDA2():
    src = open(os.path.join(REF_KNN, "ext.cpp")).read()
    assert re.findall(r'm\.def\(\s*"(\w+)"', src) == ["distCUDA2"]
    with drop_in_modules() as (_pkg, mod):
        public = [k for k in vars(mod) if not k.startswith("_") and callable(getattr(mod, k)) and getattr(mod, k).__module__ == mod.__name__]
        assert public == ["distCUDA2"]


@pytest.mark.skipif(not os.path.isdir(REF_KNN), reason="the reference tree is not mounted")
def test_reference_gaussian_model_imports_the_drop_in():
    if not reference_env.available():
        pytest.skip("the reference tree is not mounted")
    with reference_env.reference_tree():
        for k in ("simple_knn", "simple_knn._C"):
            sys.modules.pop(k, None)
        real = importlib.import_module("simple_knn._C")
        assert os.path.realpath(real.__file__) == os.path.realpath(os.path.join(ROOT, "simple_knn", "_C.py"))
        gm = importlib.import_module("scene.gaussian_model")
        assert gm.distCUDA2 is real.distCUDA2
        assert hasattr(gm.GaussianModel, "create_from_pcd")
