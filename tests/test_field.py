"""autovfx_amd.field without a GPU: the numpy restatement of the contract against the float64 truth and against recorded runs of the
reference's own SuGaR.get_field_values, what the kernels take, the install() hook, and the C ABI's refusals."""
import ctypes
import sys
import types
from unittest import mock

import numpy as np
import pytest
import torch

import field_cases as FC
from autovfx_amd import field
from helpers import fake_gpu as fake

F = np.float32


def random_case(N, K, P, seed, bad_slots=True):
    g = np.random.default_rng(seed)
    centers = g.uniform(0, 1, (P, 3)).astype(F)
    scaling = np.exp(g.normal(np.log(0.2), 0.4, (P, 3)))
    A = g.normal(size=(P, 3, 3))
    R = np.linalg.qr(A)[0]
    M = (R / scaling[:, None, :]).astype(F)
    strengths = g.uniform(0.05, 1, (P, 1)).astype(F)
    x = (centers[g.integers(0, P, N)] + g.normal(0, 0.15, (N, 3))).astype(F)
    near = np.argsort(((x[:, None, :] - centers[None]) ** 2).sum(-1), axis=1, kind="stable")       # nearest first, as SuGaR's lists
    idx = near[:, np.arange(K) % P].astype(np.int64)                                                   # (K > P: the list repeats)
    if bad_slots:
        idx[g.random((N, K)) < 0.1] = -1          # pytorch3d's missing slot
        idx[g.random((N, K)) < 0.05] = P          # one past the end
    ups = dict(g_density=g.normal(size=N).astype(F), g_opacities=g.normal(size=(N, K)).astype(F), g_beta=g.normal(size=N).astype(F))
    return dict(x=x, idx=idx, centers=centers, M=M, strengths=strengths, min_scaling=scaling.min(1).astype(F), density_factor=0.8, ups=ups)


@pytest.mark.parametrize("N,K,P", [(1, 1, 1), (65, 3, 2), (257, 16, 300), (130, 17, 40)])
def test_host_restatement_against_float64(N, K, P):
    c = random_case(N, K, P, seed=N + K)
    args = (c["x"], c["idx"], c["centers"], c["M"], c["strengths"], c["min_scaling"], c["density_factor"])
    want = FC.truth(*args, **c["ups"])
    d, o, b = field.field_values_host(*args)
    assert d.dtype == o.dtype == b.dtype == F and d.shape == (N,) and o.shape == (N, K) and b.shape == (N,)
    FC.check_forward(dict(density=d, opacities=o, beta=b), want, label=f"host {N}x{K}/{P}")
    bad = (c["idx"] < 0) | (c["idx"] >= P)
    assert np.all(o[bad] == 0)
    FC.check_grads(field.field_grads_host(*args, **c["ups"]), want, label=f"host {N}x{K}/{P}")


def test_host_restatement_far_sample_and_centre():
    """q > 1e8: the output is sigma exp(-5e7) = 0 and every gradient exactly 0; q == 0: the sample at the centre gives sigma itself."""
    centers = np.array([[0, 0, 0], [1, 1, 1]], F)
    M = np.stack([np.eye(3, dtype=F) * F(10), np.eye(3, dtype=F) * F(10)])
    x = np.array([[2000, 0, 0], [1, 1, 1]], F)
    idx = np.array([[0], [1]], np.int64)
    d, o, _ = field.field_values_host(x, idx, centers, M, np.array([0.5, 0.25], F))
    assert d[0] == 0 and d[1] == F(0.25)
    g = field.field_grads_host(x, idx, centers, M, np.array([0.5, 0.25], F), g_density=np.ones(2, F))
    assert np.all(g["x"] == 0) and np.all(g["centers"] == 0) and np.all(g["inv_scaled_rotation"] == 0)
    assert g["strengths"][0] == 0 and g["strengths"][1] == 1


@pytest.mark.parametrize("name", FC.FIXTURES)
def test_host_restatement_against_the_reference_fixtures(name):
    fx = FC.fixture(name)
    avg = fx["beta_mode"] == "average"
    want = FC.fixture_truth(name, avg)
    args = (fx["x"], fx["idx"], fx["points"], fx["inv_scaled_rotation"], fx["strengths"], fx["min_scaling"] if avg else None, fx["density_factor"])
    d, o, b = field.field_values_host(*args)
    print("reference's own fp32 errors:", FC.reference_forward_errors(name))
    FC.check_forward(dict(density=d, opacities=o, beta=b), want, FC.forward_bars(name), label=name)
    got = field.field_grads_host(*args, g_density=fx["g_density"], g_opacities=fx["g_opacities"], g_beta=fx["g_beta"] if avg else None)
    if not avg:
        got.pop("min_scaling")
    FC.check_grads(got, want, label=name)
    # and the recorded fp32 results themselves are near: twice the bar covers the restatement's and the reference's error together
    bars = FC.forward_bars(name)
    assert np.abs(d - fx["out.density"]).max() <= 2 * bars["density"]
    assert np.abs(o - fx["out.closest_gaussian_opacities"]).max() <= 2 * bars["opacities"]


def test_fixtures_cover_what_they_should():
    modes = {FC.fixture(n)["beta_mode"] for n in FC.FIXTURES}
    assert {"average", "weighted_average"} <= modes
    assert any(FC.fixture(n)["density_factor"] != 1.0 for n in FC.FIXTURES)
    assert any(FC.fixture(n)["idx"].shape[1] != 16 for n in FC.FIXTURES)
    print("gradient factors c:", FC.gradient_factors(), "forward bars / scale:", FC.forward_bars_relative())


def test_why_not_reasons():
    x, idx = torch.zeros(5, 3), torch.full((5, 4), -1, dtype=torch.int64)     # pytorch3d-style -1 slots are no reason
    c, M, s = torch.zeros(7, 3), torch.zeros(7, 3, 3), torch.zeros(7, 1)
    assert "GPU" in field._why_not(x, idx, c, M, s)
    assert not field.field_takes(x, idx, c, M, s)
    with pytest.raises(ValueError, match="GPU"):
        field.field_values(x, idx, c, M, s)
    with pytest.raises(ValueError, match="host number"):
        field.field_values(x, idx, c, M, s, density_factor=torch.tensor(1.0))
    assert "torch.Tensor" in field._why_not(x.numpy(), idx, c, M, s)
    good = dict(x=fake(5, 3), idx=fake(5, 4, dtype=torch.int64), centers=fake(7, 3), inv_scaled_rotation=fake(7, 3, 3), strengths=fake(7, 1))
    why = lambda **kw: field._why_not(**{**good, **kw})
    with mock.patch("torch.cuda.is_initialized", lambda: False):
        assert why() is None
        assert why(strengths=fake(7)) is None
        assert "float32" in why(x=fake(5, 3, dtype=torch.float64))
        assert "int64" in why(idx=fake(5, 4, dtype=torch.int32))
        assert "[N, 3]" in why(x=fake(5, 2))
        for name, reason in (("x", "[N, 3]"), ("idx", "[N, K]"), ("centers", "[P, 3]"), ("inv_scaled_rotation", "[P, 3, 3]"), ("strengths", "strengths")):
            assert reason in why(**{name: fake((), dtype=good[name].dtype)}), name          # a 0-dim tensor is a reason, not an IndexError
        assert "min_scaling" in why(min_scaling=fake(()))
        assert "[N, K]" in why(idx=fake(6, 4, dtype=torch.int64))
        assert "K must be" in why(idx=fake(5, 65, dtype=torch.int64))
        assert why(idx=fake(5, 64, dtype=torch.int64)) is None
        assert "[P, 3, 3]" in why(inv_scaled_rotation=fake(6, 3, 3))
        assert "strengths" in why(strengths=fake(7, 2))
        assert "min_scaling" in why(min_scaling=fake(6))
        assert "beta needs" in why(want_beta=True)
        assert why(want_beta=True, min_scaling=fake(7)) is None


def _stub_sugar_module(name="stubpkg.sugar_model"):
    mod = types.ModuleType(name)

    class SuGaR:
        def compute_density(self, x, closest_gaussians_idx=None, density_factor=1., return_closest_gaussian_opacities=False):
            return "reference compute_density"

        def get_field_values(self, x, **kwargs):
            return "reference get_field_values"

        def get_beta(self, x, **kwargs):
            return None

        def get_covariance(self, **kwargs):
            return None

        def render_image_gaussian_rasterizer(self, *a, **k):
            return "reference render"

    SuGaR.__module__ = name
    mod.SuGaR = SuGaR
    return mod


def test_hook_replaces_both_methods_and_restores_them():
    import autovfx_amd
    from autovfx_amd import hook
    mod = _stub_sugar_module()
    importer = types.ModuleType("stubpkg.trainer")
    importer.SuGaR = mod.SuGaR
    originals = {k: vars(mod.SuGaR)[k] for k in ("compute_density", "get_field_values", "render_image_gaussian_rasterizer", "get_beta")}
    sys.modules[mod.__name__], sys.modules[importer.__name__] = mod, importer
    try:
        autovfx_amd.install(path=False)
        for k in ("compute_density", "get_field_values"):
            assert vars(mod.SuGaR)[k] is not originals[k] and hook._is_ours(vars(mod.SuGaR)[k])
            assert vars(mod.SuGaR)["reference_" + k] is originals[k]
        assert vars(mod.SuGaR)["get_beta"] is originals["get_beta"]
        assert hook._is_ours(vars(mod.SuGaR)["render_image_gaussian_rasterizer"])      # the row of item 4 on the same class still applies
        assert importer.SuGaR is mod.SuGaR and mod.__name__ in hook.patched_modules
        first = vars(mod.SuGaR)["compute_density"]
        autovfx_amd.install(path=False)                                                   # a second install() does not wrap again
        assert vars(mod.SuGaR)["compute_density"] is first and vars(mod.SuGaR)["reference_compute_density"] is originals["compute_density"]
        # CPU tensors reach the reference untouched
        assert mod.SuGaR().compute_density(torch.zeros(4, 3)) == "reference compute_density"
        assert mod.SuGaR().get_field_values(torch.zeros(4, 3), return_sdf=True) == "reference get_field_values"
        autovfx_amd.uninstall()
        for k, v in originals.items():
            assert vars(mod.SuGaR)[k] is v
            assert "reference_" + k not in vars(mod.SuGaR)
    finally:
        autovfx_amd.uninstall()
        sys.modules.pop(mod.__name__, None)
        sys.modules.pop(importer.__name__, None)


def test_hook_leaves_a_class_without_the_four_methods_alone():
    import autovfx_amd
    mod = _stub_sugar_module("otherpkg.sugar_model")
    del mod.SuGaR.get_covariance
    original = vars(mod.SuGaR)["compute_density"]
    sys.modules[mod.__name__] = mod
    try:
        autovfx_amd.install(path=False)
        assert vars(mod.SuGaR)["compute_density"] is original and not hasattr(mod.SuGaR, "reference_compute_density")
    finally:
        autovfx_amd.uninstall()
        sys.modules.pop(mod.__name__, None)


def test_c_abi_refusals_need_no_device():
    from autovfx_amd import _lib
    L = _lib.lib
    assert L.gsr_abi_version() == 20 == _lib.ABI_VERSION
    assert L.gsr_field_scratch_bytes(1000) == 64000 and L.gsr_field_scratch_bytes(0) == 64
    assert L.gsr_field_scratch_bytes(-1) == 0 and L.gsr_field_scratch_bytes(1 << 30) == 0
    buf = (ctypes.c_char * 4096)()
    a = (ctypes.addressof(buf) + 255) & ~255                      # 256-byte aligned host memory: refusals never touch it
    ins = lambda n=4, K=2, P=3, x=a, idx=a, c=a, M=a, s=a, m=None: (n, K, P, x, idx, c, M, s, m, 1.0)
    fwd = lambda *i, density=a, opac=None, beta=None, scratch=a, nbytes=4096: L.gsr_field_forward(*i, density, opac, beta, scratch, nbytes, None)
    bwd = lambda *i, gd=a, go=None, gb=None, dx=a, accum=a, scratch=a, nbytes=4096: L.gsr_field_backward(*i, gd, go, gb, dx, accum, scratch, nbytes, None)
    for call in (fwd, bwd):
        assert call(*ins(n=0), scratch=None) == 0                                                    # nothing to do, nothing looked at
        for K in (0, 65, -1):
            assert call(*ins(K=K)) == -1 and "K =" in _lib.last_error()
        assert call(*ins(n=-1)) == -1 and "negative" in _lib.last_error()
        assert call(*ins(P=-1)) == -1 and "negative" in _lib.last_error()
        assert call(*ins(n=1 << 30)) == -1 and "2^30" in _lib.last_error()
        assert call(*ins(P=1 << 30)) == -1 and "2^30" in _lib.last_error()
        for name in ("x", "idx", "c", "M", "s"):
            assert call(*ins(**{name: None})) == -1 and "null" in _lib.last_error(), name
        assert call(*ins(), scratch=None) == -1 and "null" in _lib.last_error()
        assert call(*ins(x=a + 2)) == -1 and "misaligned" in _lib.last_error()
        assert call(*ins(idx=a + 4)) == -1 and "misaligned" in _lib.last_error()
        assert call(*ins(), scratch=a + 64) == -1 and "misaligned" in _lib.last_error()
        assert call(*ins(), nbytes=3 * 64 - 1) == -1 and "scratch too small" in _lib.last_error()
    assert fwd(*ins(), beta=a) == -1 and "min_scaling" in _lib.last_error()
    assert bwd(*ins(), gb=a) == -1 and "min_scaling" in _lib.last_error()
    assert fwd(*ins(), density=None) == -1 and "null" in _lib.last_error()
    assert fwd(*ins(), opac=a + 1) == -1 and "misaligned" in _lib.last_error()
    assert bwd(*ins(), accum=None) == -1 and "null" in _lib.last_error()
    assert bwd(*ins(), accum=a + 16) == -1 and "misaligned" in _lib.last_error()
