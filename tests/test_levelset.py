"""autovfx_amd.levelset without a GPU: the selection and interpolation against the reference's expressions bit for bit, the numpy
restatement of the contract against the float64 truth and against recorded runs of the reference's own
SuGaR.compute_level_surface_points_from_camera_fast, what the kernel takes, the C ABI's refusals, and the install() hook."""
import ctypes
import sys
import types
from unittest import mock

import numpy as np
import pytest
import torch

import levelset_cases as LC
from autovfx_amd import levelset
from helpers import fake_gpu as fake

F = np.float32
LEVELS = {1: [0.3], 3: [0.1, 0.3, 0.5], 8: [0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.7, 0.9]}
# (n, K, S, L, P): the shapes test_levelset_gpu.py runs the kernel at
SHAPES = ([(n, 16, 21, 3, 300) for n in (1, 63, 64, 65, 257, 4099)] + [(257, K, 21, 3, 300) for K in (1, 3, 17)]
          + [(257, 16, S, 3, 300) for S in (2, 3, 32)] + [(257, 16, 21, L, 300) for L in (1, 8)] + [(65, 3, 21, 3, P) for P in (1, 2)])


def shape_case(n, K, S, L, P):
    """Every slot live; rays with slots outside [0, P), live ones among them, are the edge rays' test."""
    return LC.random_case(n, K, P, seed=2000 + n + 7 * K + 11 * S + 13 * L + P, bad_slots=False)


def host(c, levels, S=21, range_size=3.0):
    return levelset.level_surface_host(c["origins"], c["dirs"], c["stds"], c["idx"], c["centers"], c["M"], c["strengths"], levels, S, range_size,
                                       c["density_factor"])


def test_crossing_host_is_the_reference_selection_bit_for_bit():
    nan = float("nan")
    d = np.array([[0.6, 0.7, 0.8, 0.9],        # d_0 above the level
                  [0.1, 0.2, 0.25, 0.29],      # nothing above the level
                  [0.1, 0.3, 0.3, 0.4],        # samples equal to the level: neither under nor above, the crossing is at s = 3
                  [0.3, 0.5, 0.6, 0.7],        # d_0 equal to the level: not under
                  [0.1, nan, 0.5, 0.6],        # a NaN is skipped as not above
                  [nan, 0.5, 0.6, 0.7],        # a NaN first: not under
                  [0.1, 0.4, 0.2, 0.9],        # a = 1
                  [0.0, 0.1, 0.2, 0.8],        # a = S - 1
                  [0.2, 0.1, 0.35, 0.2]], F)   # falls, then crosses
    tau = (np.linspace(-3, 3, 4, dtype=F)[None, :] * np.linspace(0.05, 0.4, len(d), dtype=F)[:, None]).astype(F)
    for level in (0.3, 0.1, 0.5):
        hit, a, t = levelset.crossing_host(d, tau, level)
        # :1890-1907 restated with torch
        densities, points_range = torch.tensor(d), torch.tensor(tau)[..., None]
        under_level = (densities - level < 0)
        above_level = (densities - level > 0)
        _, first_point_above_level = above_level.max(dim=-1, keepdim=True)
        empty_pixels = ~under_level[..., 0] + (first_point_above_level[..., 0] == 0)
        valid_densities = densities[~empty_pixels]
        valid_range = points_range[~empty_pixels][..., 0]
        valid_first = first_point_above_level[~empty_pixels]
        first_value = valid_densities.gather(dim=-1, index=valid_first).view(-1)
        value_before = valid_densities.gather(dim=-1, index=valid_first - 1).view(-1)
        first_t = valid_range.gather(dim=-1, index=valid_first).view(-1)
        t_before = valid_range.gather(dim=-1, index=valid_first - 1).view(-1)
        intersection_t = (level - value_before) / (first_value - value_before) * (first_t - t_before) + t_before
        assert np.array_equal(hit, ~empty_pixels.numpy())
        assert np.array_equal(a[hit], valid_first.numpy()[:, 0])
        assert t.dtype == F and np.array_equal(t[hit].view(np.uint32), intersection_t.numpy().view(np.uint32))
        assert np.all(t[~hit] == 0)
        if level == 0.3:
            assert hit.tolist() == [False, False, True, False, True, False, True, True, True] and a[hit].tolist() == [3, 2, 1, 3, 2]


@pytest.mark.parametrize("n,K,S,L,P", SHAPES)
def test_host_restatement_against_float64(n, K, S, L, P):
    """... and every random case keeps its rays near a level under the cap (LC.check asserts it)."""
    c = shape_case(n, K, S, L, P)
    got, want = host(c, LEVELS[L], S), LC.truth(c, LEVELS[L], S)
    assert got["hit"].shape == (L, n) and got["points"].shape == (L, n, 3) and got["normals"].dtype == F and got["densities"].shape == (n, S)
    LC.check(got, want, label=f"host {n}x{K} S{S} L{L} P{P}")
    if (n, K, S, L) == (4099, 16, 21, 3):
        assert want["hit"].any(1).all() and not want["hit"].all(1).any() and (want["densities"] > 0.999999).sum() > 1      # some renormalised


def test_host_restatement_edge_rays():
    c = shape_case(65, 16, 21, 3, 300)
    c["idx"][3] = -1                      # no neighbour at all
    c["idx"][4] = 300
    c["stds"][5] = 0                      # every sample at the origin: no crossing
    got = host(c, LEVELS[3])
    assert not got["hit"][:, [3, 4, 5]].any() and np.all(got["densities"][[3, 4]] == 0)
    assert np.all(got["densities"][5] == got["densities"][5, 0])
    LC.check(got, LC.truth(c, LEVELS[3]), label="host edge rays")
    c["idx"][7:30:2, 5] = -1              # live rays with missing slots: the normal pass skips them as the density pass does
    c["idx"][8:30:2, 9] = 300
    c["idx"][30:40, 1::2] = -1
    want = LC.truth(c, LEVELS[3])
    assert want["hit"][:, 7:40].any(1).all()
    LC.check(host(c, LEVELS[3]), want, label="host missing slots")
    c["density_factor"] = 40.0            # most densities renormalised at 1
    got, want = host(c, [0.5, 0.999]), LC.truth(c, [0.5, 0.999])
    assert (got["densities"] == 1).mean() > 0.3 and got["densities"].max() == 1
    LC.check(got, want, label="host renormalised")


@pytest.mark.parametrize("name", LC.FIXTURES)
def test_host_restatement_against_the_reference_fixtures(name):
    fx = LC.fixture(name)
    c, want, ref = LC.fixture_case(name), LC.fixture_truth(name), LC.reference_dense(name)
    bar_d = LC.density_bar(name)
    print(f"reference's own fp32 density error {LC.reference_density_error(name):.3e}")
    LC.check(ref, want, bar_d, label=name + " (reference)")          # the reference's own results: under the cap, inside the bars
    got = host(c, fx["levels"], fx["n_points_in_range"], fx["range_size"])
    LC.check(got, want, bar_d, label=name)
    far = ~LC.near_level(want, 2 * bar_d)                            # two fp32 results: both errors
    assert np.array_equal(got["hit"][far], ref["hit"][far]) and np.array_equal(got["a"][far & ref["hit"]], ref["a"][far & ref["hit"]])
    assert np.abs(got["densities"] - ref["densities"]).max() <= 2 * bar_d


def test_fixtures_cover_what_they_should():
    fxs = [LC.fixture(n) for n in LC.FIXTURES]
    assert {3, 16} <= {fx["knn_idx"].shape[1] for fx in fxs}
    assert {1, 3} <= {len(fx["levels"]) for fx in fxs}
    assert any(fx["n_surface_points"] == -1 and fx["perm"].size == 0 for fx in fxs) and any(fx["perm"].size for fx in fxs)
    assert any(fx["density_factor"] != 1.0 for fx in fxs)
    assert all((fx["zbuf"][..., 0] < 0).any() for fx in fxs)
    assert all(fx["levels"] in ([0.1, 0.3, 0.5], [0.3]) for fx in fxs)
    print("factors c:", LC.factors(), "density bar / largest density:", LC.density_bar_relative(),
          "density bars:", {n: LC.density_bar(n) for n in LC.FIXTURES})


def test_why_not_reasons():
    o, v, sd, idx = torch.zeros(5, 3), torch.zeros(5, 3), torch.zeros(5), torch.full((5, 4), -1, dtype=torch.int64)
    c, M, s = torch.zeros(7, 3), torch.zeros(7, 3, 3), torch.zeros(7, 1)
    assert "GPU" in levelset._why_not(o, v, sd, idx, c, M, s, [0.3])
    assert not levelset.level_surface_takes(o, v, sd, idx, c, M, s, [0.3])
    with pytest.raises(ValueError, match="GPU"):
        levelset.level_surface(o, v, sd, idx, c, M, s, [0.3])
    with pytest.raises(ValueError, match="host number"):
        levelset.level_surface(o, v, sd, idx, c, M, s, [0.3], density_factor=torch.tensor(1.0))
    with pytest.raises(ValueError, match="host number"):
        levelset.level_surface(o, v, sd, idx, c, M, s, [0.3], range_size=torch.tensor(3.0))
    assert "torch.Tensor" in levelset._why_not(o.numpy(), v, sd, idx, c, M, s, [0.3])
    good = dict(origins=fake(5, 3), dirs=fake(5, 3), stds=fake(5), idx=fake(5, 4, dtype=torch.int64), centers=fake(7, 3),
                inv_scaled_rotation=fake(7, 3, 3), strengths=fake(7, 1), levels=[0.1, 0.3, 0.5])
    why = lambda **kw: levelset._why_not(**{**good, **kw})
    with mock.patch("torch.cuda.is_initialized", lambda: False):
        assert why() is None and why(strengths=fake(7)) is None and why(levels=(0.3,)) is None
        assert "float32" in why(dirs=fake(5, 3, dtype=torch.float64))
        assert "int64" in why(idx=fake(5, 4, dtype=torch.int32))
        for name, reason in (("origins", "[n, 3]"), ("dirs", "[n, 3]"), ("stds", "[n]"), ("idx", "[n, K]"), ("centers", "[P, 3]"),
                             ("inv_scaled_rotation", "[P, 3, 3]"), ("strengths", "strengths")):
            assert reason in why(**{name: fake((), dtype=good[name].dtype)}), name
        assert "[n, 3]" in why(dirs=fake(6, 3)) and "[n]" in why(stds=fake(5, 1))
        assert "K must be" in why(idx=fake(5, 65, dtype=torch.int64)) and why(idx=fake(5, 64, dtype=torch.int64)) is None
        assert "levels" in why(levels=[]) and "levels" in why(levels=[0.1] * 9) and why(levels=[0.1] * 8) is None
        assert "host numbers" in why(levels=torch.tensor([0.3])) and "host numbers" in why(levels=[torch.tensor(0.3)])
        assert "n_points_in_range" in why(n_points_in_range=33) and "n_points_in_range" in why(n_points_in_range=1)
        assert why(n_points_in_range=32) is None and why(n_points_in_range=2) is None
        needs_grad = fake(7, 3).requires_grad_()
        assert "gradient" in why(centers=needs_grad)
        with torch.no_grad():             # the extractor's state: the model's parameters still say they require one
            assert why(centers=needs_grad) is None


def test_c_abi_refusals_need_no_device():
    from autovfx_amd import _lib
    L = _lib.lib
    assert L.gsr_abi_version() == 20 == _lib.ABI_VERSION
    buf = (ctypes.c_char * 4096)()
    a = (ctypes.addressof(buf) + 255) & ~255                      # 256-byte aligned host memory: refusals never touch it
    levels = (ctypes.c_float * 8)(0.1, 0.3, 0.5)

    def call(n=4, K=2, P=3, S=21, Lv=3, o=a, v=a, sd=a, idx=a, c=a, M=a, s=a, rng=a, lv=ctypes.byref(levels), hit=a, t=a, pts=a, nrm=a, dens=None,
             scratch=a, nbytes=4096):
        return L.gsr_level_surface(n, K, P, S, Lv, o, v, sd, idx, c, M, s, 1.0, rng, lv, hit, t, pts, nrm, dens, scratch, nbytes, None)

    assert call(n=0, scratch=None, o=None, hit=None) == 0                                            # nothing to do, nothing looked at
    for K in (0, 65, -1):
        assert call(K=K) == -1 and "K =" in _lib.last_error()
    for S in (1, 33, 0):
        assert call(S=S) == -1 and "S =" in _lib.last_error()
    for Lv in (0, 9):
        assert call(Lv=Lv) == -1 and "L =" in _lib.last_error()
    assert call(n=-1) == -1 and "negative" in _lib.last_error()
    assert call(P=-1) == -1 and "negative" in _lib.last_error()
    assert call(n=1 << 30) == -1 and "2^30" in _lib.last_error()
    assert call(P=1 << 30) == -1 and "2^30" in _lib.last_error()
    for name in ("o", "v", "sd", "idx", "c", "M", "s", "rng", "lv", "hit", "t", "pts", "scratch"):
        assert call(**{name: None}) == -1 and "null" in _lib.last_error(), name
    for name in ("o", "v", "sd", "rng", "t", "pts", "nrm", "dens"):
        assert call(**{name: a + 2}) == -1 and "misaligned" in _lib.last_error(), name
    assert call(idx=a + 4) == -1 and "misaligned" in _lib.last_error()
    assert call(scratch=a + 64) == -1 and "misaligned" in _lib.last_error()
    assert call(nbytes=3 * 64 - 1) == -1 and "scratch too small" in _lib.last_error()


# ---- the hook ----
def _stub_sugar_module(name="stublevel.sugar_model"):
    mod = types.ModuleType(name)

    class SuGaR:
        def compute_level_surface_points_from_camera_fast(self, *args, **kwargs):
            return "reference march"

        def compute_density(self, x, **kwargs):
            return "reference compute_density"

        def get_covariance(self, **kwargs):
            return None

    SuGaR.__module__ = name
    mod.SuGaR = SuGaR
    return mod


ATTR = "compute_level_surface_points_from_camera_fast"


def test_hook_replaces_the_method_and_restores_it():
    import autovfx_amd
    from autovfx_amd import hook
    mod = _stub_sugar_module()
    original = vars(mod.SuGaR)[ATTR]
    sys.modules[mod.__name__] = mod
    try:
        autovfx_amd.install(path=False)
        assert vars(mod.SuGaR)[ATTR] is not original and hook._is_ours(vars(mod.SuGaR)[ATTR])
        assert vars(mod.SuGaR)["reference_" + ATTR] is original and mod.__name__ in hook.patched_modules
        first = vars(mod.SuGaR)[ATTR]
        autovfx_amd.install(path=False)                                                   # a second install() does not wrap again
        assert vars(mod.SuGaR)[ATTR] is first and vars(mod.SuGaR)["reference_" + ATTR] is original
        # a model that is not on a GPU reaches the reference, and nothing was drawn from the generator on the way
        m = mod.SuGaR()
        m.points = m.strengths = m.scaling = m.quaternions = torch.zeros(3, 3)
        state = torch.get_rng_state()
        assert m.compute_level_surface_points_from_camera_fast(n_surface_points=100) == "reference march"
        assert torch.equal(torch.get_rng_state(), state)
        autovfx_amd.uninstall()
        assert vars(mod.SuGaR)[ATTR] is original and "reference_" + ATTR not in vars(mod.SuGaR)
    finally:
        autovfx_amd.uninstall()
        sys.modules.pop(mod.__name__, None)


def test_hook_leaves_a_class_without_the_needed_methods_alone():
    import autovfx_amd
    mod = _stub_sugar_module("otherlevel.sugar_model")
    del mod.SuGaR.get_covariance
    original = vars(mod.SuGaR)[ATTR]
    sys.modules[mod.__name__] = mod
    try:
        autovfx_amd.install(path=False)
        assert vars(mod.SuGaR)[ATTR] is original and not hasattr(mod.SuGaR, "reference_" + ATTR)
    finally:
        autovfx_amd.uninstall()
        sys.modules.pop(mod.__name__, None)


def test_lenient_install_keeps_the_reference_when_the_library_cannot_load(capsys):
    import autovfx_amd
    from autovfx_amd import hook
    mod = _stub_sugar_module("lenientlevel.sugar_model")
    sys.modules[mod.__name__] = mod
    try:
        hook.install(path=False, strict=False)
        with mock.patch.object(hook, "_load", side_effect=ImportError("libgsr_hip.so not found")):
            assert mod.SuGaR().compute_level_surface_points_from_camera_fast() == "reference march"
        assert "level-surface ray march" in capsys.readouterr().err
        assert mod.SuGaR().compute_level_surface_points_from_camera_fast() == "reference march"      # not retried
    finally:
        autovfx_amd.uninstall()
        sys.modules.pop(mod.__name__, None)
