"""The bound Gaussians without a GPU: the numpy restatement of autovfx_amd/bound.py against the float64 truth and against recorded runs of the
reference's own ``SuGaR.points`` / ``scaling`` / ``quaternions``, the branches of ``matrix_to_quaternion``, the ``standardize`` flag and its
probe, what the kernels refuse, and the hook's rows for the three properties."""
from __future__ import annotations

import sys
import types
from unittest import mock

import numpy as np
import pytest
import torch

import bound_cases as BC
from autovfx_amd import bound
from helpers import OnGpu
from meshattrs_cases import atomic_sum_check

F32 = np.float32


def host(case, standardize=False, grads=BC.OUTPUTS):
    """Outputs and gradients of the numpy restatement, by name; ``grads``: the outputs whose upstream gradient arrives."""
    c = case
    out = dict(zip(BC.OUTPUTS, bound.bound_gaussians_host(c["verts"], c["faces"], c["bary"], c["complex"], c["log_scales"], c["thickness"], standardize)))
    up = {name: (c["grad_" + name] if name in grads else None) for name in BC.OUTPUTS}
    gv, gc, gl, added, rows = bound.bound_gaussians_backward_host(c["verts"], c["faces"], c["bary"], c["complex"], c["log_scales"], up["points"],
                                                                  up["scaling"], up["quaternions"], standardize)
    out.update(grad_verts=gv, grad_complex=gc, grad_log_scales=gl, added=added, rows=rows)
    return out


def tensors(got):
    return {k: v for k, v in got.items() if k in BC.OUTPUTS + BC.GRADS}


FIXTURES = BC.fixtures()
GENERATED = {"torus_g8": lambda: BC.torus_case(9, 7, 8, seed=3), "sized_65_g3": lambda: BC.sized_case(65, 3, seed=4),
             "spread_g4": lambda: BC.sized_case(130, 4, seed=5, V=5000, spread=True), "shared_g6": lambda: BC.shared_case(300, 6, seed=8),
             **{f"branch_{k}_g1": (lambda k=k: BC.branch_case(k, 64, 1, seed=2)) for k in range(4)}}


def test_the_fixtures_are_there_and_small():
    assert sorted(FIXTURES) == sorted([f"torus_g{G}" for G in (1, 3, 4, 6)] + [f"branch_{k}" for k in range(4)])
    for name, fx in FIXTURES.items():
        assert fx["faces"].shape[0] * fx["bary"].shape[0] == len(fx["complex"]) == len(fx["ref.quaternions"]), name


def test_the_bars_are_the_recorded_ones_and_come_from_the_reference():
    worst = BC.reference_ratios()
    for k, v in BC.RECORDED.items():
        assert worst[k] == pytest.approx(v, rel=2e-3), k
        assert BC.bars()[k] == 4.0 * worst[k]
    assert BC.bars()["matrices"] == 4.0 * BC.bars()["quaternions"] and worst["matrices"] <= BC.bars()["matrices"]


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_the_restatement_on_the_fixtures_within_the_bars(name):
    case = BC.fixture_case(FIXTURES[name])
    found = BC.check(case, tensors(host(case)), what=name)
    print(name, {k: round(v, 2) for k, v in found.items()})


@pytest.mark.parametrize("name", sorted(GENERATED))
@pytest.mark.parametrize("standardize", [False, True])
def test_the_restatement_against_the_truth_within_the_bars(name, standardize):
    case = GENERATED[name]()
    found = BC.check(case, tensors(host(case, standardize)), standardize, what=name)
    print(name, standardize, {k: round(v, 2) for k, v in found.items()})


@pytest.mark.parametrize("name", sorted(FIXTURES) + sorted(GENERATED))
def test_every_case_stays_under_the_near_tie_cap_with_the_reference_shaped_result(name):
    """At most 1 % of a case's rows are near ties in the truth, and there the fp32 chain in the reference's shape is still the same
    rotation."""
    case = BC.fixture_case(FIXTURES[name]) if name in FIXTURES else GENERATED[name]()
    want = BC.truth(case, grads=False)
    tie = BC.near_ties(want["q_abs"], name)
    if name in FIXTURES:
        ref = FIXTURES[name]["ref.quaternions"]
    else:
        with torch.no_grad():
            ref = BC.StubSuGaR(case).quaternions.numpy()
    BC.check(case, dict(quaternions=ref), what=name, want=want)
    if name in FIXTURES and tie.any():
        print(name, int(tie.sum()), "near-tie rows")


@pytest.mark.parametrize("k", range(4))
def test_each_branch_of_matrix_to_quaternion_is_taken_in_its_fixture(k):
    fx = FIXTURES[f"branch_{k}"]
    case = BC.fixture_case(fx)
    assert np.all(BC.truth(case, grads=False)["q_abs"].argmax(1) == k)
    with np.errstate(all="ignore"):
        r = bound._rotation(bound._frame(case["verts"], case["faces"]), case["complex"], case["bary"].shape[0], False)
    assert np.all(r["k"] == k) and np.all(r["qk"] >= 1.0)
    # the reference's own fp32 row is this candidate's: the restatement's row, sign included
    assert np.all(np.abs(fx["ref.quaternions"] - r["out"]) < 1e-5)
    if k:
        assert (r["out"][:, 0] < 0).any() and (r["out"][:, 0] > 0).any()      # (near-half-turns of either sense: both signs of the real part)


def test_an_exact_tie_goes_to_the_lowest_index():
    case = BC.tie_case()
    with np.errstate(all="ignore"):
        r = bound._rotation(bound._frame(case["verts"], case["faces"]), case["complex"], 1, False)
    assert r["q_abs"][0, 0] == r["q_abs"][0, 1] == np.sqrt(F32(2.0)) and r["k"][0] == 0
    half = np.sqrt(F32(0.5))
    assert np.allclose(r["out"][0], [half, half, 0, 0], atol=1e-7)


def test_the_standardize_flag_agrees_with_a_standardising_matrix_to_quaternion():
    case = BC.branch_case(1, 64, 3, seed=6)
    plain = host(case, False)
    flagged = host(case, True)
    negative = plain["quaternions"][:, 0] < 0
    assert negative.any() and (~negative).any()
    assert np.array_equal(flagged["quaternions"], np.where(negative[:, None], -plain["quaternions"], plain["quaternions"]))
    with mock.patch.object(BC, "matrix_to_quaternion", BC.matrix_to_quaternion_standardized):
        model = BC.StubSuGaR(case, requires_grad=True)
        q = model.quaternions
        (q * torch.from_numpy(case["grad_quaternions"])).sum().backward()
    assert (q[:, 0] >= 0).all()
    only = dict(case, grad_points=np.zeros_like(case["grad_points"]), grad_scaling=np.zeros_like(case["grad_scaling"]))
    BC.check(only, dict(quaternions=q.detach().numpy(), grad_verts=model._points.grad.numpy(), grad_complex=model._quaternions.grad.numpy()),
             standardize=True, what="the standardising stub")
    BC.check(only, tensors(host(only, True, grads=("quaternions",))), standardize=True, what="the flag")
    # the flip negates the row's gradient with it: the gradients of a flipped row for an upstream g are those of the plain row for -g
    mirrored = dict(only, grad_quaternions=np.where(negative[:, None], -only["grad_quaternions"], only["grad_quaternions"]))
    a, b = host(only, True, grads=("quaternions",)), host(mirrored, False, grads=("quaternions",))
    assert np.array_equal(a["grad_complex"], b["grad_complex"]) and np.array_equal(a["added"], b["added"])


def test_the_probe_tells_the_two_versions_apart():
    assert bound.standardizes(BC.matrix_to_quaternion) is False
    assert bound.standardizes(BC.matrix_to_quaternion_standardized) is True
    q = BC.matrix_to_quaternion(torch.tensor(bound._PROBE, dtype=torch.float32)[None])[0]
    assert q[0] < -0.05 and abs(float(q.norm()) - 1.0) < 1e-6


@pytest.mark.parametrize("grads", [("points",), ("scaling",), ("quaternions",), ("points", "quaternions"), ()])
def test_backward_host_with_absent_upstream_gradients(grads):
    case = BC.sized_case(65, 3, seed=7)
    zeroed = dict(case, **{"grad_" + name: np.zeros_like(case["grad_" + name]) for name in BC.OUTPUTS if name not in grads})
    got = host(case, grads=grads)
    BC.check(zeroed, {k: got[k] for k in BC.GRADS}, what="+".join(grads) or "none")
    atomic_sum_check(got["grad_verts"], got["added"], got["rows"], len(case["verts"]), "the face-order sum")
    if "quaternions" not in grads:
        assert not got["grad_complex"].any()
    if "scaling" not in grads:
        assert not got["grad_log_scales"].any()


def test_host_degenerate_rows():
    case = BC.sized_case(8, 3, seed=9)
    case["faces"][1] = [0, 0, 5]                       # a zero-area face
    case["complex"][3 * 2 + 1] = 0.0                   # complex = (0, 0)
    case["faces"][3] = [0, 1, len(case["verts"])]      # an index out of range
    case["faces"][4] = [2, -1, 3]
    got = host(case)
    for name in BC.OUTPUTS + BC.GRADS:
        assert np.isfinite(got[name]).all(), name
    for f in (3, 4):
        rows = slice(3 * f, 3 * f + 3)
        assert not got["points"][rows].any() and not got["quaternions"][rows].any() and not got["grad_complex"][rows].any()
    assert len(got["rows"]) == 3 * 6
    plain = BC.sized_case(8, 3, seed=9)
    keep = np.ones(24, bool)
    for f in (1, 2, 3, 4):
        keep[3 * f:3 * f + 3] = False
    assert all(np.array_equal(got[name][keep], host(plain)[name][keep]) for name in BC.OUTPUTS + ("grad_complex", "grad_log_scales"))
    assert np.array_equal(got["scaling"], host(plain)["scaling"])


# ---- what the kernels refuse ----------------------------------------------------------------------------------------------------------

def _args(case, cls=torch.Tensor, **changed):
    t = {k: torch.from_numpy(np.ascontiguousarray(case[k])).as_subclass(cls) for k in ("verts", "faces", "bary", "complex", "log_scales", "thickness")}
    t.update(changed)
    return [t[k] for k in ("verts", "faces", "bary", "complex", "log_scales", "thickness")]


def test_refusals_raise_value_error_with_their_reason():
    case = BC.sized_case(4, 3, seed=1)
    with pytest.raises(ValueError, match="must be on a GPU"):
        bound.bound_gaussians(*_args(case))
    t = lambda k: torch.from_numpy(case[k]).as_subclass(OnGpu)     # a device is asked for before a dtype or a shape: these say they are on one
    rand = lambda *shape: torch.rand(*shape).as_subclass(OnGpu)
    for changed, reason in ((dict(verts=t("verts").double()), "verts must be float32"),
                            (dict(faces=t("faces").int()), "faces must be int64"),
                            (dict(verts=t("verts")[:, :2]), r"verts must be \[V, 3\]"),
                            (dict(complex=t("complex")[:-1]), r"complex must be \[F G, 2\]"),
                            (dict(log_scales=t("log_scales").reshape(-1)), r"log_scales must be \[F G, 2\]"),
                            (dict(bary=rand(9, 3), complex=rand(36, 2), log_scales=rand(36, 2)), "at most 8"),
                            (dict(thickness=rand(2)), "thickness must hold one element"),
                            (dict(thickness=3.7e-6), "must be a torch.Tensor")):
        with pytest.raises(ValueError, match=reason):
            bound.bound_gaussians(*_args(case, OnGpu, **changed))
    with pytest.raises(ValueError, match="want must name"):
        bound.bound_gaussians(*_args(case), want=("normals",))
    with pytest.raises(ValueError, match="want must name"):
        bound.bound_gaussians(*_args(case), want=())


def test_cabi_refusals_need_no_device():
    from autovfx_amd import _lib
    L = _lib.lib
    assert L.gsr_bound_gaussians(-1, 1, 1, *[None] * 6, 0, None, None, None, None) == -1 and "negative count" in _lib.last_error()
    assert L.gsr_bound_gaussians(3, 1, 9, *[None] * 6, 0, None, None, None, None) == -1 and "G outside 1..8" in _lib.last_error()
    assert L.gsr_bound_gaussians(3, 1 << 29, 8, *[None] * 6, 0, None, None, None, None) == -1 and "2^31" in _lib.last_error()
    assert L.gsr_bound_gaussians(3, 0, 1, *[None] * 6, 0, None, None, None, None) == 0
    assert L.gsr_bound_gaussians(3, 1, 1, *[None] * 6, 0, None, None, None, None) == 0                     # nothing wanted
    assert L.gsr_bound_gaussians(3, 1, 1, *[None] * 6, 0, 4096, None, None, None) == -1 and "null pointer" in _lib.last_error()
    assert L.gsr_bound_gaussians(3, 1, 1, 4096, 4096, 4096, None, None, None, 0, 4098, None, None, None) == -1 and "misaligned" in _lib.last_error()
    assert L.gsr_bound_gaussians_backward(3, 1, 0, *[None] * 5, 0, *[None] * 7) == -1 and "G outside 1..8" in _lib.last_error()
    assert L.gsr_bound_gaussians_backward(3, 1, 1, *[None] * 5, 0, *[None] * 7) == -1 and "null pointer" in _lib.last_error()
    assert L.gsr_bound_gaussians_backward(0, 0, 1, *[None] * 5, 0, *[None] * 7) == 0


# ---- the hook -------------------------------------------------------------------------------------------------------------------------

NAMES = ("points", "scaling", "quaternions")


def _stub_sugar_module(name):
    mod = types.ModuleType(name)

    class SuGaR:
        binded_to_surface_mesh = False

        @property
        def points(self):
            return "reference points"

        @points.setter
        def points(self, value):
            self.set_points = value

        @property
        def scaling(self):
            return "reference scaling"

        @property
        def quaternions(self):
            return "reference quaternions"

        @property
        def surface_mesh(self):
            return None

        def get_covariance(self, **kwargs):
            return None

        def render_image_gaussian_rasterizer(self, **kwargs):
            return "reference render"

    SuGaR.__module__ = name
    mod.SuGaR = SuGaR
    return mod


def test_hook_replaces_the_three_properties_and_restores_them():
    import autovfx_amd
    from autovfx_amd import hook
    mod = _stub_sugar_module("stubbound.sugar_model")
    originals = {n: vars(mod.SuGaR)[n] for n in NAMES}
    render = vars(mod.SuGaR)["render_image_gaussian_rasterizer"]
    sys.modules[mod.__name__] = mod
    try:
        autovfx_amd.install(path=False)
        first = {n: vars(mod.SuGaR)[n] for n in NAMES}
        for n in NAMES:
            assert isinstance(first[n], property) and first[n] is not originals[n] and hook._is_ours(first[n].fget)
            assert vars(mod.SuGaR)["reference_" + n] is originals[n]
            assert first[n].fset is originals[n].fset and first[n].fdel is originals[n].fdel
        assert mod.__name__ in hook.patched_modules
        assert vars(mod.SuGaR)["render_image_gaussian_rasterizer"] is not render                  # the geometry-reuse wrapper, as before
        autovfx_amd.install(path=False)                                                           # a second install() changes nothing
        assert all(vars(mod.SuGaR)[n] is first[n] and vars(mod.SuGaR)["reference_" + n] is originals[n] for n in NAMES)
        m = mod.SuGaR()                                                                           # not bound: the reference's getters
        assert (m.points, m.scaling, m.quaternions) == ("reference points", "reference scaling", "reference quaternions")
        assert m.reference_points == "reference points"
        m.points = 5
        assert m.set_points == 5
        autovfx_amd.uninstall()
        assert all(vars(mod.SuGaR)[n] is originals[n] and "reference_" + n not in vars(mod.SuGaR) for n in NAMES)
        assert vars(mod.SuGaR)["render_image_gaussian_rasterizer"] is render
    finally:
        autovfx_amd.uninstall()
        sys.modules.pop(mod.__name__, None)


def test_hook_leaves_a_class_without_surface_mesh_alone():
    import autovfx_amd
    mod = _stub_sugar_module("otherbound.sugar_model")
    del mod.SuGaR.surface_mesh
    originals = {n: vars(mod.SuGaR)[n] for n in NAMES}
    sys.modules[mod.__name__] = mod
    try:
        autovfx_amd.install(path=False)
        assert all(vars(mod.SuGaR)[n] is originals[n] and not hasattr(mod.SuGaR, "reference_" + n) for n in NAMES)
    finally:
        autovfx_amd.uninstall()
        sys.modules.pop(mod.__name__, None)


def test_lenient_install_keeps_the_getters_when_the_library_cannot_load(capsys):
    import autovfx_amd
    from autovfx_amd import hook
    mod = _stub_sugar_module("lenientbound.sugar_model")
    sys.modules[mod.__name__] = mod
    try:
        hook.install(path=False, strict=False)
        with mock.patch.object(hook, "_load", side_effect=ImportError("libgsr_hip.so not found")):
            assert mod.SuGaR().quaternions == "reference quaternions"
        assert "bound Gaussians" in capsys.readouterr().err
        assert mod.SuGaR().points == "reference points"                                           # not retried
    finally:
        autovfx_amd.uninstall()
        sys.modules.pop(mod.__name__, None)


def test_a_cpu_model_and_the_excluded_flags_reach_the_original_getter():
    """The drop-ins decide from the model's flags and its tensors' descriptions: a recording original sees every such access."""
    case = BC.sized_case(4, 3, seed=2)
    seen = []
    getters = {n: getattr(bound, "drop_in_" + n)(lambda self, n=n: seen.append(n) or n) for n in NAMES}
    model = BC.StubSuGaR(case)                                                                    # on the CPU
    assert [getters[n](model) for n in NAMES] == list(NAMES) and seen == list(NAMES)
    for change in (dict(binded_to_surface_mesh=False), dict(editable=True), dict(scale_activation=torch.nn.functional.softplus)):
        model = BC.StubSuGaR(case)
        vars(model).update(change)
        reason = bound._why_original(model)
        assert reason and "GPU" not in reason, change
    assert getters["points"].fallback is not None and "SuGaR.points" in getters["points"].__doc__
