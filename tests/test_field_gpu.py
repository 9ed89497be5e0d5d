"""autovfx_amd.field on the GPU: the fused density field and its backward against the float64 truth, held to the bars tests/field_cases.py
derives from the reference's own fp32 results; the cases where the kernels could go wrong; the drop-ins through install()."""
import ctypes
import math
import sys
import types
from unittest import mock

import numpy as np
import pytest
import torch

import field_cases as FC
from autovfx_amd.field import field_values
from test_field import random_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
NAMES = ("x", "centers", "inv_scaled_rotation", "strengths", "min_scaling")


def run_op(c, ups=("g_density", "g_opacities", "g_beta"), grads=NAMES, flat_strengths=False, mangle=None, density_factor=None, want_opacities=True,
           want_beta=True):
    """The op on case ``c``: outputs and the gradients of sum(g * output) over the upstream gradients named in ``ups``."""
    from autovfx_amd import field
    t = {"x": c["x"], "centers": c["centers"], "inv_scaled_rotation": c["M"], "strengths": c["strengths"].reshape(-1) if flat_strengths else c["strengths"],
         "min_scaling": c["min_scaling"]}
    t = {k: torch.tensor(v, device=DEV) for k, v in t.items()}
    idx = torch.tensor(c["idx"], device=DEV)
    if mangle is not None:
        t, idx = mangle(t, idx)
    for k in grads:
        t[k].requires_grad_(True)
    df = c["density_factor"] if density_factor is None else density_factor
    d, o, b = field.field_values(t["x"], idx, t["centers"], t["inv_scaled_rotation"], t["strengths"], t["min_scaling"] if want_beta else None, df,
                                 want_opacities=want_opacities, want_beta=want_beta)
    got = {k: (None if v is None else v.detach().cpu().numpy()) for k, v in (("density", d), ("opacities", o), ("beta", b))}
    loss = sum((torch.tensor(c["ups"][u], device=DEV) * out).sum() for u, out in (("g_density", d), ("g_opacities", o), ("g_beta", b)) if u in ups)
    if grads and ups:
        loss.backward()
    got["grad"] = {k: (None if t[k].grad is None else t[k].grad.cpu().numpy()) for k in NAMES}
    return got


def truth_of(c, ups=("g_density", "g_opacities", "g_beta")):
    return FC.truth(c["x"], c["idx"], c["centers"], c["M"], c["strengths"], c["min_scaling"], c["density_factor"],
                    **{u: c["ups"][u] for u in ups})


def check(c, label, **kw):
    ups = kw.get("ups", ("g_density", "g_opacities", "g_beta"))
    got, want = run_op(c, **kw), truth_of(c, ups)
    FC.check_forward(got, want, label=label)
    bad = (c["idx"] < 0) | (c["idx"] >= len(c["centers"]))
    assert np.all(got["opacities"][bad] == 0)
    FC.check_grads({k: v for k, v in got["grad"].items() if k in kw.get("grads", NAMES)}, want, label=label)
    return got, want


SHAPES = [(N, 16, 300) for N in (1, 63, 64, 65, 257, 4099)] + [(257, K, 300) for K in (1, 3, 17)] + [(65, 3, 1), (65, 3, 2), (4099, 17, 2), (1, 1, 1)]


@pytest.mark.parametrize("N,K,P", SHAPES)
def test_forward_and_backward_shapes(N, K, P):
    check(random_case(N, K, P, seed=1000 + N + K + P), f"{N}x{K}/{P}")


@pytest.mark.parametrize("ups", [("g_density",), ("g_opacities",), ("g_beta",), ("g_density", "g_opacities"), ("g_density", "g_opacities", "g_beta")])
def test_upstream_gradients_one_at_a_time(ups, monkeypatch):
    """An output that the loss does not use reaches gsr_field_backward as a NULL upstream gradient, not as a tensor of zeros."""
    from autovfx_amd import _lib
    seen, real = [], _lib.lib

    class Watch:
        def __getattr__(self, name):
            fn = getattr(real, name)
            return (lambda *a: (seen.append(tuple(p is not None for p in a[10:13])), fn(*a))[1]) if name == "gsr_field_backward" else fn

    with monkeypatch.context() as m:
        m.setattr(_lib, "lib", Watch())
        got, _ = check(random_case(257, 16, 300, seed=7), "+".join(ups), ups=ups)
    assert seen == [tuple(u in ups for u in ("g_density", "g_opacities", "g_beta"))]
    if ups == ("g_beta",):
        assert all(np.all(got["grad"][k] == 0) for k in ("x", "centers", "inv_scaled_rotation", "strengths"))
    else:
        assert (np.all(got["grad"]["min_scaling"] == 0)) == ("g_beta" not in ups)


@pytest.mark.parametrize("want_opacities,want_beta", [(False, False), (True, False), (False, True)])
def test_outputs_not_asked_for(want_opacities, want_beta):
    """``compute_density``'s call shape and the two between it and the trainers': the kernels run without the opacity and beta outputs,
    without min_scaling and without their upstream gradients, and are held to the same truth."""
    c = random_case(257, 16, 300, seed=17)
    ups = ("g_density",) + (("g_opacities",) if want_opacities else ()) + (("g_beta",) if want_beta else ())
    got, want = run_op(c, ups=ups, want_opacities=want_opacities, want_beta=want_beta), truth_of(c, ups)
    assert (got["opacities"] is None) == (not want_opacities) and (got["beta"] is None) == (not want_beta)
    FC.check_forward(got, want, label=f"opacities {want_opacities}, beta {want_beta}")
    if want_beta:
        FC.check_grads(got["grad"], want, label="with beta")
    else:
        assert got["grad"].pop("min_scaling") is None
        FC.check_grads(got["grad"], want, label="without beta")


def test_inputs_that_need_no_gradient_get_none():
    c = random_case(257, 16, 300, seed=8)
    got, _ = check(c, "no dx", grads=("centers", "strengths"))
    assert got["grad"]["x"] is None and got["grad"]["inv_scaled_rotation"] is None and got["grad"]["min_scaling"] is None
    got = run_op(c, grads=())
    assert all(v is None for v in got["grad"].values())


def test_flat_strengths_and_non_contiguous_inputs():
    c = random_case(257, 16, 300, seed=9)
    a, _ = check(c, "strengths [P]", flat_strengths=True)
    assert a["grad"]["strengths"].shape == (300,)

    def mangle(t, idx):
        wide = lambda v: torch.stack([v, v * 2], -1)[..., 0]                       # every tensor a strided view
        out = {k: wide(v) for k, v in t.items()}
        out["inv_scaled_rotation"] = t["inv_scaled_rotation"].transpose(1, 2).contiguous().transpose(1, 2)
        assert not any(v.is_contiguous() for k, v in out.items() if v.numel() > 1 and k != "strengths") and not wide(idx).is_contiguous()
        return out, wide(idx)

    b, _ = check(c, "non-contiguous", mangle=mangle)
    assert np.array_equal(a["density"], b["density"]) and np.array_equal(a["opacities"], b["opacities"])
    assert b["grad"]["strengths"].shape == (300, 1)


def test_every_slot_on_one_gaussian():
    """4 099 x 16 pairs, all adding into one accumulator line."""
    c = random_case(4099, 16, 300, seed=10, bad_slots=False)
    c["idx"][:] = 17
    got, _ = check(c, "one Gaussian")
    rest = np.arange(300) != 17
    assert all(np.all(got["grad"][k].reshape(300, -1)[rest] == 0) for k in ("centers", "inv_scaled_rotation", "strengths", "min_scaling"))


def test_duplicates_and_out_of_range_slots():
    c = random_case(257, 16, 300, seed=11, bad_slots=False)
    c["idx"][:, 1::2] = c["idx"][:, 0::2]                 # every neighbour twice
    c["idx"][::3, 5] = -1
    c["idx"][1::3, 6] = 300
    c["idx"][5] = -1                                      # a sample with no neighbour at all
    c["idx"][6, :] = np.iinfo(np.int64).max
    got, _ = check(c, "duplicates, -1 and P")
    assert got["density"][5] == 0 and got["beta"][5] == 0 and np.all(got["grad"]["x"][5] == 0) and got["density"][6] == 0


def test_far_sample_centre_sample_and_clamped_scale():
    """q > 1e8: sigma exp(-5e7) = 0 and gradients exactly 0.  q == 0: the strength itself.  A scale at get_covariance's 1e-8 clamp: matrix
    entries of 1e8, q far above 1e8 for any sample off the centre."""
    c = random_case(65, 3, 4, seed=12, bad_slots=False)
    c["M"][3] = (c["M"][3].astype(np.float64) / np.linalg.norm(c["M"][3].astype(np.float64), axis=0) * np.array([5.0, 5.0, 1e8])).astype(F)
    c["idx"][:] = np.array([0, 1, 2])
    c["idx"][0] = 0
    c["x"][0] = c["centers"][0] + F(3000.0)              # far: q > 1e8
    c["idx"][1] = 1
    c["x"][1] = c["centers"][1]                           # at the centre: q == 0
    c["idx"][2] = 3
    c["x"][2] = c["centers"][3] + F(0.01)                 # off the centre of the Gaussian with the clamped scale
    c["idx"][3] = 3
    c["x"][3] = c["centers"][3]                           # and on it
    got, _ = check(c, "far / centre / clamped scale")
    assert got["density"][0] == 0 and np.all(got["grad"]["x"][0] == 0)
    assert np.all(got["opacities"][1] == F(c["density_factor"]) * c["strengths"][1, 0])
    assert got["density"][2] == 0 and np.all(got["grad"]["x"][2] == 0)
    assert np.all(got["opacities"][3] == F(c["density_factor"]) * c["strengths"][3, 0])
    assert np.all(np.isfinite(got["grad"]["inv_scaled_rotation"]))


def _abi_call(c, N, K, P, stream=None, null=()):
    """gsr_field_forward and gsr_field_backward straight through ctypes, every output prefilled with 0xFF bytes; the optional pointers
    named in ``null`` are passed as NULL."""
    from autovfx_amd import _lib
    L = _lib.lib
    t = {k: torch.tensor(np.ascontiguousarray(v), device=DEV) for k, v in (("x", c["x"]), ("idx", c["idx"]), ("c", c["centers"]), ("M", c["M"]),
                                                                             ("s", c["strengths"]), ("m", c["min_scaling"]))}
    ups = {k: torch.tensor(v, device=DEV) for k, v in c["ups"].items()}
    ff = lambda *shape: torch.full(shape, 255, dtype=torch.uint8, device=DEV).view(torch.float32)
    density, opac, beta, dx = ff(N * 4), ff(N, K * 4), ff(N * 4), ff(N, 12)
    accum = torch.zeros(P, 16, device=DEV)
    nbytes = L.gsr_field_scratch_bytes(P)
    scratch = torch.full((nbytes,), 255, dtype=torch.uint8, device=DEV)
    s = ctypes.c_void_p(stream.cuda_stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    ptr = lambda name, tensor: None if name in null else tensor.data_ptr()
    ins = (N, K, P, t["x"].data_ptr(), t["idx"].data_ptr(), t["c"].data_ptr(), t["M"].data_ptr(), t["s"].data_ptr(), ptr("min_scaling", t["m"]),
           c["density_factor"])
    assert L.gsr_field_forward(*ins, density.data_ptr(), ptr("opacities", opac), ptr("beta", beta), scratch.data_ptr(), nbytes, s) == 0, _lib.last_error()
    assert L.gsr_field_backward(*ins, ptr("g_density", ups["g_density"]), ptr("g_opacities", ups["g_opacities"]), ptr("g_beta", ups["g_beta"]),
                                ptr("dx", dx), accum.data_ptr(), scratch.data_ptr(), nbytes, s) == 0, _lib.last_error()
    return density, opac, beta, dx, accum


@pytest.mark.parametrize("null", [("g_density",), ("g_opacities",), ("g_beta",), ("opacities",), ("beta",), ("dx",), ("g_density", "g_beta"),
                                  ("opacities", "beta", "g_opacities", "g_beta", "min_scaling"), ("g_density", "g_opacities", "g_beta")],
                         ids="+".join)
def test_c_abi_with_optional_pointers_null(null):
    """Every optional pointer of the two calls as NULL, one at a time and in the combinations the binding produces (the last but one is
    ``compute_density``'s): a NULL upstream gradient counts as zeros, a NULL output is not written (its 0xFF prefill stays), the rest is
    held to the float64 truth."""
    N, K, P = 321, 17, 40
    c = random_case(N, K, P, seed=18)
    density, opac, beta, dx, accum = _abi_call(c, N, K, P, null=null)
    torch.cuda.synchronize()
    want = FC.truth(c["x"], c["idx"], c["centers"], c["M"], c["strengths"], c["min_scaling"], c["density_factor"],
                    **{u: c["ups"][u] for u in ("g_density", "g_opacities", "g_beta") if u not in null})
    outs = {"density": density, "opacities": opac, "beta": beta}
    for name in ("opacities", "beta", "dx"):
        if name in null:
            assert torch.isnan({**outs, "dx": dx}[name]).all(), name
    if "min_scaling" in null:
        want["beta"] = None
    FC.check_forward({k: (None if k in null else v.cpu().numpy()) for k, v in outs.items()}, want, label="C ABI, NULL " + "+".join(null))
    a = accum.cpu().numpy()
    got = {"x": None if "dx" in null else dx.cpu().numpy(), "centers": a[:, 0:3], "inv_scaled_rotation": a[:, 3:12], "strengths": a[:, 12],
           "min_scaling": a[:, 13]}
    FC.check_grads(got, want, label="C ABI, NULL " + "+".join(null))
    if "g_beta" in null:
        assert np.all(a[:, 13] == 0)
    if "g_density" in null and "g_opacities" in null:
        assert np.all(a[:, :13] == 0) and ("dx" in null or np.all(got["x"] == 0))
    assert np.all(a[:, 14:] == 0)


def test_every_output_element_is_written():
    N, K, P = 321, 17, 40
    c = random_case(N, K, P, seed=13)
    density, opac, beta, dx, accum = _abi_call(c, N, K, P)
    torch.cuda.synchronize()
    for name, out in (("density", density), ("opacities", opac), ("beta", beta), ("dx", dx), ("accum", accum)):
        assert not torch.isnan(out).any(), name
    want = truth_of(c)
    FC.check_forward(dict(density=density.cpu().numpy(), opacities=opac.cpu().numpy(), beta=beta.cpu().numpy()), want, label="C ABI")
    a = accum.cpu().numpy()
    FC.check_grads({"x": dx.cpu().numpy(), "centers": a[:, 0:3], "inv_scaled_rotation": a[:, 3:12], "strengths": a[:, 12], "min_scaling": a[:, 13]},
                   want, label="C ABI")
    assert np.all(a[:, 14:] == 0)


def test_side_stream():
    c = random_case(4099, 16, 300, seed=15)
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        got = run_op(c)
    side.synchronize()
    main = run_op(c)
    assert np.array_equal(got["density"], main["density"]) and np.array_equal(got["opacities"], main["opacities"])
    FC.check_grads(got["grad"], truth_of(c), label="side stream")


@pytest.mark.parametrize("name", FC.FIXTURES)
def test_reference_fixtures(name):
    fx = FC.fixture(name)
    avg = fx["beta_mode"] == "average"
    c = dict(x=fx["x"], idx=fx["idx"], centers=fx["points"], M=fx["inv_scaled_rotation"], strengths=fx["strengths"], min_scaling=fx["min_scaling"],
             density_factor=fx["density_factor"], ups={k: fx[k] for k in ("g_density", "g_opacities", "g_beta")})
    ups = ("g_density", "g_opacities", "g_beta") if avg else ("g_density", "g_opacities")
    got, want = run_op(c, ups=ups), FC.fixture_truth(name, avg)
    if not avg:
        got["beta"] = None
        got["grad"].pop("min_scaling")
    print("reference's own fp32 errors:", FC.reference_forward_errors(name))
    FC.check_forward(got, want, FC.forward_bars(name), label=name)
    FC.check_grads(got["grad"], want, label=name)


# ---- the drop-ins through install(), on a class shaped like the reference's ----
def _stub_module(c, beta_mode):
    mod = types.ModuleType("stubfield.sugar_model")
    put = lambda a: torch.tensor(a, device=DEV)

    class SuGaR:
        """What the drop-ins read of a SuGaR model, with the density field in dense torch expressions."""

        def __init__(self):
            self.points, self.strengths, self._M = put(c["centers"]).requires_grad_(), put(c["strengths"]).requires_grad_(), put(c["M"]).requires_grad_()
            self.scaling = put(np.stack([c["min_scaling"], c["min_scaling"] * 2, c["min_scaling"] * 3], 1)).requires_grad_()
            self.knn_idx, self.beta_mode, self.knn_to_track, self.nearest_calls = put(c["idx"]), beta_mode, c["idx"].shape[1], 0

        def get_covariance(self, return_full_matrix=False, return_sqrt=False, inverse_scales=False):
            assert return_full_matrix and return_sqrt and inverse_scales
            return self._M

        def get_gaussians_closest_to_samples(self, x, n_closest_gaussian=None):
            self.nearest_calls += 1
            return self.knn_idx

        def get_beta(self, x, closest_gaussians_idx=None, closest_gaussians_opacities=None, densities=None, opacity_min_clamp=1e-32):
            m = self.scaling.min(dim=-1)[0][closest_gaussians_idx]
            if self.beta_mode == "average":
                return m.mean(dim=1)
            total = closest_gaussians_opacities.sum(dim=-1, keepdim=True)
            return (m * (closest_gaussians_opacities / total.clamp(min=opacity_min_clamp))).sum(dim=-1)

        def _dense(self, x, idx, strengths, centers, M, density_factor):
            w = (M[idx].transpose(-1, -2) @ (x[:, None] - centers[idx])[..., None])[..., 0]
            o = density_factor * strengths[idx][..., 0] * torch.exp(-0.5 * (w * w).sum(-1).clamp(0.0, 1e8))
            return o.sum(-1), o

        def compute_density(self, x, closest_gaussians_idx=None, density_factor=1., return_closest_gaussian_opacities=False):
            idx = self.get_gaussians_closest_to_samples(x) if closest_gaussians_idx is None else closest_gaussians_idx
            d, o = self._dense(x, idx, self.strengths, self.points, self.get_covariance(True, True, True), density_factor)
            return (d, o) if return_closest_gaussian_opacities else d

        def get_field_values(self, x, gaussian_idx=None, closest_gaussians_idx=None, gaussian_strengths=None, gaussian_centers=None,
                             gaussian_inv_scaled_rotation=None, return_sdf=True, density_threshold=1., density_factor=1., return_sdf_grad=False,
                             sdf_grad_max_value=10., opacity_min_clamp=1e-16, return_closest_gaussian_opacities=False, return_beta=False):
            idx = self.knn_idx[gaussian_idx] if closest_gaussians_idx is None else closest_gaussians_idx
            d, o = self._dense(x, idx, self.strengths if gaussian_strengths is None else gaussian_strengths,
                               self.points if gaussian_centers is None else gaussian_centers,
                               self.get_covariance(True, True, True) if gaussian_inv_scaled_rotation is None else gaussian_inv_scaled_rotation,
                               density_factor)
            fields = {"density": d.clone()}
            d = torch.where(d >= 1, d / (d.detach() + 1e-12), d)
            if return_closest_gaussian_opacities:
                fields["closest_gaussian_opacities"] = o
            beta = self.get_beta(x, closest_gaussians_idx=idx, closest_gaussians_opacities=o, densities=d, opacity_min_clamp=opacity_min_clamp)
            if return_beta:
                fields["beta"] = beta
            if return_sdf:
                fields["sdf"] = beta * (torch.sqrt(-2 * torch.log(d.clamp(min=opacity_min_clamp))) - math.sqrt(-2 * math.log(min(density_threshold, 1.))))
            if return_sdf_grad:
                fields["sdf_grad"] = torch.zeros_like(x)
            return fields

    SuGaR.__module__ = mod.__name__
    mod.SuGaR = SuGaR
    return mod


@pytest.mark.parametrize("beta_mode", ["average", "weighted_average"])
def test_drop_ins_through_install(beta_mode):
    import autovfx_amd
    c = random_case(513, 16, 300, seed=16, bad_slots=False)
    mod = _stub_module(c, beta_mode)
    sys.modules[mod.__name__] = mod
    try:
        autovfx_amd.install(path=False)
        S = mod.SuGaR
        assert hasattr(S, "reference_compute_density") and hasattr(S, "reference_get_field_values")
        m = S()
        x = torch.tensor(c["x"], device=DEV, requires_grad=True)
        rel = FC.forward_bars_relative()
        near = lambda a, b, key: float((a - b).detach().abs().max()) <= 2 * rel[key] * float(b.detach().abs().max())       # two fp32 results: both errors
        kw = dict(return_sdf=True, density_factor=0.9, return_closest_gaussian_opacities=True, return_beta=True)
        from autovfx_amd import field
        op_outputs = []
        with mock.patch.object(field, "field_values", lambda *a, **k: (op_outputs.append(field_values(*a, **k)), op_outputs[-1])[1]):
            ours = m.get_field_values(x, gaussian_idx=torch.arange(513, device=DEV), **kw)
        ref = m.reference_get_field_values(x, gaussian_idx=torch.arange(513, device=DEV), **kw)
        assert list(ours) == list(ref) == ["density", "closest_gaussian_opacities", "beta", "sdf"]
        assert all(ours[k].shape == ref[k].shape and ours[k].dtype == ref[k].dtype for k in ref)
        assert near(ours["density"], ref["density"], "density") and near(ours["closest_gaussian_opacities"], ref["closest_gaussian_opacities"], "opacities")
        assert near(ours["beta"], ref["beta"], "beta") if beta_mode == "average" else torch.allclose(ours["beta"], ref["beta"], rtol=1e-5, atol=0)
        # density is a fresh tensor: a copy of the kernel's sum that shares storage with nothing else, taken before the >= 1 renormalisation
        (op_density, op_opacities, _), = op_outputs
        own = lambda t: (t.untyped_storage().data_ptr(), t.untyped_storage().nbytes())
        assert ours["density"]._base is None and own(ours["density"])[1] == 513 * 4
        assert all(own(ours["density"])[0] != own(t)[0] for t in (op_density, op_opacities, ours["closest_gaussian_opacities"], ours["beta"], ours["sdf"]))
        assert ours["closest_gaussian_opacities"] is op_opacities
        saturated = op_density >= 1
        assert saturated.any() and not saturated.all()
        assert torch.equal(ours["density"], op_density) and bool((ours["density"][saturated] >= 1).all()) and float(ours["density"].detach().max()) > 1
        d = ours["density"].detach()
        renorm = torch.where(d >= 1, d / (d + 1e-12), d)
        want_sdf = ours["beta"].detach() * (torch.sqrt(-2 * torch.log(renorm.clamp(min=1e-16))) - 0.0)
        assert torch.equal(ours["sdf"].detach(), want_sdf) and bool((ours["sdf"][saturated].abs() <= 1e-3 * ours["beta"][saturated]).all())
        if beta_mode == "weighted_average":       # beta is get_beta's, from the op's opacities (the same expression twice: a few ulp)
            again = m.get_beta(x, closest_gaussians_idx=m.knn_idx, closest_gaussians_opacities=ours["closest_gaussian_opacities"], opacity_min_clamp=1e-16)
            assert torch.allclose(ours["beta"], again, rtol=1e-6, atol=0)
        # gradients flow into the model through the drop-in (the sdf itself has NaN gradients where a density was renormalised to 1)
        (ours["density"].sum() + ours["closest_gaussian_opacities"].sum() + ours["beta"].sum()).backward()
        g_ours = [t.grad.clone() for t in (x, m.points, m._M, m.strengths, m.scaling)]
        for t in (x, m.points, m._M, m.strengths, m.scaling):
            t.grad = None
        (ref["density"].sum() + ref["closest_gaussian_opacities"].sum() + ref["beta"].sum()).backward()
        for a, t in zip(g_ours, (x, m.points, m._M, m.strengths, m.scaling)):
            assert torch.allclose(a, t.grad, rtol=1e-3, atol=1e-4 * float(t.grad.abs().max()))
        # only the keys asked for
        assert list(m.get_field_values(x, closest_gaussians_idx=m.knn_idx, return_sdf=False)) == ["density"]
        # compute_density: one tensor, or two; the neighbour search is the model's own
        dens = m.compute_density(x)
        assert m.nearest_calls == 1 and dens.shape == (513,)
        dens2, opac2 = m.compute_density(x, closest_gaussians_idx=m.knn_idx, density_factor=0.9, return_closest_gaussian_opacities=True)
        assert torch.equal(dens2, ours["density"]) and torch.equal(opac2, ours["closest_gaussian_opacities"])
        assert near(dens, m.reference_compute_density(x), "density")
        assert all(own(ours["density"])[0] != own(t)[0] for t in (dens, dens2, opac2))
        # ... so writing into it in place changes nothing else: not the kernel's own outputs, the other fields, or a second call
        kept = {k: v.detach().clone() for k, v in ours.items() if k != "density"}
        kept_op = op_density.detach().clone()
        ours["density"].detach().fill_(-7.0)
        assert all(torch.equal(ours[k].detach(), v) for k, v in kept.items()) and torch.equal(op_density.detach(), kept_op)
        dens3, opac3 = m.compute_density(x, closest_gaussians_idx=m.knn_idx, density_factor=0.9, return_closest_gaussian_opacities=True)
        assert torch.equal(dens3, dens2) and torch.equal(opac3, opac2)
        again = m.get_field_values(x, gaussian_idx=torch.arange(513, device=DEV), **kw)
        assert torch.equal(again["density"], dens2) and all(torch.equal(again[k], v) for k, v in kept.items())
        # what the kernels do not take runs the reference: return_sdf_grad, CPU tensors
        assert "sdf_grad" in m.get_field_values(x, closest_gaussians_idx=m.knn_idx, return_sdf_grad=True)
        cpu = S.__new__(S)
        for k, v in vars(m).items():
            setattr(cpu, k, v.detach().cpu() if isinstance(v, torch.Tensor) else v)
        on_cpu = cpu.get_field_values(x.detach().cpu(), closest_gaussians_idx=cpu.knn_idx, return_beta=True)
        assert on_cpu["density"].device.type == "cpu" and list(on_cpu) == ["density", "beta", "sdf"]
        assert near(on_cpu["density"], m.get_field_values(x, closest_gaussians_idx=m.knn_idx, return_sdf=False)["density"].cpu(), "density")
        assert cpu.compute_density(x.detach().cpu(), closest_gaussians_idx=cpu.knn_idx).device.type == "cpu"
    finally:
        autovfx_amd.uninstall()
        sys.modules.pop(mod.__name__, None)
    assert not hasattr(mod.SuGaR, "reference_compute_density")
