"""autovfx_amd.levelset on the GPU: the fused ray march against the float64 truth, held to the bars tests/levelset_cases.py derives from
the reference's own fp32 results; the shapes where the kernel could go wrong; the drop-in through install() against recorded runs of
the reference's own SuGaR.compute_level_surface_points_from_camera_fast."""
import ctypes
import sys
import types
from unittest import mock

import numpy as np
import pytest
import torch

import levelset_cases as LC
from levelset_cases import quaternion_apply, quaternion_invert      # noqa: F401  (the names the stub's "reference module" imported)
from test_levelset import LEVELS, SHAPES, shape_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32


def run_op(c, levels, S=21, range_size=3.0, want_normals=True, mangle=None):
    from autovfx_amd import levelset
    t = {k: torch.tensor(np.ascontiguousarray(c[k]), device=DEV) for k in ("origins", "dirs", "stds", "idx", "centers", "M", "strengths")}
    if mangle is not None:
        t = mangle(t)
    with torch.no_grad():
        out = levelset.level_surface(t["origins"], t["dirs"], t["stds"], t["idx"], t["centers"], t["M"], t["strengths"], levels, S, range_size,
                                     c["density_factor"], want_normals=want_normals, want_densities=True)
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}


@pytest.mark.parametrize("n,K,S,L,P", SHAPES)
def test_kernel_shapes(n, K, S, L, P):
    c = shape_case(n, K, S, L, P)
    got = run_op(c, LEVELS[L], S)
    assert got["hit"].shape == (L, n) and got["hit"].dtype == bool and got["normals"].shape == (L, n, 3) and got["densities"].shape == (n, S)
    LC.check(got, LC.truth(c, LEVELS[L], S), label=f"{n}x{K} S{S} L{L} P{P}")


def test_edge_rays_and_renormalised_densities():
    """Rays whose slots are all -1 or all one past the end, slots of both kinds among live ones, a zero standard deviation; then
    densities renormalised at 1."""
    c = shape_case(65, 16, 21, 3, 300)
    c["idx"][3] = -1
    c["idx"][4] = 300
    c["idx"][6] = np.iinfo(np.int64).max
    c["stds"][5] = 0
    got = run_op(c, LEVELS[3])
    assert not got["hit"][:, [3, 4, 5, 6]].any() and np.all(got["densities"][[3, 4, 6]] == 0)
    assert np.all(got["densities"][5] == got["densities"][5, 0])
    for key in ("t", "points", "normals"):
        assert np.all(got[key][:, [3, 4, 5, 6]] == 0)
    LC.check(got, LC.truth(c, LEVELS[3]), label="edge rays")
    c["idx"][7:30:2, 5] = -1              # live rays with missing slots: the normal pass skips them as the density pass does
    c["idx"][8:30:2, 9] = 300
    c["idx"][30:40, 1::2] = -1
    want = LC.truth(c, LEVELS[3])
    assert want["hit"][:, 7:40].any(1).all()
    LC.check(run_op(c, LEVELS[3]), want, label="missing slots")
    c = shape_case(65, 16, 21, 3, 300)
    c["density_factor"] = 40.0
    got = run_op(c, [0.5, 0.999])
    assert (got["densities"] == 1).mean() > 0.3 and got["densities"].max() == 1
    LC.check(got, LC.truth(c, [0.5, 0.999]), label="renormalised")


def test_without_normals_and_non_contiguous_inputs():
    c = shape_case(257, 16, 21, 3, 300)
    a, b = run_op(c, LEVELS[3]), run_op(c, LEVELS[3], want_normals=False)
    assert b["normals"] is None and all(np.array_equal(a[k], b[k]) for k in ("hit", "t", "points", "densities"))

    def mangle(t):
        wide = lambda v: torch.stack([v, v * 2], -1)[..., 0]
        out = {k: wide(v) for k, v in t.items()}
        assert not any(v.is_contiguous() for k, v in out.items() if v.numel() > 1 and k != "strengths")
        return out

    m = run_op(c, LEVELS[3], mangle=mangle)
    assert all(np.array_equal(a[k], m[k]) for k in ("hit", "t", "points", "normals", "densities"))


@pytest.mark.parametrize("with_normals", [True, False])
def test_c_abi_writes_every_output_element(with_normals):
    """Straight through ctypes on a side stream, every output and the scratch prefilled with 0xFF bytes; a NULL output is not written."""
    from autovfx_amd import _lib
    n, K, P, S, Lv = 321, 17, 40, 21, 3
    c = shape_case(n, K, S, Lv, P)
    t = {k: torch.tensor(np.ascontiguousarray(c[k]), device=DEV) for k in ("origins", "dirs", "stds", "idx", "centers", "M", "strengths")}
    ff = lambda *shape: torch.full(shape, 255, dtype=torch.uint8, device=DEV)
    hit, tt, pts, nrm, dens = ff(Lv, n), ff(Lv, n * 4).view(torch.float32), ff(Lv, n, 12).view(torch.float32), ff(Lv, n, 12).view(torch.float32), ff(n, S * 4).view(torch.float32)
    nbytes = _lib.lib.gsr_field_scratch_bytes(P)
    scratch = ff(nbytes)
    rng = torch.linspace(-3.0, 3.0, S).to(DEV)
    levels = (ctypes.c_float * 8)(*LEVELS[3])
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    rc = _lib.lib.gsr_level_surface(n, K, P, S, Lv, t["origins"].data_ptr(), t["dirs"].data_ptr(), t["stds"].data_ptr(), t["idx"].data_ptr(),
                                    t["centers"].data_ptr(), t["M"].data_ptr(), t["strengths"].data_ptr(), c["density_factor"], rng.data_ptr(),
                                    ctypes.byref(levels), hit.data_ptr(), tt.data_ptr(), pts.data_ptr(), nrm.data_ptr() if with_normals else None,
                                    dens.data_ptr(), scratch.data_ptr(), nbytes, ctypes.c_void_p(side.cuda_stream))
    assert rc == 0, _lib.last_error()
    side.synchronize()
    assert bool((hit <= 1).all()) and not torch.isnan(tt).any() and not torch.isnan(pts).any() and not torch.isnan(dens).any()
    assert not torch.isnan(nrm).any() if with_normals else bool(torch.isnan(nrm).all())
    got = dict(hit=hit.cpu().numpy(), t=tt.cpu().numpy(), points=pts.cpu().numpy(), normals=nrm.cpu().numpy(), densities=dens.cpu().numpy())
    LC.check(got, LC.truth(c, LEVELS[3], S), label="C ABI", normals=with_normals)


@pytest.mark.parametrize("name", LC.FIXTURES)
def test_kernel_on_the_reference_fixtures(name):
    fx = LC.fixture(name)
    got = run_op(LC.fixture_case(name), fx["levels"], fx["n_points_in_range"], fx["range_size"])
    print(f"reference's own fp32 density error {LC.reference_density_error(name):.3e}")
    LC.check(got, LC.fixture_truth(name), LC.density_bar(name), label=name)


# ---- the drop-in through install(), on a class shaped like the reference's ----
def _stub_module(calls):
    mod = types.ModuleType("stublevelgpu.sugar_model")

    class SuGaR(LC.StubModel):
        def compute_level_surface_points_from_camera_fast(self, *args, **kwargs):
            calls.append(kwargs)
            return "reference march"

        def compute_density(self, x, **kwargs):
            raise AssertionError("not on this path")

        def get_covariance(self, return_full_matrix=False, return_sqrt=False, inverse_scales=False):
            return LC.StubModel.get_covariance(self, return_full_matrix, return_sqrt, inverse_scales)

    SuGaR.__module__ = mod.__name__
    mod.SuGaR = SuGaR
    return mod


@pytest.fixture
def installed():
    import autovfx_amd
    calls = []
    mod = _stub_module(calls)
    sys.modules[mod.__name__] = mod
    try:
        autovfx_amd.install(path=False)
        assert hasattr(mod.SuGaR, "reference_compute_level_surface_points_from_camera_fast")
        yield mod.SuGaR, calls
    finally:
        autovfx_amd.uninstall()
        sys.modules.pop(mod.__name__, None)
    assert not hasattr(mod.SuGaR, "reference_compute_level_surface_points_from_camera_fast")


def _march(model, fx, rasterizer, **kw):
    args = dict(nerf_cameras=model.cameras, cam_idx=0, rasterizer=rasterizer, surface_levels=fx["levels"], n_surface_points=fx["n_surface_points"],
                density_factor=fx["density_factor"], return_pixel_idx=True, return_gaussian_idx=True, return_normals=True)
    args.update(kw)
    with torch.no_grad():
        return model.compute_level_surface_points_from_camera_fast(**args)


@pytest.mark.parametrize("name", LC.FIXTURES)
def test_drop_in_through_install_against_the_reference_fixtures(name, installed):
    SuGaR, calls = installed
    fx = LC.fixture(name)
    model, rasterizer = SuGaR(fx, DEV), LC.StubRasterizer(fx["zbuf"], fx["pix_to_face"], DEV)
    drawn = []

    def randperm(n, *a, **k):
        drawn.append(n)
        assert n == len(fx["perm"])
        return torch.tensor(fx["perm"])

    with mock.patch("torch.randperm", randperm):
        out = _march(model, fx, rasterizer)
    assert len(drawn) == (1 if fx["perm"].size else 0) and rasterizer.calls == 1 and model.texture_calls == 1 and model.splat_calls == 1
    assert not calls and list(out) == fx["levels"]
    want, ref, bar_d = LC.fixture_truth(name), LC.reference_dense(name), LC.density_bar(name)
    n = want["hit"].shape[1]
    # the rows the reference kept, in its order: pixel_idx and gaussian_idx of every ray, from the fixture's own inputs
    H, W = int(fx["H"]), int(fx["W"])
    seen = fx["zbuf"][..., 0].reshape(-1) >= 0
    order = fx["perm"][:n] if fx["perm"].size else np.arange(n)
    pixel_of = np.arange(H * W)[seen][order]
    gaussian_of = (fx["pix_to_face"][..., 0].reshape(-1) // int(fx["n_tri"]))[seen][order]
    got = {"hit": np.zeros((len(fx["levels"]), n), bool), "t": None, "points": np.zeros((len(fx["levels"]), n, 3), F),
           "normals": np.zeros((len(fx["levels"]), n, 3), F)}
    near = LC.near_level(want, bar_d)
    for l, level in enumerate(fx["levels"]):
        o = out[level]
        assert list(o) == ["intersection_points", "pixel_idx", "gaussian_idx", "normals"]
        assert all(o[k].dtype == torch.tensor(fx[f"out{l}.{k}"]).dtype and o[k].device.type == torch.device(DEV).type for k in o)
        pix = o["pixel_idx"].cpu().numpy()
        rows = np.searchsorted(np.sort(pixel_of), pix)
        rows = np.argsort(pixel_of)[rows]                      # the ray of each returned row
        assert np.array_equal(pixel_of[rows], pix) and np.all(np.diff(rows) > 0)          # compacted in the reference's order
        assert np.array_equal(o["gaussian_idx"].cpu().numpy(), gaussian_of[rows])
        got["hit"][l][rows] = True
        got["points"][l][rows] = o["intersection_points"].cpu().numpy()
        got["normals"][l][rows] = o["normals"].cpu().numpy()
        far = ~near[l]
        assert np.array_equal(got["hit"][l][far], ref["hit"][l][far])
        if not near[l].any():                                  # then the nested dict has the reference's very rows
            assert np.array_equal(pix, fx[f"out{l}.pixel_idx"]) and np.array_equal(o["gaussian_idx"].cpu().numpy(), fx[f"out{l}.gaussian_idx"])
    # t is not returned: recover it for the check from the truth's own rows (points and normals carry the comparison)
    got["t"] = np.where(got["hit"], want["t"], 0)
    LC.check(got, want, bar_d, label="drop-in " + name)
    # only the keys asked for
    with mock.patch("torch.randperm", randperm):
        assert list(_march(model, fx, rasterizer, return_pixel_idx=False, return_gaussian_idx=False, return_normals=False)[fx["levels"][0]]) == ["intersection_points"]


def test_refused_calls_reach_the_original_with_the_generator_untouched(installed):
    SuGaR, calls = installed
    fx = LC.fixture(LC.FIXTURES[0])
    model, rasterizer = SuGaR(fx, DEV), LC.StubRasterizer(fx["zbuf"], fx["pix_to_face"], DEV)
    state = torch.get_rng_state()
    refused = [dict(compute_intersection_for_flat_gaussian=True), dict(compute_flat_normals=True), dict(just_use_depth_as_level=True),
               dict(use_gaussian_depth=True), dict(n_points_in_range=33), dict(surface_levels=[0.1] * 9), dict(density_factor=torch.tensor(1.0))]
    for kw in refused:
        assert _march(model, fx, rasterizer, n_surface_points=100, **kw) == "reference march"
    model.knn_to_track = 65
    assert _march(model, fx, rasterizer, n_surface_points=100) == "reference march"
    cpu = SuGaR(fx, "cpu")
    assert _march(cpu, fx, rasterizer, n_surface_points=100) == "reference march"
    assert len(calls) == len(refused) + 2 and all(k["n_surface_points"] == 100 for k in calls) and calls[4]["n_points_in_range"] == 33
    assert torch.equal(torch.get_rng_state(), state) and rasterizer.calls == 0 and model.texture_calls == 0


def test_a_refusal_after_the_draw_gives_the_generator_back(installed):
    """The model's own camera returns float64 world points: the kernel does not take them, which shows only after torch.randperm.  The
    original then runs from the generator state the call found."""
    SuGaR, calls = installed
    fx = LC.fixture(LC.FIXTURES[0])
    model, rasterizer = SuGaR(fx, DEV), LC.StubRasterizer(fx["zbuf"], fx["pix_to_face"], DEV)
    camera = model.cameras.p3d_cameras[0]
    unproject = camera.unproject_points
    camera.unproject_points = lambda *a, **k: unproject(*a, **k).double()
    state = torch.get_rng_state()
    assert _march(model, fx, rasterizer, n_surface_points=100) == "reference march"
    assert len(calls) == 1 and rasterizer.calls == 1 and torch.equal(torch.get_rng_state(), state)
