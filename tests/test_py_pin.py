"""The preprocess stage held to the reference's own importable Python (tests/golden/pypin/, tests/golden/make_py_fixtures.py).

The reference restates three parts of its preprocess kernel in Python: the SH colour (``eval_sh``, render()'s
``convert_SHs_python`` branch), the 3D covariance (``get_covariance``, the ``compute_cov3D_python`` branch) and the camera
matrices (``getWorld2View2`` / ``getProjectionMatrix`` / ``Camera``).  The fixtures hold what those functions computed -- in
fp32, as render() hands it to the rasterizer, and in fp64 as the truth -- for clouds and cameras chosen where the stage goes
wrong.  Here the CPU oracle's ``sh_to_rgb`` / ``cov3d_from_scale_rot`` and this package's camera code are held to them.

Bit equality with the reference's fp32 Python is the wrong bar (its operation order -- ``bmm``, ``norm``, division -- is not
the kernel's); the bars are against the fp64 truth, per element, and no worse than twice the reference's own fp32 error.
"""
import glob
import os

import numpy as np
import pytest
import torch

from autovfx_amd import cameras
from oracle import cpu_oracle

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pypin")
CASES = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(HERE, "*.npz")) if "cameras" not in p)
EPS = float(np.finfo(np.float32).eps)
COV_ULPS, SH_ULPS = 16.0, 4.0       # per-element bars: cov3D e <= 16 eps rowmax|Sigma|, SH e <= 4 eps s


def load(name):
    with np.load(os.path.join(HERE, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def oracle_inputs(f, *, precomp=False):
    """The call render() makes: the getters' outputs (plain mode) or the Python-prep tuple (``precomp``)."""
    kw = dict(means3D=f["raw_xyz"], opacities=f["get_opacity"], width=int(f["image_width"]), height=int(f["image_height"]),
              viewmatrix=f["viewmatrix"], projmatrix=f["projmatrix"], campos=f["campos"], tanfovx=float(f["tanfovx"]),
              tanfovy=float(f["tanfovy"]), sh_degree=int(f["sh_degree"]), scale_modifier=float(f["scale_modifier"]))
    if precomp:
        kw.update(colors_precomp=f["colors_precomp"], cov3D_precomp=f["cov3D_precomp"])
    else:
        kw.update(shs=np.concatenate((f["raw_features_dc"], f["raw_features_rest"]), 1), scales=f["get_scaling"],
                  rotations=f["get_rotation"])
    return kw


def sh_errors(rgb, f, rows):
    """Per-element |rgb - clamp(truth, 0)| / (eps s) on ``rows``."""
    want = np.maximum(f["truth_sh_pre"], 0.0)
    return np.abs(rgb.astype(np.float64) - want)[rows] / (EPS * f["truth_sh_scale"][rows])


def cov_errors(cov, f, rows):
    """Per-element |cov - truth| / (eps rowmax|truth|) on ``rows``."""
    t = f["truth_cov3D"][rows]
    return np.abs(cov.astype(np.float64)[rows] - t) / (EPS * np.abs(t).max(1, keepdims=True))


def check_sh(name, rgb, clamped, f, rows):
    """The SH bar, shared with the GPU test: per element 4 eps s, the maximum no worse than max(2 x the reference's fp32
    Python, 1 eps), and the same values clamped to 0 (except where the fp64 pre-clamp value is within the bar of 0).
    Returns (max error, reference max error) in units of eps s."""
    e, e_ref = sh_errors(rgb, f, rows), sh_errors(f["colors_precomp"], f, rows)
    assert e.max() <= SH_ULPS, f"{name}: SH error {e.max():.2f} eps s > {SH_ULPS}"
    assert e.max() <= max(2.0 * e_ref.max(), 1.0), f"{name}: SH error {e.max():.2f} > 2 x reference {e_ref.max():.2f} (eps s)"
    pre = f["truth_sh_pre"][rows]
    near = np.abs(pre) <= SH_ULPS * EPS * f["truth_sh_scale"][rows]
    theirs = f["colors_precomp"][rows] == 0.0
    differ = (clamped[rows] != theirs) & ~near
    assert not differ.any(), f"{name}: clamp decisions differ at {np.argwhere(differ)[:5].tolist()}"
    assert (clamped[rows] == (pre < 0))[~near].all(), f"{name}: clamp decisions differ from the fp64 truth"
    return float(e.max()), float(e_ref.max())


@pytest.fixture(scope="module")
def fixtures():
    assert CASES, "tests/golden/pypin/ holds no fixtures"
    return {n: load(n) for n in CASES}


@pytest.mark.parametrize("name", CASES)
def test_oracle_preprocess_against_the_reference_python(name, fixtures):
    f = fixtures[name]
    out = cpu_oracle.preprocess(**oracle_inputs(f))
    vis = out["radii"] > 0
    assert vis.sum() >= 20, f"{name}: only {vis.sum()} visible Gaussians"
    # cov3D
    e, e_ref = cov_errors(out["cov3D_out"], f, vis), cov_errors(f["cov3D_precomp"], f, vis)
    assert e.max() <= COV_ULPS, f"{name}: cov3D error {e.max():.2f} eps rowmax > {COV_ULPS}"
    assert e.max() <= max(2.0 * e_ref.max(), 1.0), f"{name}: cov3D error {e.max():.2f} > 2 x reference {e_ref.max():.2f}"
    # SH colour (the oracle's clamp decisions: its ``clamped`` output)
    sh, sh_ref = check_sh(name, out["rgb"], out["clamped"].astype(bool), f, vis)
    print(f"{name}: visible {vis.sum()}/{vis.size}  cov3D {e.max():.2f} (ref {e_ref.max():.2f}) eps rowmax  "
          f"SH {sh:.2f} (ref {sh_ref:.2f}) eps s  clamped {int(out['clamped'][vis].sum())}")


@pytest.mark.parametrize("name", CASES)
def test_oracle_precomputed_path_is_the_same_geometry(name, fixtures):
    """The Python-prep tuple through the oracle: same radii as its own scale / rotation / SH path except where the fp64 radius
    3 sqrt(lambda_max) sits on an integer, and the colours pass through untouched."""
    f = fixtures[name]
    a = cpu_oracle.preprocess(**oracle_inputs(f))
    b = cpu_oracle.preprocess(**oracle_inputs(f, precomp=True))
    edge = radius_on_integer(f)
    np.testing.assert_array_equal(a["radii"][~edge], b["radii"][~edge])
    vis = b["radii"] > 0
    np.testing.assert_array_equal(b["depths"][vis], a["depths"][vis])
    np.testing.assert_array_equal(b["means2D"][vis], a["means2D"][vis])


def radius_on_integer(f, rel=1e-5):
    """Rows whose fp64 screen radius 3 sqrt(lambda_max) (forward.cu:74-113,217-222 in double, from the truth cov3D) lies within
    ``rel`` of an integer: there a last-bit difference of the covariance may move ceil() by one."""
    V = f["viewmatrix"].astype(np.float64).reshape(4, 4).T          # stored transposed
    p = f["raw_xyz"].astype(np.float64)
    t = p @ V[:3, :3].T + V[:3, 3]
    W, H = int(f["image_width"]), int(f["image_height"])
    tx, ty = float(np.float32(f["tanfovx"])), float(np.float32(f["tanfovy"]))
    fx, fy = W / (2.0 * tx), H / (2.0 * ty)
    z = t[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        x = np.clip(t[:, 0] / z, -1.3 * tx, 1.3 * tx) * z
        y = np.clip(t[:, 1] / z, -1.3 * ty, 1.3 * ty) * z
        J = np.zeros((len(p), 2, 3))
        J[:, 0, 0], J[:, 0, 2] = fx / z, -fx * x / (z * z)
        J[:, 1, 1], J[:, 1, 2] = fy / z, -fy * y / (z * z)
        c = f["truth_cov3D"]
        S = np.stack((c[:, [0, 1, 2]], c[:, [1, 3, 4]], c[:, [2, 4, 5]]), 1)
        T = J @ V[:3, :3][None]
        C = T @ S @ T.transpose(0, 2, 1)
        a, b, d = C[:, 0, 0] + 0.3, C[:, 0, 1], C[:, 1, 1] + 0.3
        mid = 0.5 * (a + d)
        r = 3.0 * np.sqrt(mid + np.sqrt(np.maximum(0.1, mid * mid - (a * d - b * b))))
        return (z > 0.2) & (np.abs(r - np.round(r)) <= rel * r)


# ---- cameras ----------------------------------------------------------------------------------------------------------------

def camera_rows():
    f = load("cameras")
    return [{k: v[i] for k, v in f.items()} for i in range(len(f["names"]))]


@pytest.mark.parametrize("i", range(6))
def test_camera_matrices_equal_the_reference(i):
    c = camera_rows()[i]
    R, T, trans, scale = c["R"], c["T"], c["trans"], float(c["scale"])
    fovx, fovy, zn, zf = float(c["FoVx"]), float(c["FoVy"]), float(c["znear"]), float(c["zfar"])
    # getWorld2View2 and getProjectionMatrix: the same float64 / float32 operations in the same order -- bit for bit
    np.testing.assert_array_equal(cameras.world_to_view(R, T, trans, scale), c["getWorld2View2"])
    np.testing.assert_array_equal(cameras.projection_matrix(zn, zf, fovx, fovy).numpy(), c["getProjectionMatrix"])
    # the reference Camera's matrices (scene/cameras.py): transposes, a bmm and an inverse of the above
    wv = torch.tensor(cameras.world_to_view(R, T, trans, scale)).transpose(0, 1).contiguous()
    np.testing.assert_array_equal(wv.numpy(), c["world_view_transform"])
    if np.all(trans == 0) and scale == 1.0:
        cam = cameras.Camera.from_Rt(R, T, fovx, fovy, int(c["width"]), int(c["height"]), znear=zn, zfar=zf)
        for k in ("world_view_transform", "projection_matrix", "full_proj_transform"):
            np.testing.assert_array_equal(getattr(cam, k).numpy(), c[k], err_msg=k)
        # camera_center = world_view_transform.inverse()[3, :3]: the reference inverts the transposed view (a strided tensor),
        # this package its contiguous copy, and the LU runs in another order -- the same centre to within one rounding
        centre = c["camera_center"].astype(np.float64)
        np.testing.assert_allclose(cam.camera_center.numpy(), centre, rtol=0, atol=2 * EPS * max(1.0, np.abs(centre).max()))
    else:
        # from_Rt has no translate / scale; the centre the reference derives by inverting its float32 view matrix is
        # the float64 one, rounded, to within the inverse's rounding
        centre = (np.linalg.inv(np.vstack((np.hstack((R.T, T[:, None])), [0, 0, 0, 1])))[:3, 3] + trans) * scale
        np.testing.assert_allclose(c["camera_center"], centre, rtol=0, atol=8 * EPS * max(1.0, np.abs(centre).max()))


def test_case_cameras_are_the_camera_fixtures():
    """Each case's viewmatrix / projmatrix / campos are the reference Camera's for its pose (cameras.npz)."""
    rows = camera_rows()
    for name in CASES:
        f, c = load(name), rows[int(load(name)["camera_index"])]
        np.testing.assert_array_equal(f["viewmatrix"], c["world_view_transform"], err_msg=name)
        np.testing.assert_array_equal(f["projmatrix"], c["full_proj_transform"], err_msg=name)
        np.testing.assert_array_equal(f["campos"], c["camera_center"], err_msg=name)


# ---- drift guard ------------------------------------------------------------------------------------------------------------

from test_render_mirror import needs_reference  # noqa: E402


@needs_reference
def test_fixtures_regenerate_to_the_committed_arrays():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_py_fixtures", os.path.join(os.path.dirname(HERE), "make_py_fixtures.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    fresh = gen.build()
    assert sorted(fresh) == sorted(CASES + ["cameras"])
    for name, arrays in fresh.items():
        old = load(name)
        assert sorted(arrays) == sorted(old), name
        for k, v in arrays.items():
            np.testing.assert_array_equal(np.asarray(v), old[k], err_msg=f"{name}.{k}")
