"""Panoramas (autovfx_amd/panorama.py, the reference's render_panorama.py:100-145 and utils/py360_utils.py:7-65), CPU side.

* ``c2e_host`` -- the numpy restatement of the reference's ``c2e`` -- against the reference's own function (imported from the
  reference tree through tests/shims/reference_env.py), and against the committed golden outputs (tests/golden/pano/c2e_*.npz);
* the face-type map against ``equirect_facetype``; the cube cameras against ``create_cube_map_views``;
* the seam-padding map ``pad_source`` (the kernel's mapping, restated) against the reference's padded cube;
* the C ABI's refusals (no device needed: nothing is launched) and the tensor API's refusal of CPU tensors;
* the install() hook for modules named ``render_panorama``.

Reference-dependent cases skip where the reference tree is absent (the GPU box).
"""
import ctypes
import glob
import importlib
import os
import sys
import types
from unittest import mock

import numpy as np
import pytest
import torch

from autovfx_amd import panorama as pano

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from shims import reference_env  # noqa: E402

needs_reference = pytest.mark.skipif(not reference_env.available(), reason="reference tree not mounted")
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "pano", "c2e_*.npz")))


def _reference_py360():
    """The reference's ``c2e`` / ``equirect_facetype`` (only inside ``reference_env.reference_tree()``)."""
    from utils.py360_utils import c2e, equirect_facetype
    return c2e, equirect_facetype


def _face_dict(faces):
    return {k: faces[i] for i, k in enumerate(pano.FACE_ORDER)}


@needs_reference
@pytest.mark.parametrize("S", [2, 8, 33, 64])
def test_c2e_host_equals_the_reference(S):
    rng = np.random.default_rng(S)
    with reference_env.reference_tree():
        c2e, _ = _reference_py360()
        for h, w in ((8, 16), (16, 32), (24, 64), (64, 128)):
            for C in (1, 3, 4):
                faces = _face_dict(rng.random((6, S, S, C)).astype(np.float32))
                ref = c2e(faces, h, w, mode="bilinear", cube_format="dict")
                got = pano.c2e_host(faces, h, w)
                assert got.shape == ref.shape == (h, w, C) and got.dtype == np.float64
                assert np.abs(got - ref).max() <= 1e-12, (S, h, w, C)


@needs_reference
@pytest.mark.parametrize("S", [2, 8, 33])
def test_c2e_host_on_constant_faces_shows_every_seam(S):
    """One constant per face and channel: a tap that reads the wrong neighbour (or a pad the reference leaves at zero) shows."""
    with reference_env.reference_tree():
        c2e, _ = _reference_py360()
        for h, w in ((8, 16), (16, 32), (24, 64), (64, 128)):
            faces = _face_dict([np.full((S, S, 3), i + 1, np.float32) * np.array([1, 10, 100], np.float32) for i in range(6)])
            ref = c2e(faces, h, w, mode="bilinear", cube_format="dict")
            assert np.abs(pano.c2e_host(faces, h, w) - ref).max() <= 1e-12, (S, h, w)


@needs_reference
def test_pad_source_is_the_reference_padding():
    """Read through ``pad_source``, six faces of distinct texel ids give the reference's padded cube (sample_cubefaces) exactly."""
    with reference_env.reference_tree():
        import utils.py360_utils as py360
        captured = {}

        def spy(input, coordinates, **kw):
            captured["padded"] = np.array(input)
            return np.zeros(np.asarray(coordinates[0]).shape)

        for S in (2, 3, 7):
            ids = np.arange(1, 6 * S * S + 1, dtype=np.float64).reshape(6, S, S)
            with mock.patch.object(py360, "map_coordinates", spy):
                py360.sample_cubefaces(ids, np.zeros((2, 2), np.int32), np.zeros((2, 2)), np.zeros((2, 2)), order=1)
            nk, nr, nc = pano.pad_source(S)
            ours = np.where(nk >= 0, ids[np.maximum(nk, 0), nr, nc], 0.0)
            assert np.array_equal(ours, captured["padded"]), S


@needs_reference
def test_face_type_equals_equirect_facetype():
    with reference_env.reference_tree():
        _, equirect_facetype = _reference_py360()
        for h, w in ((2, 8), (3, 8), (8, 16), (16, 32), (24, 64), (7, 24), (64, 128), (512, 1024), (1024, 2048)):
            ref = equirect_facetype(h, w)
            got = pano.face_type(h, w)
            assert got.dtype == ref.dtype and np.array_equal(got, ref), (h, w)


@needs_reference
def test_cube_map_cameras_equal_the_reference():
    center = np.array([0.3, -1.2, 2.5])
    with reference_env.reference_tree():
        import render_panorama as rp
        with mock.patch.object(torch.Tensor, "to", lambda self, *a, **k: self):   # the reference's Camera moves its image to "cuda"
            ref = rp.create_cube_map_views(center, 64)
    ours = pano.cube_map_cameras(center, 64)
    assert list(ours) == list(ref) == list(pano.VIEW_ORDER)
    for name, r in ref.items():
        o = ours[name]
        for attr in ("world_view_transform", "projection_matrix", "full_proj_transform", "camera_center"):
            assert torch.equal(getattr(o, attr), getattr(r, attr)), (name, attr)
        assert (o.FoVx, o.FoVy, o.image_width, o.image_height, o.znear, o.zfar) == (r.FoVx, r.FoVy, r.image_width, r.image_height,
                                                                                    r.znear, r.zfar)


@needs_reference
def test_golden_files_are_the_references_output():
    """tests/golden/make_pano_golden.py, re-run against the reference: the committed outputs are what its c2e returns today."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    try:
        import make_pano_golden as mk
    finally:
        sys.path.remove(os.path.join(HERE, "golden"))
    assert len(GOLDEN) == len(mk.CASES)
    for name, S, h, w, C, seed in mk.CASES:
        g = np.load(mk.path_of(name))
        assert np.array_equal(g["faces"], mk.faces_for(S, C, seed))
        assert (int(g["h"]), int(g["w"])) == (h, w)
        assert np.array_equal(g["c2e"], mk.reference_c2e(g["faces"], h, w)), name


@pytest.mark.parametrize("path", GOLDEN, ids=os.path.basename)
def test_c2e_host_against_the_golden_files(path):
    g = np.load(path)
    got = pano.c2e_host(list(g["faces"]), int(g["h"]), int(g["w"]))
    assert np.abs(got - g["c2e"]).max() <= 1e-12


def test_face_type_rules():
    """Without the reference: the side faces take quarters of the width rolled by 3w/8, the poles mirror each other."""
    for h, w in ((8, 16), (64, 128), (1024, 2048)):
        tp = pano.face_type(h, w)
        assert set(np.unique(tp)) == set(range(6))
        assert np.array_equal(tp[::-1] == 5, tp == 4)
        mid = tp[h // 2]
        assert np.array_equal(mid, np.roll(np.repeat(np.arange(4), w // 4), 3 * w // 8))


def test_sizes_are_refused():
    for h, w in ((16, 20), (1, 16), (16, 0)):
        with pytest.raises(ValueError):
            pano.equirect_grid(h, w)


def test_abi_refuses_without_launching():
    """gsr_cube_to_equirect checks its arguments before it touches a device: w % 8, h < 2, S < 2, C, null pointers."""
    from autovfx_amd import _lib
    lib = _lib.lib
    fake = (ctypes.c_void_p * 6)(*([0x1000] * 6))
    none6 = (ctypes.c_void_p * 6)(*([0x1000] * 5 + [None]))
    g = 0x1000
    good = dict(faces=fake, S=8, C=4, depth=None, u=g, v=g, ceil=g, h=16, w=32, out=g, u8=None, od=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib.gsr_cube_to_equirect(a["faces"], a["S"], a["C"], a["depth"], a["u"], a["v"], a["ceil"], a["h"], a["w"], a["out"],
                                        a["u8"], a["od"], None)

    for bad in (dict(w=36), dict(w=0), dict(h=1), dict(S=1), dict(C=0), dict(C=5), dict(u=None), dict(ceil=None), dict(out=None),
                dict(faces=None), dict(faces=none6), dict(od=g), dict(od=g, depth=none6)):
        assert call(**bad) == -1, bad
        assert _lib.last_error()


def test_tensor_api_refuses_cpu_tensors():
    faces = [torch.zeros(4, 8, 8) for _ in range(6)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pano.cube_to_equirect(faces, 16, 32)
    with pytest.raises(ValueError):
        pano.cube_to_equirect(faces, 16, 36)


# ------------------------------------------------------------------------------------------------------------------------------------
# install(): modules named render_panorama
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def clean_hook():
    import autovfx_amd
    from autovfx_amd import hook
    parked = {n: sys.modules.pop(n) for n in [n for n in sys.modules if n.split(".")[-1] == "render_panorama"]}
    yield hook
    autovfx_amd.uninstall()
    for n in [n for n in sys.modules if n.split(".")[-1] == "render_panorama"]:
        del sys.modules[n]
    sys.modules.update(parked)


def _reference_like(*a, **k):
    return "reference"


def test_hook_patches_an_imported_render_panorama_module(clean_hook):
    import autovfx_amd
    mod = types.ModuleType("render_panorama")
    mod.render_panorama = _reference_like
    sys.modules["render_panorama"] = mod
    autovfx_amd.install(path=False)
    assert mod.render_panorama is pano.render_panorama
    assert mod.reference_render_panorama is _reference_like
    assert "render_panorama" in clean_hook.patched_modules
    autovfx_amd.uninstall()
    assert mod.render_panorama is _reference_like and not hasattr(mod, "reference_render_panorama")
    assert "render_panorama" not in clean_hook.patched_modules


def test_hook_patches_a_render_panorama_module_imported_later(clean_hook, tmp_path, monkeypatch):
    import autovfx_amd
    pkg = tmp_path / "gs_like"
    pkg.mkdir()
    (pkg / "__init__.py").write_text("")
    (pkg / "render_panorama.py").write_text("def render_panorama(gaussians, pipeline, background, center, output_dir, pano_h=1024, "
                                            "pano_w=2048):\n    return 'reference'\n")
    monkeypatch.syspath_prepend(str(tmp_path))
    autovfx_amd.install(path=False)
    try:
        mod = importlib.import_module("gs_like.render_panorama")
        assert mod.render_panorama is pano.render_panorama
        assert mod.reference_render_panorama(None, None, None, None, None) == "reference"
        assert "gs_like.render_panorama" in clean_hook.patched_modules
        autovfx_amd.uninstall()
        assert mod.render_panorama(None, None, None, None, None) == "reference"
    finally:
        sys.modules.pop("gs_like", None)
