"""The melting frame loop with ``AUTOVFX_AMD_MELT_CLOSEST=gpu`` against the default: a small melting scene whose module's ``o3d`` is a
double that answers with the contract's numpy restatement, rendered once per mode -- the same files, the same pixels and ``.npy`` bytes,
and in ``gpu`` mode the double is never asked."""
from __future__ import annotations

import os
import types

import numpy as np
import pytest

from autovfx_amd import frame_loop
from autovfx_amd.meshquery import closest_triangles_host

import meshquery_cases as cases
import test_frame_loop as tfl      # the scene mirror, the shims and the file comparison of the frame loop's own tests

pytestmark = pytest.mark.gpu
N_FRAMES = 3


class _Ids:
    def __init__(self, a):
        self._a = a

    def cpu(self):
        return self

    def numpy(self):
        return self._a


class _ExactScene:
    """``open3d.t.geometry.RaycastingScene`` as far as the loop uses it, answered by ``closest_triangles_host``."""
    asked, answers = [], []

    def add_triangles(self, mesh):
        self.verts, self.faces = np.asarray(mesh.vertices, np.float32), np.asarray(mesh.faces, np.int64)

    def compute_closest_points(self, points):
        type(self).asked.append(len(points))
        ids = closest_triangles_host(np.asarray(points, np.float32), self.verts, self.faces)[0]
        type(self).answers.append(ids)
        return {"primitive_ids": _Ids(ids)}


_o3d = types.SimpleNamespace(
    t=types.SimpleNamespace(geometry=types.SimpleNamespace(RaycastingScene=_ExactScene,
                                                           TriangleMesh=types.SimpleNamespace(from_legacy=lambda mesh: mesh))),
    core=types.SimpleNamespace(Tensor=types.SimpleNamespace(from_numpy=lambda a: a)))


def _scene_pair(tmp):
    ours, theirs, objects = tfl._gpu_scenes(tmp, n_frames=N_FRAMES, wh=(96, 54), P_base=6000, P_obj=3000)
    chair = objects[0]
    verts, faces = cases.cube_sphere(5, 0.3)                                       # 300 faces around the object's Gaussians
    tfl.trimesh_double.save_mesh(chair["object_path"], verts, faces)
    melting = os.path.join(tmp, "blender_cache", "blend", "melting_meshes", "chair")
    os.makedirs(melting)
    for i in range(N_FRAMES):                                                      # per frame a lower cap of the sphere, shrunk a little
        keep = verts[faces].mean(axis=1)[:, 2] < 0.2 - 0.15 * i
        tfl.trimesh_double.save_mesh(os.path.join(melting, "{0:03d}_obj.stl".format(i + 1)), verts * 0.97, faces[keep])
        if i == 1:
            side = verts[faces].mean(axis=1)[:, 0] > 0.15
            tfl.trimesh_double.save_mesh(os.path.join(melting, "{0:03d}_obj_dup.stl".format(i + 1)), verts * 1.02, faces[side])
    for s in (ours, theirs):
        s.blender_cache_dir = os.path.join(tmp, "blender_cache")
    return ours, theirs


def test_gpu_mode_writes_the_files_of_the_host_mode(tmp_path, monkeypatch):
    host, gpu = _scene_pair(str(tmp_path))
    monkeypatch.setattr(tfl, "o3d", _o3d)
    _ExactScene.asked, _ExactScene.answers = [], []
    monkeypatch.setenv("AUTOVFX_AMD_MELT_CLOSEST", "host")
    frame_loop.render_from_3DGS(host)
    assert len(_ExactScene.asked) == 1 + N_FRAMES + 1 and _ExactScene.asked[0] >= 3000     # the Gaussians once, then the centres
    kept = [int(np.isin(_ExactScene.answers[0], ids).sum()) for ids in _ExactScene.answers[1:]]
    assert all(0 < k < _ExactScene.asked[0] for k in kept) and len(set(kept)) > 1, kept      # the masks select: neither all nor none
    _ExactScene.asked = []
    monkeypatch.setenv("AUTOVFX_AMD_MELT_CLOSEST", "gpu")
    monkeypatch.setattr(_ExactScene, "__init__", lambda self: pytest.fail("gpu mode built the module's ray-casting scene"))
    frame_loop.render_from_3DGS(gpu)
    assert _ExactScene.asked == []
    tfl.assert_same_frame_files(gpu.traj_results_dir, host.traj_results_dir, N_FRAMES)
