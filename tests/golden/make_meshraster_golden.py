"""Generate tests/golden/meshraster/huge_z_37x53.npz: the mesh z-buffer's contract on a scene whose finite depths (z times 1e19) overflow
the perspective correction's products, recorded from ``autovfx_amd.meshraster.rasterize_face_verts_host`` once the kernels had been seen
to give the same bits on an MI355X (tests/test_meshraster_gpu.py::test_huge_finite_coordinates).  There the contract's ``min`` and
``max`` must be C's ``fminf`` / ``fmaxf``: with numpy's NaN-propagating ``minimum`` / ``maximum`` every output differs.

    python tests/golden/make_meshraster_golden.py

tests/test_meshraster.py::test_huge_depths_are_pinned holds the restatement to the file.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import meshraster_cases as cases  # noqa: E402
from autovfx_amd.meshraster import rasterize_face_verts_host  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    H, W, n_faces, seed = cases.SCENES[0]
    fv = cases.scaled_scene(n_faces, seed, z_scale=1e19)
    face, z, bary, dists = rasterize_face_verts_host(fv, *cases.one_mesh(fv), (H, W), 0.0, 10, perspective_correct=True, clip_barycentric_coords=True)
    path = os.path.join(HERE, "meshraster", "huge_z_37x53.npz")
    np.savez_compressed(path, face_verts=fv, pix_to_face=face.astype(np.int16), zbuf=z, bary_coords=bary, dists=dists)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
