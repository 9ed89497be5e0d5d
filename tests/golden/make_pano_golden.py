"""Generate tests/golden/pano/c2e_*.npz from the REFERENCE's own ``c2e`` (sugar/gaussian_splatting/utils/py360_utils.py:7-65).
Run in the build container (needs /root/reference and scipy):

    python tests/golden/make_pano_golden.py

Each fixture stores six float32 faces ``[6, S, S, C]`` (the reference's dict order: front, right, back, left, up, down), the panorama
size and the reference's float64 ``c2e(faces, h, w, mode='bilinear', cube_format='dict')``.  The faces are noise plus a different
constant per face, so every seam tap is visible.  tests/test_panorama.py regenerates the outputs where the reference exists and checks
them against the committed files; tests/test_panorama_gpu.py checks the HIP kernel against them on the GPU box.  (They live in a
directory of their own: every tests/golden/*.npz outside the bw_ / ply_ prefixes is a rasterizer vector to tests/test_golden.py.)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pano")
FACE_ORDER = ("front", "right", "back", "left", "up", "down")
CASES = (("S5_8x16_c3", 5, 8, 16, 3, 11), ("S8_16x32_c4", 8, 16, 32, 4, 12), ("S16_24x64_c1", 16, 24, 64, 1, 13))


def faces_for(S: int, C: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    base = np.arange(1, 7, dtype=np.float32)[:, None, None, None] * 0.125
    return (base + 0.1 * rng.random((6, S, S, C))).astype(np.float32)


def reference_c2e(faces: np.ndarray, h: int, w: int) -> np.ndarray:
    from shims import reference_env
    with reference_env.reference_tree():
        from utils.py360_utils import c2e
        return c2e({k: faces[i] for i, k in enumerate(FACE_ORDER)}, h, w, mode="bilinear", cube_format="dict")


def path_of(name: str) -> str:
    return os.path.join(HERE, f"c2e_{name}.npz")


def main() -> None:
    os.makedirs(HERE, exist_ok=True)
    for name, S, h, w, C, seed in CASES:
        faces = faces_for(S, C, seed)
        np.savez_compressed(path_of(name), faces=faces, h=h, w=w, c2e=reference_c2e(faces, h, w))
        print(path_of(name))


if __name__ == "__main__":
    main()
