"""``simple_knn._C`` -- the extension-module surface of the reference (``ext.cpp`` binds one function, ``distCUDA2``), backed by the
HIP kernels of libgsr_hip.so (``autovfx_amd/knn.py``, C ABI ``gsr_knn3_mean_dist``).

``distCUDA2(points)``: float32 ``[P, 3]`` on a GPU -> float32 ``[P]``, the mean squared distance of every point to its three nearest
neighbours, queued on torch's current stream.  Non-contiguous input is made contiguous, as the reference does.  Deliberate
differences: a CPU tensor and a shape other than ``[P, 3]`` are refused with an exception before anything is
launched.  There is no fallback: importing this module raises when the library is missing or of another ABI.
"""
from __future__ import annotations

import torch

from autovfx_amd import _lib  # noqa: F401  (loads and checks libgsr_hip.so: no library, no module)
from autovfx_amd.knn import mean_dist3


def distCUDA2(points: torch.Tensor) -> torch.Tensor:
    return mean_dist3(points)
