"""Which calls the kernels take: the words the modules in front of the HIP kernels share when they say so.

Every function that judges a call returns None when nothing stands against it, else the reason as a sentence that names the argument, what
was expected and what was got.  A check reads ``isinstance``, ``is_cuda``, ``device``, ``dtype``, ``dim()``, ``shape`` and nothing else of a
tensor: no data, no wait for the device, no GPU initialised.  Only :func:`capturing` needs the library, so a module asks it last: a call
refused for any other reason never loads it.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence, Tuple

import torch


def tensors(named: Sequence[Tuple[str, object, torch.dtype]], like=None, host: Optional[str] = None) -> Optional[str]:
    """``named``: ``(name, tensor, dtype)``.  Every one a ``torch.Tensor`` (settled for all before an attribute of any is read), then each in
    turn on a GPU, on ``like``'s device (the first one's without ``like``) and of its dtype.  ``host``: the function that does run on the
    CPU, for the reason to point to."""
    for name, t, _ in named:
        if not isinstance(t, torch.Tensor):
            return f"{name} must be a torch.Tensor, not {type(t).__name__}"
    device = (named[0][1] if like is None else like).device
    for name, t, dtype in named:
        if not t.is_cuda:
            return f"{name} must be on a GPU (got {t.device}); there is no CPU path, see {host or 'the *_host functions'}"
        if t.device != device:
            return f"{name} must be on {device} (got {t.device})"
        if t.dtype != dtype:
            return f"{name} must be {str(dtype).replace('torch.', '')} (got {t.dtype})"
    return None


def shaped(name: str, t: torch.Tensor, text: str, ok: bool) -> Optional[str]:
    """``ok``: whether ``t`` has the shape ``text`` describes."""
    return None if ok else f"{name} must be {text} (got {list(t.shape)})"


def mesh(verts, faces, host: Optional[str] = None) -> Optional[str]:
    """``verts [V, 3]`` float32 and ``faces [F, 3]`` int64 on one GPU.  How many of each is the caller's to limit."""
    return (tensors((("verts", verts, torch.float32), ("faces", faces, torch.int64)), host=host)
            or shaped("verts", verts, "[V, 3]", verts.dim() == 2 and verts.shape[1] == 3)
            or shaped("faces", faces, "[F, 3]", faces.dim() == 2 and faces.shape[1] == 3))


def gaussians(n: int, idx, centers, inv_scaled_rotation, strengths, max_k: int, n_name: str = "n") -> Optional[str]:
    """The shapes of a neighbour list over Gaussians, for tensors :func:`tensors` let through: ``idx [n, K]`` with ``1 <= K <= max_k``,
    ``centers [P, 3]``, ``inv_scaled_rotation [P, 3, 3]``, ``strengths [P]`` or ``[P, 1]``."""
    if idx.dim() != 2 or idx.shape[0] != n:
        return shaped("idx", idx, f"[{n_name}, K] with {n_name} = {n}", False)
    if not 1 <= idx.shape[1] <= max_k:
        return f"K must be in 1..{max_k} (got {idx.shape[1]})"
    if centers.dim() != 2 or centers.shape[1] != 3:
        return shaped("centers", centers, "[P, 3]", False)
    P = centers.shape[0]
    return (shaped("inv_scaled_rotation", inv_scaled_rotation, f"[P, 3, 3] with P = {P}", tuple(inv_scaled_rotation.shape) == (P, 3, 3))
            or shaped("strengths", strengths, f"[P] or [P, 1] with P = {P}", tuple(strengths.shape) in ((P,), (P, 1))))


def capturing(because: str) -> Optional[str]:
    """The one reason that needs the library, looked up on it at call time."""
    from . import _lib

    return f"the current stream is capturing a graph ({because})" if _lib.capturing() else None


def c(t: torch.Tensor) -> torch.Tensor:
    return t.detach().contiguous()


def cs(*ts: torch.Tensor) -> Tuple[torch.Tensor, ...]:
    return tuple(t.detach().contiguous() for t in ts)


def refuse(fn_name: str, why: Optional[str]) -> None:
    if why is not None:
        raise ValueError(f"{fn_name}: {why}")


def dressed(fn: Callable, name: str, original: Callable, target: str, where: str) -> Callable:
    """``fn``, a function of the calling module that runs ``original`` for the calls the kernels do not take, made up as what
    ``autovfx_amd.install()`` puts in place of ``target``.  The library is loaded here, so that a missing one shows when the patch is made."""
    from . import _lib  # noqa: F401

    fn.__name__ = fn.__qualname__ = name
    fn.fallback = original
    fn.__doc__ = (f"{target}: HIP kernels where they apply (autovfx_amd/{where}.py), "
                  f"{getattr(original, '__module__', '?')}.{getattr(original, '__name__', '?')} otherwise.")
    return fn
