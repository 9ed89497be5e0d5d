"""autovfx_amd._takes at each of its branches: the words every module in front of the HIP kernels judges a call with.  No GPU, no library
but for the capture check."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from autovfx_amd import _takes
from helpers import OnOtherGpu, fake_gpu

F32, I64 = torch.float32, torch.int64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _NoAttributes:
    """Whatever is read of it raises: a check that reaches past ``isinstance`` shows."""

    def __getattribute__(self, name):
        if name == "__class__":
            return _NoAttributes
        raise AssertionError(f"the check read .{name} of something that is no tensor")


def test_tensors_names_the_first_thing_wrong():
    a, i = fake_gpu(4, 3), fake_gpu(4, 2, dtype=I64)
    assert _takes.tensors((("a", a, F32), ("i", i, I64))) is None
    assert _takes.tensors((("a", a.t(), F32),)) is None                                      # a non-contiguous view is a tensor like another
    # no tensor: said before an attribute of any argument is read, whichever place it stands in
    for bad, word in ((np.zeros((4, 3), np.float32), "ndarray"), (None, "NoneType"), (_NoAttributes(), "_NoAttributes")):
        assert _takes.tensors((("a", a, F32), ("i", bad, I64))) == f"i must be a torch.Tensor, not {word}"
        assert _takes.tensors((("a", bad, F32), ("i", i, I64))) == f"a must be a torch.Tensor, not {word}"
        assert _takes.tensors((("a", _NoAttributes(), F32), ("i", bad, I64))).startswith("a must be a torch.Tensor")
    # a CPU tensor, with and without a host function to point to
    assert _takes.tensors((("a", torch.zeros(4, 3), F32),)) == "a must be on a GPU (got cpu); there is no CPU path, see the *_host functions"
    assert _takes.tensors((("a", a, F32), ("i", torch.zeros(4, dtype=I64), I64)), host="f_host") == \
        "i must be on a GPU (got cpu); there is no CPU path, see f_host"
    # another GPU: against the first tensor, and against ``like``
    other = fake_gpu(4, 3, cls=OnOtherGpu)
    assert _takes.tensors((("a", a, F32), ("b", other, F32))) == "b must be on cuda:0 (got cuda:1)"
    assert _takes.tensors((("b", other, F32), ("a", a, F32))) == "a must be on cuda:1 (got cuda:0)"
    assert _takes.tensors((("b", other, F32),)) is None
    assert _takes.tensors((("b", other, F32),), like=a) == "b must be on cuda:0 (got cuda:1)"
    assert _takes.tensors((("a", a, F32),), like=other) == "a must be on cuda:1 (got cuda:0)"
    # a dtype, for a float and for an index argument
    for dtype in (torch.float16, torch.float64, torch.int32, I64):
        assert _takes.tensors((("a", fake_gpu(4, 3, dtype=dtype), F32),)) == f"a must be float32 (got {dtype})"
    for dtype in (torch.int32, F32):
        assert _takes.tensors((("a", a, F32), ("i", fake_gpu(4, dtype=dtype), I64))) == f"i must be int64 (got {dtype})"
    assert _takes.tensors((("o", fake_gpu(4, dtype=I64), torch.int32),)) == "o must be int32 (got torch.int64)"


def test_tensors_order_of_reasons():
    """No tensor before no GPU before another device before another dtype, and per tensor in the order given."""
    a = fake_gpu(4, 3)
    cpu_f64, other_f64 = torch.zeros(4, 3, dtype=torch.float64), fake_gpu(4, 3, dtype=torch.float64, cls=OnOtherGpu)
    assert "torch.Tensor" in _takes.tensors((("a", cpu_f64, F32), ("b", None, F32)))
    assert "on a GPU" in _takes.tensors((("a", a, F32), ("b", cpu_f64, F32)))
    assert "must be on cuda:0" in _takes.tensors((("a", a, F32), ("b", other_f64, F32)))
    assert "must be float32" in _takes.tensors((("a", a, F32), ("b", fake_gpu(4, 3, dtype=torch.float64), F32)))
    assert _takes.tensors((("a", fake_gpu(4, 3, dtype=torch.float64), F32), ("b", cpu_f64, F32))).startswith("a must be float32")


def test_shaped():
    t = fake_gpu(5, 2)
    assert _takes.shaped("t", t, "[n, 2]", True) is None
    assert _takes.shaped("t", t, "[n, 3]", False) == "t must be [n, 3] (got [5, 2])"
    assert _takes.shaped("t", fake_gpu(()), "[n]", False) == "t must be [n] (got [])"


def test_mesh():
    verts, faces = fake_gpu(7, 3), fake_gpu(5, 3, dtype=I64)
    assert _takes.mesh(verts, faces) is None
    assert _takes.mesh(fake_gpu(0, 3), fake_gpu(0, 3, dtype=I64)) is None                    # nothing of either
    assert _takes.mesh(fake_gpu(3, 7).t(), fake_gpu(3, 5, dtype=I64).t()) is None            # non-contiguous: the caller copies
    for bad in (fake_gpu(7), fake_gpu(7, 3, 1), fake_gpu(7, 2), fake_gpu(7, 4)):             # rank - 1, rank + 1, last dimension 2 and 4
        assert _takes.mesh(bad, faces) == f"verts must be [V, 3] (got {list(bad.shape)})"
    for bad in (fake_gpu(5, dtype=I64), fake_gpu(5, 3, 1, dtype=I64), fake_gpu(5, 2, dtype=I64), fake_gpu(5, 4, dtype=I64)):
        assert _takes.mesh(verts, bad) == f"faces must be [F, 3] (got {list(bad.shape)})"
    assert _takes.mesh(verts, fake_gpu(5, 3, dtype=torch.int32)) == "faces must be int64 (got torch.int32)"
    assert _takes.mesh(fake_gpu(7, 3, dtype=torch.float64), faces) == "verts must be float32 (got torch.float64)"
    assert _takes.mesh(verts, fake_gpu(5, 3, dtype=I64, cls=OnOtherGpu)) == "faces must be on cuda:0 (got cuda:1)"
    assert _takes.mesh(torch.zeros(7, 3), faces, "mesh_host").endswith("see mesh_host")
    assert "torch.Tensor" in _takes.mesh(verts, None) and "torch.Tensor" in _takes.mesh(np.zeros((7, 3), np.float32), faces)


def test_gaussians():
    n, P, max_k = 5, 7, 16
    good = dict(idx=fake_gpu(n, 4, dtype=I64), centers=fake_gpu(P, 3), inv_scaled_rotation=fake_gpu(P, 3, 3), strengths=fake_gpu(P, 1))
    why = lambda **over: _takes.gaussians(n, max_k=max_k, **{**good, **over})
    assert why() is None and why(strengths=fake_gpu(P)) is None
    assert why(idx=fake_gpu(n, max_k, dtype=I64)) is None and why(idx=fake_gpu(n, 1, dtype=I64)) is None
    assert why(idx=fake_gpu(4, n, dtype=I64).t(), centers=fake_gpu(3, P).t()) is None         # non-contiguous
    assert _takes.gaussians(0, fake_gpu(0, 4, dtype=I64), fake_gpu(0, 3), fake_gpu(0, 3, 3), fake_gpu(0), max_k) is None
    assert why(idx=fake_gpu(n, 0, dtype=I64)) == "K must be in 1..16 (got 0)"
    assert why(idx=fake_gpu(n, max_k + 1, dtype=I64)) == "K must be in 1..16 (got 17)"
    for bad in (fake_gpu(n, dtype=I64), fake_gpu(n, 4, 1, dtype=I64), fake_gpu(n + 1, 4, dtype=I64), fake_gpu((), dtype=I64)):
        assert why(idx=bad) == f"idx must be [n, K] with n = 5 (got {list(bad.shape)})"
    assert _takes.gaussians(n, n_name="N", max_k=max_k, **{**good, "idx": fake_gpu(6, 4, dtype=I64)}) == "idx must be [N, K] with N = 5 (got [6, 4])"
    for bad in (fake_gpu(P), fake_gpu(P, 3, 1), fake_gpu(P, 2), fake_gpu(P, 4)):
        assert why(centers=bad) == f"centers must be [P, 3] (got {list(bad.shape)})"
    for bad in (fake_gpu(P, 3, 2), fake_gpu(P, 3), fake_gpu(P, 3, 3, 1), fake_gpu(P + 1, 3, 3), fake_gpu(P, 2, 3)):
        assert why(inv_scaled_rotation=bad) == f"inv_scaled_rotation must be [P, 3, 3] with P = 7 (got {list(bad.shape)})"
    for bad in (fake_gpu(P, 2), fake_gpu(P + 1), fake_gpu(P, 1, 1), fake_gpu(())):
        assert why(strengths=bad) == f"strengths must be [P] or [P, 1] with P = 7 (got {list(bad.shape)})"


def test_capturing_asks_the_library_at_call_time(monkeypatch):
    from autovfx_amd import _lib
    assert _takes.capturing("the call allocates") is None
    monkeypatch.setattr(_lib, "capturing", lambda: True)
    assert _takes.capturing("the call allocates") == "the current stream is capturing a graph (the call allocates)"


def test_a_refused_call_does_not_load_the_library():
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import torch\n"
            "from autovfx_amd import _takes\n"
            "assert 'GPU' in _takes.tensors((('x', torch.zeros(3), torch.float32),))\n"
            "assert 'GPU' in _takes.mesh(torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int64))\n"
            "try:\n"
            "    _takes.refuse('f', 'a reason')\n"
            "except ValueError:\n"
            "    pass\n"
            "assert 'autovfx_amd._lib' not in sys.modules, sorted(k for k in sys.modules if k.startswith('autovfx_amd'))\n"
            "print('ok')\n") % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]


def test_c_and_cs():
    t = fake_gpu(3, 5).t().requires_grad_()
    for got in (_takes.c(t),) + _takes.cs(t, t):
        assert got.is_contiguous() and not got.requires_grad and got.shape == t.shape
    plain = torch.zeros(4)
    assert _takes.c(plain).data_ptr() == plain.data_ptr() and _takes.cs() == ()


def test_refuse():
    assert _takes.refuse("f", None) is None
    with pytest.raises(ValueError, match=r"^f: x must be \[n\] \(got \[\]\)$"):
        _takes.refuse("f", "x must be [n] (got [])")


def test_dressed():
    def original(x):
        return x

    def wrapper(x):
        return original(x)

    got = _takes.dressed(wrapper, "op", original, "package._C.op", "module")
    assert got is wrapper and got.__name__ == got.__qualname__ == "op" and got.fallback is original
    assert got.__module__ == __name__
    assert got.__doc__ == f"package._C.op: HIP kernels where they apply (autovfx_amd/module.py), {__name__}.original otherwise."
    assert "?.?" in _takes.dressed(lambda: None, "op", object(), "t", "m").__doc__          # an original without a name still gets a sentence
