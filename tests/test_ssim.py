"""The SSIM drop-in without a GPU: the PyTorch restatement against the reference's ``loss_utils.ssim`` bit for bit, the window the
kernels get, the calls that go to the fallback, ``install()`` on a miniature tree and on the reference's own module, and the C ABI's
refusals."""
from __future__ import annotations

import importlib
import importlib.util
import os
import subprocess
import sys
import textwrap

import pytest
import torch

import autovfx_amd
from autovfx_amd import hook
from autovfx_amd import ssim as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/sugar"
REF_LOSS_UTILS = [os.path.join(REF, "gaussian_splatting", "utils", "loss_utils.py"), os.path.join(REF, "sugar_utils", "loss_utils.py")]
mounted = pytest.mark.skipif(not all(os.path.isfile(p) for p in REF_LOSS_UTILS), reason="the reference tree is not mounted")


def load_reference(path):
    spec = importlib.util.spec_from_file_location(f"reference_loss_utils_{abs(hash(path))}", path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def images(shape, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g).to(dtype)


@mounted
@pytest.mark.parametrize("path", REF_LOSS_UTILS)
@pytest.mark.parametrize("shape,size_average", [((3, 33, 47), True), ((2, 4, 20, 25), True), ((2, 4, 20, 25), False),
                                                ((1, 1, 9, 1), True), ((4, 12, 13), True)])
def test_restatement_equals_the_reference_bitwise(path, shape, size_average):
    ref = load_reference(path)
    a, b = images(shape, 1), images(shape, 2)
    assert torch.equal(S.ssim_restated(a, b, 11, size_average), ref.ssim(a, b, 11, size_average))
    assert torch.equal(S.ssim_restated(a, b, 5, size_average), ref.ssim(a, b, 5, size_average))
    x1, x2 = a.clone().requires_grad_(True), a.clone().requires_grad_(True)
    S.ssim_restated(x1, b, 11, size_average).sum().backward()
    ref.ssim(x2, b, 11, size_average).sum().backward()
    assert torch.equal(x1.grad, x2.grad)


@mounted
def test_kernel_window_is_the_reference_gaussian_bitwise():
    ref = load_reference(REF_LOSS_UTILS[0])
    want = ref.gaussian(11, 1.5)
    assert want.dtype == torch.float32
    assert torch.equal(S.gaussian_window(), want)
    assert torch.equal(torch.tensor(list(S.WINDOW11), dtype=torch.float32), want)


def test_kernel_window_is_normalised_and_symmetric():
    w = torch.tensor(list(S.WINDOW11), dtype=torch.float32)
    assert torch.equal(w, w.flip(0)) and abs(float(w.double().sum()) - 1.0) < 1e-6 and len(S.WINDOW11) == 11


FALLBACKS = {
    "cpu": lambda: (images((3, 16, 18), 3), images((3, 16, 18), 4), 11, True),
    "cpu_batch_per_image": lambda: (images((2, 3, 16, 18), 3), images((2, 3, 16, 18), 4), 11, False),
    "float64": lambda: (images((3, 16, 18), 3, torch.float64), images((3, 16, 18), 4, torch.float64), 11, True),
    "window_7": lambda: (images((3, 16, 18), 3), images((3, 16, 18), 4), 7, True),
    "3d_per_image": lambda: (images((3, 16, 18), 3), images((3, 16, 18), 4), 11, False),
    "mismatched_shapes": lambda: (images((3, 16, 18), 3), images((3, 16, 17), 4), 11, True),
    "2d_input": lambda: (images((16, 18), 3), images((16, 18), 4), 11, True),
    "float16": lambda: (images((3, 16, 18), 3, torch.float16), images((3, 16, 18), 4, torch.float16), 11, True),
}


def outcome(fn, args):
    try:
        return fn(*args)
    except Exception as e:   # the type is what must agree
        return type(e)


@mounted
@pytest.mark.parametrize("case", sorted(FALLBACKS))
def test_fallback_cases_give_the_reference_result_or_exception(case):
    ref = load_reference(REF_LOSS_UTILS[0])
    args = FALLBACKS[case]()
    assert not S._fused_takes(*args)
    ours, theirs = outcome(S.ssim, args), outcome(ref.ssim, args)
    if isinstance(theirs, type):
        assert ours is theirs
    else:
        assert torch.equal(ours, theirs)
    wrapped = S.drop_in(ref.ssim)                     # as install() builds it around the reference's own
    again = outcome(wrapped, args)
    assert again is theirs if isinstance(theirs, type) else torch.equal(again, theirs)


def test_fused_path_is_refused_where_it_does_not_apply():
    a = images((3, 8, 8), 5)
    assert not S._fused_takes(a, a, 11, True)          # CPU tensors
    assert not S._fused_takes(a, "a", 11, True)


LOSS_UTILS_SRC = """\
def create_window(window_size, channel):
    return 'window'

def _ssim(img1, img2, window, window_size, channel, size_average=True):
    return 'inner'

def ssim(img1, img2, window_size=11, size_average=True):
    return 'reference'

def l1_loss(a, b):
    return 'l1'
"""


@pytest.fixture
def fake_tree(tmp_path, monkeypatch):
    """utils/loss_utils.py as the reference has it, a trainer that imports ``ssim`` from it, and a ``loss_utils`` without an ``ssim``
    trio (which is left alone)."""
    mine = lambda n: n.split(".")[0] in ("utils", "trainer_like", "other_pkg")
    parked = {n: sys.modules.pop(n) for n in [n for n in sys.modules if mine(n)]}
    (tmp_path / "utils").mkdir()
    (tmp_path / "utils" / "__init__.py").write_text("")
    (tmp_path / "utils" / "loss_utils.py").write_text(LOSS_UTILS_SRC)
    (tmp_path / "trainer_like.py").write_text("from utils.loss_utils import l1_loss, ssim\nfrom utils.loss_utils import ssim as metric\n")
    (tmp_path / "other_pkg").mkdir()
    (tmp_path / "other_pkg" / "__init__.py").write_text("")
    (tmp_path / "other_pkg" / "loss_utils.py").write_text("def ssim(a, b):\n    return 'unrelated'\n")
    monkeypatch.syspath_prepend(str(tmp_path))
    yield tmp_path
    autovfx_amd.uninstall()
    for name in [n for n in sys.modules if mine(n)]:
        del sys.modules[name]
    sys.modules.update(parked)


def test_install_before_import_patches_loss_utils(fake_tree):
    autovfx_amd.install()
    trainer = importlib.import_module("trainer_like")
    lu = sys.modules["utils.loss_utils"]
    assert lu.ssim.__module__ == "autovfx_amd.ssim" and lu.ssim.fallback is lu.reference_ssim
    assert trainer.ssim is lu.ssim and trainer.metric is lu.ssim
    assert lu.reference_ssim(None, None) == "reference" and trainer.l1_loss(None, None) == "l1"
    assert lu.ssim("not", "tensors") == "reference"          # everything the kernels do not take goes to the original
    other = importlib.import_module("other_pkg.loss_utils")
    assert other.ssim(None, None) == "unrelated" and not hasattr(other, "reference_ssim")
    assert [n for n in hook.patched_modules if n.endswith("loss_utils")] == ["utils.loss_utils"]   # (other tests import renderers)
    autovfx_amd.uninstall()
    assert lu.ssim(None, None) == "reference" and not hasattr(lu, "reference_ssim")
    assert trainer.ssim is lu.ssim and trainer.metric is lu.ssim


def test_install_after_import_rebinds_existing_importers(fake_tree):
    trainer = importlib.import_module("trainer_like")
    original = trainer.ssim
    autovfx_amd.install()
    autovfx_amd.install()   # idempotent
    lu = sys.modules["utils.loss_utils"]
    assert lu.reference_ssim is original and lu.ssim.fallback is original
    assert trainer.ssim is lu.ssim and trainer.metric is lu.ssim and lu.ssim is not original
    autovfx_amd.uninstall()
    assert lu.ssim is original and trainer.ssim is original and trainer.metric is original


def test_lenient_install_leaves_ssim_when_the_library_cannot_load(fake_tree, monkeypatch):
    import builtins
    real_import = builtins.__import__

    def no_kernels(name, globals=None, locals=None, fromlist=(), level=0):
        if name == "ssim" and level == 1 and globals and globals.get("__name__") == "autovfx_amd.hook":
            raise ImportError("no libgsr_hip.so")
        return real_import(name, globals, locals, fromlist, level)

    monkeypatch.setattr(builtins, "__import__", no_kernels)
    autovfx_amd.install()   # strict: the failure surfaces where the module is imported
    with pytest.raises(ImportError):
        importlib.import_module("utils.loss_utils")
    sys.modules.pop("utils.loss_utils", None)
    autovfx_amd.uninstall()
    hook.install(strict=False)
    lu = importlib.import_module("utils.loss_utils")
    assert lu.ssim(None, None) == "reference" and "utils.loss_utils" not in hook.patched_modules


@mounted
def test_install_patches_the_real_reference_loss_utils():
    """The reference's own ``utils/loss_utils.py`` and its SuGaR copy, imported unchanged from where they lie in a fresh
    interpreter after ``install()``: ``ssim`` is the drop-in, the original is kept with the same signature."""
    code = textwrap.dedent(f"""
        import inspect, sys
        sys.path[:0] = [{os.path.join(REF, 'gaussian_splatting')!r}, {REF!r}]
        import autovfx_amd
        autovfx_amd.install()
        from utils import loss_utils as a
        from sugar_utils import loss_utils as b
        from utils.loss_utils import ssim
        for m in (a, b):
            print(m.ssim.__module__, m.reference_ssim.__module__, m.ssim.fallback is m.reference_ssim,
                  inspect.signature(m.ssim) == inspect.signature(m.reference_ssim))
        print(ssim is a.ssim)
    """)
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300, cwd="/tmp")
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.split() == ["autovfx_amd.ssim", "utils.loss_utils", "True", "True",
                                "autovfx_amd.ssim", "sugar_utils.loss_utils", "True", "True", "True"], r.stdout


def test_cabi_refusals_need_no_device():
    from autovfx_amd import _lib
    L, win = _lib.lib, S.WINDOW11
    ok = (4096, 4096, win, 0, 4096, None, 4096, 1 << 20, None)
    assert L.gsr_ssim_scratch_bytes(1, 3, 10, 10) == 4 * 3
    assert L.gsr_ssim_scratch_bytes(2, 3, 1080, 1920) == 4 * 2 * 3 * 60 * 68   # one float per 32 x 16 tile
    for dims in ((0, 3, 10, 10), (1, 0, 10, 10), (1, 3, -1, 10), (1, 3, 10, 0), (1 << 16, 1 << 15, 1, 1), (1, 1, 1 << 16, 1 << 15)):
        assert L.gsr_ssim_scratch_bytes(*dims) == 0
        assert L.gsr_ssim_forward(*dims, *ok) == -1 and "bad size" in _lib.last_error()
        assert L.gsr_ssim_backward(*dims, 4096, 4096, 4096, win, 0, 4096, 4096, None) == -1 and "bad size" in _lib.last_error()
    assert L.gsr_ssim_forward(1, 3, 10, 10, 4096, 4096, None, 0, 4096, None, 4096, 1 << 20, None) == -1 and "null" in _lib.last_error()
    assert L.gsr_ssim_forward(1, 3, 10, 10, None, 4096, win, 0, 4096, None, 4096, 1 << 20, None) == -1 and "null" in _lib.last_error()
    assert L.gsr_ssim_forward(1, 3, 10, 10, 4096, 4096, win, 0, 4096, None, None, 1 << 20, None) == -1 and "null" in _lib.last_error()
    assert L.gsr_ssim_forward(1, 3, 10, 10, 4098, 4096, win, 0, 4096, None, 4096, 1 << 20, None) == -1 and "aligned" in _lib.last_error()
    assert L.gsr_ssim_forward(1, 3, 10, 10, 4096, 4096, win, 0, 4096, 4097, 4096, 1 << 20, None) == -1 and "aligned" in _lib.last_error()
    assert L.gsr_ssim_forward(1, 3, 10, 10, 4096, 4096, win, 0, 4096, None, 4096, 11, None) == -1 and "scratch" in _lib.last_error()
    assert L.gsr_ssim_backward(1, 3, 10, 10, 4096, 4096, None, win, 0, 4096, 4096, None) == -1 and "null" in _lib.last_error()
    assert L.gsr_ssim_backward(1, 3, 10, 10, 4096, 4096, 4096, None, 0, 4096, 4096, None) == -1 and "null" in _lib.last_error()
    assert L.gsr_ssim_backward(1, 3, 10, 10, 4096, 4096, 4096, win, 0, 4096, 4094, None) == -1 and "aligned" in _lib.last_error()
