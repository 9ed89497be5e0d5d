"""The fused Adam without a GPU: torch.optim.Adam's interface and results on the CPU (every CPU step is torch's own), checkpoints in
both directions, the rules that send a step to torch, the C ABI's refusals, ``install()`` on a miniature tree and on the
reference's own ``scene/gaussian_model.py``."""
from __future__ import annotations

import copy
import importlib
import inspect
import sys
import types

import numpy as np
import pytest
import torch

import autovfx_amd
from autovfx_amd import _lib, hook
from autovfx_amd import optim as O
from shims import reference_env

SHAPES = {"xyz": (40, 3), "f_dc": (40, 1, 3), "f_rest": (40, 15, 3), "opacity": (40, 1), "scaling": (40, 3), "rotation": (40, 4)}
LRS = {"xyz": 1.6e-4, "f_dc": 2.5e-3, "f_rest": 2.5e-3 / 20.0, "opacity": 0.05, "scaling": 5e-3, "rotation": 1e-3}


def groups(device="cpu", seed=0):
    g = torch.Generator().manual_seed(seed)
    return [{"params": [torch.nn.Parameter(torch.randn(SHAPES[k], generator=g).to(device))], "lr": LRS[k], "name": k} for k in SHAPES]


def clone_groups(gs):
    return [{**gr, "params": [torch.nn.Parameter(p.detach().clone()) for p in gr["params"]]} for gr in gs]


def expon_lr(step, lr_init=1.6e-4, lr_final=1.6e-6, max_steps=30):   # the shape of get_expon_lr_func (numpy float64 out)
    t = np.clip(step / max_steps, 0, 1)
    return np.exp(np.log(lr_init) * (1 - t) + np.log(lr_final) * t)


def set_grads(gs, it):
    for i, gr in enumerate(gs):
        for p in gr["params"]:
            gen = torch.Generator().manual_seed(1000 * it + i)
            p.grad = torch.randn(p.shape, generator=gen) * 10.0 ** (-(it % 5))
            if it % 7 == 3 and gr["name"] == "opacity":
                p.grad = None


def test_constructor_and_type_are_torchs():
    assert inspect.signature(O.Adam) == inspect.signature(torch.optim.Adam)
    opt = O.Adam(groups(), lr=0.0, eps=1e-15)
    assert isinstance(opt, torch.optim.Adam)
    assert opt.defaults == torch.optim.Adam(groups(), lr=0.0, eps=1e-15).defaults


def test_cpu_steps_are_torchs_bit_for_bit():
    a = groups()
    b = clone_groups(a)
    ta, ob = torch.optim.Adam(a, lr=0.0, eps=1e-15), O.Adam(b, lr=0.0, eps=1e-15)
    for it in range(40):
        for opt in (ta, ob):
            opt.param_groups[0]["lr"] = expon_lr(it)       # update_learning_rate (gaussian_model.py:179-185)
        set_grads(a, it)
        set_grads(b, it)
        ta.step()
        ob.step()
        for ga, gb in zip(a, b):
            pa, pb = ga["params"][0], gb["params"][0]
            assert torch.equal(pa, pb)
            sa, sb = ta.state.get(pa), ob.state.get(pb)
            assert (sa is None) == (sb is None)
            if sa:
                assert sb["step"].dtype == torch.float32 and sb["step"].device.type == "cpu" and torch.equal(sa["step"], sb["step"])
                assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"])


@pytest.mark.parametrize("first", ["torch", "ours"])
def test_state_dict_round_trips_with_torch(first):
    make = {"torch": torch.optim.Adam, "ours": O.Adam}
    second = "ours" if first == "torch" else "torch"
    a = groups()
    opt_a = make[first](a, lr=0.0, eps=1e-15)
    for it in range(5):
        set_grads(a, it)
        opt_a.step()
    sd = opt_a.state_dict()
    b, c = clone_groups(a), clone_groups(a)
    opt_b, opt_c = make[second](b, lr=0.0, eps=1e-15), make[first](c, lr=0.0, eps=1e-15)
    opt_b.load_state_dict(copy.deepcopy(sd))   # (loading keeps the dict's CPU tensors: two loads of one dict would share them)
    opt_c.load_state_dict(copy.deepcopy(sd))
    assert opt_b.state_dict()["param_groups"] == sd["param_groups"]
    for it in range(5, 12):
        set_grads(b, it)
        set_grads(c, it)
        opt_b.step()
        opt_c.step()
    for gb, gc in zip(b, c):
        assert torch.equal(gb["params"][0], gc["params"][0])
    sb, sc = opt_b.state_dict()["state"], opt_c.state_dict()["state"]
    assert sb.keys() == sc.keys()
    for k in sb:
        assert sb[k]["step"].device.type == "cpu" and sb[k]["step"].dtype == torch.float32
        for key in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(sb[k][key], sc[k][key])


# --- the rules that send a step to torch, on "meta" tensors (real tensor types and layouts, no storage, no GPU) ---

def meta_group(**over):
    p = torch.nn.Parameter(torch.empty(8, 3, device="meta"))
    p.grad = torch.empty(8, 3, device="meta")
    group = {"params": [p], "lr": 1e-3, "betas": (0.9, 0.999), "eps": 1e-15, "weight_decay": 0, "amsgrad": False, "foreach": None,
             "maximize": False, "capturable": False, "differentiable": False, "fused": None, "decoupled_weight_decay": False}
    group.update(over)
    return group


def with_param(make_p, make_g=None):
    p = make_p()
    if make_g is not None:
        p.grad_dtype = None   # (allows a gradient of another dtype)
    p.grad = make_g(p) if make_g else torch.zeros_like(p)
    return meta_group(params=[p])


def takes(*gs, state=None, capturing=False):
    return O.kernel_takes(list(gs), {} if state is None else state, capturing, device_type="meta")


FALLBACKS = {
    "amsgrad": lambda: [meta_group(amsgrad=True)],
    "maximize": lambda: [meta_group(maximize=True)],
    "capturable": lambda: [meta_group(capturable=True)],
    "differentiable": lambda: [meta_group(differentiable=True)],
    "fused": lambda: [meta_group(fused=True)],
    "foreach_false": lambda: [meta_group(foreach=False)],
    "weight_decay": lambda: [meta_group(weight_decay=1e-4)],
    "decoupled_weight_decay": lambda: [meta_group(weight_decay=1e-2, decoupled_weight_decay=True)],
    "tensor_lr": lambda: [meta_group(lr=torch.tensor(1e-3))],
    "beta1_at_most_half": lambda: [meta_group(betas=(0.5, 0.999))],
    "beta1_above_one": lambda: [meta_group(betas=(1.2, 0.999))],   # (param_groups edited after the constructor's checks)
    "tensor_betas": lambda: [meta_group(betas=(torch.tensor(0.9), torch.tensor(0.999)))],
    "float16": lambda: [with_param(lambda: torch.nn.Parameter(torch.empty(8, device="meta", dtype=torch.float16)))],
    "bfloat16": lambda: [with_param(lambda: torch.nn.Parameter(torch.empty(8, device="meta", dtype=torch.bfloat16)))],
    "float64": lambda: [with_param(lambda: torch.nn.Parameter(torch.empty(8, device="meta", dtype=torch.float64)))],
    "complex64": lambda: [with_param(lambda: torch.nn.Parameter(torch.empty(8, device="meta", dtype=torch.complex64)))],
    "cpu_param": lambda: [with_param(lambda: torch.nn.Parameter(torch.empty(8)))],
    "two_devices": lambda: [meta_group(), with_param(lambda: torch.nn.Parameter(torch.empty(8)))],
    "non_contiguous_param": lambda: [with_param(lambda: torch.nn.Parameter(torch.empty(3, 8, device="meta").t()))],
    "non_contiguous_grad": lambda: [with_param(lambda: torch.nn.Parameter(torch.empty(8, 3, device="meta")),
                                               lambda p: torch.empty(3, 8, device="meta").t())],
    "grad_other_dtype": lambda: [with_param(lambda: torch.nn.Parameter(torch.empty(8, device="meta")),
                                            lambda p: torch.empty(8, device="meta", dtype=torch.float16))],
    "param_subclass": lambda: [with_param(lambda: type("MyParam", (torch.nn.Parameter,), {})(torch.empty(8, device="meta")))],
}


def test_plain_groups_take_the_kernel():
    assert takes(meta_group())
    assert takes(meta_group(), meta_group(lr=np.float64(2e-4), betas=(0.6, 0.99), eps=1e-8))   # numpy lr, other betas
    assert takes(meta_group(), with_param(lambda: torch.nn.Parameter(torch.empty(0, device="meta"))))
    nograd = meta_group()
    nograd["params"][0].grad = None
    assert takes(meta_group(), nograd)


@pytest.mark.parametrize("case", sorted(FALLBACKS))
def test_fallback_cases(case):
    assert not takes(*FALLBACKS[case]())


def test_fallback_when_nothing_has_a_gradient_or_the_stream_captures():
    g = meta_group()
    g["params"][0].grad = None
    assert not takes(g)
    assert not takes(meta_group(), capturing=True)


@pytest.mark.parametrize("what", ["step_on_device", "step_float64", "exp_avg_other_shape", "exp_avg_sq_non_contiguous",
                                  "exp_avg_float16"])
def test_fallback_on_state_the_kernel_cannot_take(what):
    g = meta_group()
    p = g["params"][0]
    st = {"step": torch.tensor(3.0), "exp_avg": torch.empty(8, 3, device="meta"), "exp_avg_sq": torch.empty(8, 3, device="meta")}
    assert takes(g, state={p: dict(st)})
    if what == "step_on_device":
        st["step"] = torch.tensor(3.0, device="meta")
    elif what == "step_float64":
        st["step"] = torch.tensor(3.0, dtype=torch.float64)
    elif what == "exp_avg_other_shape":
        st["exp_avg"] = torch.empty(24, device="meta")
    elif what == "exp_avg_sq_non_contiguous":
        st["exp_avg_sq"] = torch.empty(3, 8, device="meta").t()
    else:
        st["exp_avg"] = torch.empty(8, 3, device="meta", dtype=torch.float16)
    assert not takes(g, state={p: st})


def test_cpu_fallback_keeps_torchs_exceptions():
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.zeros(4).to_sparse()
    for cls in (torch.optim.Adam, O.Adam):
        with pytest.raises(RuntimeError, match="sparse"):
            cls([p]).step()


def test_cabi_refusals_need_no_device():
    L = _lib.lib
    T = _lib.AdamTensor
    good = lambda **k: T(**{"param": 4096, "grad": 8192, "exp_avg": 12288, "exp_avg_sq": 16384, "numel": 100, "step_size": -1e-3,
                            "bias2_sqrt": 0.03, **k})
    call = lambda ts, n=None: L.gsr_adam_step((T * max(len(ts), 1))(*ts), len(ts) if n is None else n, 0.1, 0.999, 1e-3, 1e-15, None)
    assert call([good()], 0) == -1 and "count" in _lib.last_error()
    assert call([good()], -1) == -1 and "count" in _lib.last_error()
    assert call([good()] * 17) == -1 and "count" in _lib.last_error()
    assert L.gsr_adam_step(None, 1, 0.1, 0.999, 1e-3, 1e-15, None) == -1 and "null" in _lib.last_error()
    for w in (0.5, 0.7, -0.1, float("nan")):
        assert L.gsr_adam_step((T * 1)(good()), 1, w, 0.999, 1e-3, 1e-15, None) == -1 and "w =" in _lib.last_error()
    assert call([good(numel=-1)]) == -1 and "numel" in _lib.last_error()
    for k in ("param", "grad", "exp_avg", "exp_avg_sq"):
        assert call([good(), good(**{k: None})]) == -1 and "tensor 1: null" in _lib.last_error()
        assert call([good(**{k: 4098})]) == -1 and "aligned" in _lib.last_error()
    assert _lib.ADAM_MAX_TENSORS == 16 and ctypes_size() == 48


def ctypes_size():
    import ctypes
    return ctypes.sizeof(_lib.AdamTensor)


# --- install() ---

MODEL_SRC = """\
import torch


class GaussianModel:
    def __init__(self):
        self._xyz = torch.nn.Parameter(torch.zeros(4, 3))
        self.optimizer = None

    def training_setup(self, training_args):
        self.optimizer = torch.optim.Adam([{'params': [self._xyz], 'lr': 0.01, 'name': 'xyz'}], lr=0.0, eps=1e-15)
        return 'set up'

    def replace_tensor_to_optimizer(self, tensor, name):
        return {}
"""
OTHER_MODEL_SRC = """\
import torch


class GaussianModel:
    def training_setup(self, training_args):
        self.optimizer = torch.optim.Adam([torch.nn.Parameter(torch.zeros(2))])
"""


@pytest.fixture
def fake_model_tree(tmp_path, monkeypatch):
    """scene/gaussian_model.py shaped like the reference's, a trainer that imports it, and a ``gaussian_model`` whose class lacks
    ``replace_tensor_to_optimizer`` (left alone)."""
    mine = lambda n: n.split(".")[0] in ("scene", "trainer_like", "other_pkg")
    parked = {n: sys.modules.pop(n) for n in [n for n in sys.modules if mine(n)]}
    (tmp_path / "scene").mkdir()
    (tmp_path / "scene" / "__init__.py").write_text("")
    (tmp_path / "scene" / "gaussian_model.py").write_text(MODEL_SRC)
    (tmp_path / "trainer_like.py").write_text("from scene.gaussian_model import GaussianModel\n")
    (tmp_path / "other_pkg").mkdir()
    (tmp_path / "other_pkg" / "__init__.py").write_text("")
    (tmp_path / "other_pkg" / "gaussian_model.py").write_text(OTHER_MODEL_SRC)
    monkeypatch.syspath_prepend(str(tmp_path))
    yield tmp_path
    autovfx_amd.uninstall()
    for name in [n for n in sys.modules if mine(n)]:
        del sys.modules[name]
    sys.modules.update(parked)


def test_install_before_import_patches_training_setup(fake_model_tree):
    from autovfx_amd import gaussian_model as ours_gm
    before = dict(vars(ours_gm.GaussianModel))
    autovfx_amd.install()
    trainer = importlib.import_module("trainer_like")
    cls = sys.modules["scene.gaussian_model"].GaussianModel
    assert trainer.GaussianModel is cls and "reference_training_setup" in cls.__dict__
    m = cls()
    assert m.training_setup(None) == "set up"
    assert type(m.optimizer) is O.Adam and m.optimizer.param_groups[0]["name"] == "xyz"
    assert m.optimizer.param_groups[0]["params"][0] is m._xyz and m.optimizer.defaults["eps"] == 1e-15 and not m.optimizer.state
    other = importlib.import_module("other_pkg.gaussian_model").GaussianModel
    assert "reference_training_setup" not in other.__dict__
    o = other()
    o.training_setup(None)
    assert type(o.optimizer) is torch.optim.Adam
    assert dict(vars(ours_gm.GaussianModel)) == before
    assert hook.patched_models == ["scene.gaussian_model"] and not any(n.endswith("gaussian_model") for n in hook.patched_modules)
    autovfx_amd.uninstall()
    assert "reference_training_setup" not in cls.__dict__
    m.training_setup(None)
    assert type(m.optimizer) is torch.optim.Adam


def test_install_after_import_patches_the_class_in_place(fake_model_tree):
    trainer = importlib.import_module("trainer_like")
    original = trainer.GaussianModel.__dict__["training_setup"]
    autovfx_amd.install()
    autovfx_amd.install()   # idempotent
    cls = trainer.GaussianModel
    assert cls.reference_training_setup is original and cls.__dict__["training_setup"] is not original
    m = cls()
    m.training_setup(None)
    assert type(m.optimizer) is O.Adam
    autovfx_amd.uninstall()
    assert cls.__dict__["training_setup"] is original


def test_lenient_install_keeps_torchs_adam_when_the_library_cannot_load(fake_model_tree, monkeypatch):
    import builtins
    real_import = builtins.__import__

    def no_kernels(name, globals=None, locals=None, fromlist=(), level=0):
        if name == "optim" and level == 1 and globals and globals.get("__name__") == "autovfx_amd.hook":
            raise ImportError("no libgsr_hip.so")
        return real_import(name, globals, locals, fromlist, level)

    monkeypatch.setattr(builtins, "__import__", no_kernels)
    autovfx_amd.install()   # strict: the failure surfaces at the first training_setup
    cls = importlib.import_module("scene.gaussian_model").GaussianModel
    with pytest.raises(ImportError):
        cls().training_setup(None)
    autovfx_amd.uninstall()
    sys.modules.pop("scene.gaussian_model", None)
    hook.install(strict=False)
    cls = importlib.import_module("scene.gaussian_model").GaussianModel
    m = cls()
    assert m.training_setup(None) == "set up" and type(m.optimizer) is torch.optim.Adam


# --- the reference's own GaussianModel (CPU, under the shims) ---

def _training_args():
    return types.SimpleNamespace(percent_dense=0.01, position_lr_init=1.6e-4, position_lr_final=1.6e-6, position_lr_delay_mult=0.01,
                                 position_lr_max_steps=30_000, feature_lr=2.5e-3, opacity_lr=0.05, scaling_lr=5e-3, rotation_lr=1e-3)


def _reference_run(gm_module, patched: bool):
    torch.manual_seed(0)
    n = 64
    m = gm_module.GaussianModel(3)
    m._xyz = torch.nn.Parameter(torch.randn(n, 3))
    m._features_dc = torch.nn.Parameter(torch.randn(n, 1, 3))
    m._features_rest = torch.nn.Parameter(torch.randn(n, 15, 3) * 0.1)
    m._scaling = torch.nn.Parameter(torch.randn(n, 3) - 3)
    m._rotation = torch.nn.Parameter(torch.randn(n, 4))
    m._opacity = torch.nn.Parameter(torch.randn(n, 1))
    m.max_radii2D = torch.zeros(n)
    m.spatial_lr_scale = 2.0
    args = _training_args()
    m.training_setup(args)
    assert (type(m.optimizer) is O.Adam) == patched and isinstance(m.optimizer, torch.optim.Adam)

    def train(its, start):
        for it in range(start, start + its):
            m.update_learning_rate(it)
            loss = sum((t * t).sum() for t in (m._xyz, m._features_dc, m._features_rest, m._scaling, m._rotation, m._opacity))
            loss.backward()
            m.optimizer.step()
            m.optimizer.zero_grad(set_to_none=True)

    train(4, 1)
    m.reset_opacity()
    train(2, 5)
    mask = torch.zeros(m._xyz.shape[0], dtype=torch.bool)
    mask[::5] = True
    m.prune_points(mask)
    k = 7
    m.densification_postfix(torch.randn(k, 3), torch.randn(k, 1, 3), torch.zeros(k, 15, 3), torch.randn(k, 1), torch.randn(k, 3),
                            torch.randn(k, 4))
    train(3, 7)
    snap = m.capture()
    m2 = gm_module.GaussianModel(3)
    m2.restore(snap, args)
    assert (type(m2.optimizer) is O.Adam) == patched
    m = m2
    train(2, 10)
    tensors = [t.detach().clone() for t in (m._xyz, m._features_dc, m._features_rest, m._opacity, m._scaling, m._rotation)]
    return tensors, m.optimizer.state_dict()


@pytest.mark.skipif(not reference_env.available(), reason="the reference tree is not mounted")
def test_reference_gaussian_model_trains_the_same_with_this_adam():
    with reference_env.reference_tree():
        gm = importlib.import_module("scene.gaussian_model")
        want, want_sd = _reference_run(gm, patched=False)
        try:
            autovfx_amd.install()
            assert gm.GaussianModel.training_setup._autovfx_amd_wrapped and "scene.gaussian_model" in hook.patched_models
            got, got_sd = _reference_run(gm, patched=True)
        finally:
            autovfx_amd.uninstall()
        assert "reference_training_setup" not in gm.GaussianModel.__dict__
    for a, b in zip(want, got):
        assert torch.equal(a, b)
    assert want_sd["param_groups"] == got_sd["param_groups"] and want_sd["state"].keys() == got_sd["state"].keys()
    for k in want_sd["state"]:
        for key in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(want_sd["state"][k][key], got_sd["state"][k][key])
