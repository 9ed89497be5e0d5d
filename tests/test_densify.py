"""The HIP densification without a GPU: ``plan_host`` and the Python surgery against the reference's own ``GaussianModel`` (where
its tree is mounted) and against recorded runs of it (tests/golden/densify/ref_*.npz, always), the restated method of the GPU tests
against the host path on non-finite rows and on rows of chosen classes (with the non-finite rules spelled out on ``plan_host``'s
masks), the hook rows, ``kernel_takes`` rule by rule, the C ABI's refusals."""
from __future__ import annotations

import glob
import importlib
import os
import sys
import types

import numpy as np
import pytest
import torch

import autovfx_amd
from autovfx_amd import _lib, hook
from autovfx_amd import densify as D
from autovfx_amd import optim as O
from shims import reference_env

import densify_cases as C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "densify", "ref_*.npz")))   # a directory of their own: tests/golden/*.npz are the rasterizer's vectors
THR, MIN_OP = 0.0002, 0.005


# --- recorded runs of the reference ---

def model_from_fixture(z, device="cpu", opt_cls=torch.optim.Adam):
    m = C.Model({k: torch.from_numpy(z["in." + k]).to(device) for k in C.ATTRS}, opt_cls)
    m.percent_dense = float(z["percent_dense"])
    for k in ("accum", "denom", "max_radii2D"):
        setattr(m, {"accum": "xyz_gradient_accum"}.get(k, k), torch.from_numpy(z["in." + k]).to(device))
    if "in.xyz.step" in z.files:
        for group in m.optimizer.param_groups:
            name = group["name"]
            m.optimizer.state[group["params"][0]] = {"step": torch.from_numpy(z[f"in.{name}.step"]).clone(),
                                                     "exp_avg": torch.from_numpy(z[f"in.{name}.exp_avg"]).to(device),
                                                     "exp_avg_sq": torch.from_numpy(z[f"in.{name}.exp_avg_sq"]).to(device)}
    return m


def fixture_call(z):
    mss = float(z["max_screen_size"])
    return float(z["max_grad"]), float(z["min_opacity"]), float(z["extent"]), None if mss < 0 else mss


def inject_samples(monkeypatch, z, device="cpu"):
    samples = torch.from_numpy(z["samples"]).to(device)

    def normal(mean, std):
        assert mean.shape == std.shape == samples.shape
        return samples

    monkeypatch.setattr(torch, "normal", normal)


def test_fixtures_are_there():
    assert len(FIXTURES) >= 3 and all(os.path.getsize(f) < 1 << 20 for f in FIXTURES)


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(f) for f in FIXTURES])
def test_recorded_reference_runs_replay_bit_for_bit(path, monkeypatch):
    z = np.load(path)
    m = model_from_fixture(z)
    assert D.kernel_takes(m, *fixture_call(z), device_type="cpu")
    inject_samples(monkeypatch, z)
    D.densify_and_prune_host(m, *fixture_call(z))
    got = C.snapshot(m)
    want = {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("out.")}
    C.assert_same(want, got)
    assert not got["max_radii2D"].any() and got["xyz"].shape[0] > z["in.xyz"].shape[0]


# --- the reference's own methods ---

def _reference_model(gm, n, seed, steps):
    m = gm.GaussianModel(3)
    for name, t in C.random_tensors(n, 3, seed).items():
        setattr(m, C.ATTRS[name], torch.nn.Parameter(t))
    m.spatial_lr_scale = 1.0
    m.training_setup(types.SimpleNamespace(percent_dense=0.01, position_lr_init=1.6e-4, position_lr_final=1.6e-6, position_lr_delay_mult=0.01,
                                           position_lr_max_steps=30_000, feature_lr=2.5e-3, opacity_lr=0.05, scaling_lr=5e-3, rotation_lr=1e-3))
    C.train_steps(m, steps)
    C.fill_stats(m, seed + 7)
    return m


def _shape(m, case):
    """Edit the statistics / parameters of ``m`` in place for one named case."""
    bound = 0.01 * 5.0
    with torch.no_grad():
        if case == "no_clones":
            m._scaling += 3.0                                            # everything above the dense bound
        elif case == "no_splits":
            m._scaling -= 3.0
        elif case == "on_threshold":
            m.denom[:] = 1.0
            m.xyz_gradient_accum[:] = torch.tensor(THR, dtype=torch.float32)   # g == fl(thr) exactly: `>=` holds for clones and splits
            m._scaling[::3, 0] = torch.log(torch.tensor(bound, dtype=torch.float32))   # big as close to the dense bound as exp gets
        elif case == "big_radii":
            m.max_radii2D[:] = 1e6


CASES = [("plain", 4096, 3, None), ("plain", 4096, 3, 20), ("no_clones", 300, 2, 20), ("no_splits", 300, 2, None), ("on_threshold", 300, 1, 20),
         ("big_radii", 300, 1, 20), ("plain", 300, 0, 20), ("plain", 2, 1, 20)]


@pytest.mark.skipif(not reference_env.available(), reason="the reference tree is not mounted")
@pytest.mark.parametrize("case, n, steps, mss", CASES, ids=[f"{c}-{n}-{s}-{m}" for c, n, s, m in CASES])
def test_host_restatement_equals_the_references_own_method(case, n, steps, mss):
    with reference_env.reference_tree():
        gm = importlib.import_module("scene.gaussian_model")
        results = []
        for which in ("reference", "host"):
            m = _reference_model(gm, n, 5, steps)
            _shape(m, case)
            if which == "host":                                            # two stats calls through both routes too
                assert D.kernel_takes(m, THR, MIN_OP, 5.0, mss, device_type="cpu")
            torch.manual_seed(3)
            with torch.no_grad():
                (m.densify_and_prune if which == "reference" else lambda *a: D.densify_and_prune_host(m, *a))(THR, MIN_OP, 5.0, mss)
            results.append((C.snapshot(m), torch.get_rng_state()))
    (want, rng_w), (got, rng_g) = results
    C.assert_same(want, got)
    assert torch.equal(rng_w, rng_g) and not got["max_radii2D"].any()
    if case == "plain" and n == 4096:
        assert got["xyz"].shape[0] > n
    if case == "big_radii":
        assert got["xyz"].shape[0] >= n * 0.9                              # the screen-size test never fires inside the method


@pytest.mark.skipif(not reference_env.available(), reason="the reference tree is not mounted")
def test_installed_on_a_cpu_model_the_references_methods_run():
    with reference_env.reference_tree():
        gm = importlib.import_module("scene.gaussian_model")
        out = []
        for patched in (False, True):
            if patched:
                autovfx_amd.install()
            try:
                assert ("reference_densify_and_prune" in gm.GaussianModel.__dict__) == patched
                m = _reference_model(gm, 200, 9, 1)
                vp = torch.zeros(200, 3, requires_grad=True)
                vp.grad = torch.randn(200, 3, generator=torch.Generator().manual_seed(1))
                m.add_densification_stats(vp, torch.arange(200) % 3 == 0)
                torch.manual_seed(3)
                with torch.no_grad():
                    m.densify_and_prune(THR, MIN_OP, 5.0, 20)
                out.append(C.snapshot(m))
            finally:
                autovfx_amd.uninstall()
        assert "reference_densify_and_prune" not in gm.GaussianModel.__dict__
    C.assert_same(*out)


def test_restated_model_of_the_tests_equals_the_host_path():
    """The reference-shaped restatement the GPU tests use as their truth (densify_cases.Model) against plan_host, on the CPU."""
    for n, steps, mss in ((500, 2, 20), (500, 0, None), (3, 1, 20)):
        base = C.Model(C.random_tensors(n, 3, n))
        C.train_steps(base, steps)
        C.fill_stats(base)
        a, b = C.twin(base), C.twin(base)
        torch.manual_seed(1)
        a.reference_densify_and_prune(THR, MIN_OP, 5.0, mss)
        rng = torch.get_rng_state()
        torch.manual_seed(1)
        D.densify_and_prune_host(b, THR, MIN_OP, 5.0, mss)
        C.assert_same(C.snapshot(a), C.snapshot(b))
        assert torch.equal(rng, torch.get_rng_state())


# --- non-finite rows and runs of one class: the truth of the GPU tests holds on them ---

def both_on_the_cpu(base, mss, extent=5.0):
    a, b = C.twin(base), C.twin(base)
    torch.manual_seed(1)
    a.reference_densify_and_prune(THR, MIN_OP, extent, mss)
    rng = torch.get_rng_state()
    torch.manual_seed(1)
    assert D.kernel_takes(b, THR, MIN_OP, extent, mss, device_type="cpu")
    D.densify_and_prune_host(b, THR, MIN_OP, extent, mss)
    got = C.snapshot(b)
    C.assert_same(C.snapshot(a), got)
    assert torch.equal(rng, torch.get_rng_state())
    return got


@pytest.mark.parametrize("n, degree, steps", [(128, 3, 1), (3000, 3, 1), (5000, 0, 0)])
def test_non_finite_rows_restated_method_equals_the_host_path(n, degree, steps):
    base, _ = C.non_finite_model(n, degree, steps)
    for mss, extent in ((None, 5.0), (20, 5.0), (20, 100.0)):             # extent 100: the clone bound is exp(0)
        got = both_on_the_cpu(base, mss, extent)
        assert any(bool(v.isnan().any()) for v in got.values()) and got["xyz"].shape[0] != n


@pytest.mark.parametrize("n", [3000, 5000])
def test_non_finite_rows_are_classified_by_the_rules(n):
    """What gaussian_model.py:399-411 does with a NaN or an infinity, said once more, row kind by row kind, about plan_host's masks."""
    m, rows = C.non_finite_model(n, 0, 0)
    injected = torch.cat(list(rows.values()))
    assert injected.unique().numel() == injected.numel() and {0, 63, 64, 1023, 1024} <= set(injected.tolist())
    scaling, opacity = m._scaling.detach(), m._opacity.detach()
    big = torch.exp(scaling).max(dim=1).values
    small, large = big <= 0.05, big > 0.05
    dim = (torch.sigmoid(opacity) < MIN_OP).reshape(-1)
    hot = (m.xyz_gradient_accum >= THR).reshape(-1)
    for ws in (None, 0.5):
        plan = D.plan_host(m.xyz_gradient_accum, m.denom, scaling, opacity, THR, 0.05, MIN_OP, ws)
        keep, clone, split = plan["keep"], plan["clone"], plan["split"]
        wide = big > ws if ws else torch.zeros(n, dtype=torch.bool)
        at = lambda *kinds: torch.cat([rows[k] for k in kinds])
        # any NaN in a scale: the largest scale is NaN, every comparison with it is false
        r = at("scaling.nan.0", "scaling.nan.1", "scaling.nan.2", "scaling.nan0.+inf2")
        assert hot[r].any() and not hot[r].all() and scaling[r].isnan().any(dim=1).all()
        assert not clone[r].any() and not split[r].any() and torch.equal(keep[r], ~dim[r]) and not dim[r].all()
        # g = NaN is g = 0
        r = at("accum.nan", "denom.0.accum0", "denom.nan", "denom.+inf.accum+inf")
        assert (m.xyz_gradient_accum[r] / m.denom[r]).isnan().all() and not clone[r].any() and not split[r].any()
        assert torch.equal(keep[r], ~dim[r] & ~wide[r])
        # a negative gradient: its norm clones a small row, the gradient itself splits nothing
        r = at("accum.negative", "accum.-inf")
        assert small[r].any() and large[r].any() and not split[r].any()
        assert torch.equal(clone[r], small[r] & ~dim[r]) and clone[r].any() and torch.equal(keep[r], ~dim[r] & ~wide[r])
        # an infinite gradient is hot
        r = at("accum.+inf", "denom.0.accum+")
        assert torch.equal(split[r], large[r]) and torch.equal(clone[r], small[r] & ~dim[r]) and split[r].any() and clone[r].any()
        # an infinite scale is large, a zero scale (exp(-inf)) leaves the other two to decide
        r = at("scaling.+inf.0", "scaling.+inf.1", "scaling.+inf.2")
        assert torch.equal(split[r], hot[r]) and not clone[r].any() and torch.equal(keep[r], ~hot[r] & ~dim[r] & ~wide[r])
        assert wide[r].all() if ws else not wide[r].any()
        r = at("scaling.-inf.0", "scaling.-inf.1", "scaling.-inf.2")
        assert torch.equal(split[r], hot[r] & large[r]) and torch.equal(clone[r], hot[r] & small[r] & ~dim[r]) and split[r].any()
        # sigmoid(NaN) < min_opacity is false; sigmoid(-inf) = 0, sigmoid(+inf) = 1
        r = at("opacity.nan", "opacity.+inf")
        assert not dim[r].any() and (keep[r] | split[r] | wide[r]).all()
        r = rows["opacity.-inf"]
        assert dim[r].all() and not keep[r].any() and not clone[r].any() and torch.equal(split[r], hot[r] & large[r])
        for mask in (keep, clone, split, ~keep & ~split):
            assert mask[injected].any()
    # exp(0) on the clone bound (percent_dense * extent = 1): `<=` clones, nothing splits
    r = rows["scaling.exp0"]
    plan = D.plan_host(m.xyz_gradient_accum, m.denom, scaling, opacity, THR, 0.01 * 100.0, MIN_OP, 0.1 * 100.0)
    assert bool((big[r] == 1.0).all()) and torch.equal(plan["clone"][r], hot[r] & ~dim[r]) and plan["clone"][r].any() and not plan["split"][r].any()


LAYOUT_N = 4096 + 37
LAYOUTS = ([(name, 3 if name == "mod7" else 0, LAYOUT_N) for name in C.run_layouts(8)]
           + [(f"seam{k}", degree, 0) for k in (1047, 1048, 1049) for degree in (2, 1)] + [("only_children", 2, 0), ("no_child", 1, 0), ("scanA", 0, 262_145 + 1024)])


def layout(name, n):
    """The class list of a named layout (the GPU tests build theirs here too)."""
    if name.startswith("seam"):
        return C.seam_layout(int(name[4:]), seed=int(name[4:]))
    if name in ("only_children", "no_child"):
        return torch.full((300,), C.SPLIT if name == "only_children" else C.SPLIT_PRUNED)
    if name.startswith("scan"):
        return C.scan_layouts(n)[name[4:]]
    return C.run_layouts(n)[name]


@pytest.mark.parametrize("name, degree, n", LAYOUTS, ids=[f"{name}-d{d}" for name, d, _ in LAYOUTS])
def test_rows_of_chosen_classes_restated_method_equals_the_host_path(name, degree, n):
    cls = layout(name, n)
    base = C.rows_of_classes(cls, degree, seed=3, steps=1 if degree else 0)   # asserts plan_host's three masks are these classes
    for mss in (None, 20):
        got = both_on_the_cpu(base, mss)
        assert got["xyz"].shape[0] == C.rows_left(cls, mss)
    if name.startswith("seam"):
        assert got["xyz"].shape[0] == int(name[4:]) + 1000


# --- the hook rows ---

NEEDS = ("densification_postfix", "prune_points", "cat_tensors_to_optimizer")


@pytest.mark.parametrize("attr", ["add_densification_stats", "densify_and_prune"])
@pytest.mark.parametrize("complete", [True, False])
def test_hook_rows(attr, complete, monkeypatch):
    original = lambda self, *a: "reference"
    module = types.ModuleType("hook_rows_densify.gaussian_model")
    owner = type("GaussianModel", (), {})
    module.GaussianModel = owner
    for name in NEEDS[:3 if complete else 2]:
        setattr(owner, name, lambda *a, **k: None)
    setattr(owner, attr, original)
    monkeypatch.setitem(sys.modules, module.__name__, module)
    try:
        autovfx_amd.install(path=False)
        if not complete:
            assert vars(owner)[attr] is original and module.__name__ not in hook.patched_models
            return
        assert vars(owner)[attr] is not original and vars(owner)["reference_" + attr] is original
        assert hook.patched_models.count(module.__name__) == 1
        before = dict(vars(owner))
        autovfx_amd.install(path=False)
        assert dict(vars(owner)) == before and hook.patched_models.count(module.__name__) == 1
        assert getattr(owner(), attr)(*([None] * (2 if attr == "add_densification_stats" else 4))) == "reference"   # nothing the kernels take
    finally:
        autovfx_amd.uninstall()
    assert vars(owner)[attr] is original and "reference_" + attr not in vars(owner)


# --- kernel_takes ---

def meta_model(n=100, k=15, state=True):
    m = C.Model({name: torch.empty((n,) + (D._TAIL.get(name) or (k, 3)), device="meta") for name in C.ATTRS})
    if state:
        for g in m.optimizer.param_groups:
            p = g["params"][0]
            m.optimizer.state[p] = {"step": torch.tensor(1.0), "exp_avg": torch.empty_like(p), "exp_avg_sq": torch.empty_like(p)}
    return m


def test_kernel_takes_rule_by_rule():
    takes = lambda m, a=(THR, MIN_OP, 5.0, 20), **k: D.kernel_takes(m, *a, device_type="meta", **k)
    assert takes(meta_model()) and takes(meta_model(state=False)) and takes(meta_model(k=0)) and takes(meta_model(), (THR, MIN_OP, 5.0, None))
    assert takes(meta_model(), (np.float64(THR), MIN_OP, np.float64(5.0), 0))
    assert not takes(meta_model(), capturing=True)
    assert not D.kernel_takes(meta_model(), THR, MIN_OP, 5.0, 20)                       # not on a GPU
    for call in ((0.0, MIN_OP, 5.0, 20), (-1.0, MIN_OP, 5.0, 20), (float("nan"), MIN_OP, 5.0, 20), (THR, MIN_OP, float("inf"), 20),
                 (THR, MIN_OP, 5.0, -3), (THR, torch.tensor(MIN_OP), 5.0, 20), (THR, MIN_OP, np.float32(5.0), 20), (THR, MIN_OP, 1e41, 20)):
        assert not takes(meta_model(), call), call
    assert not takes(meta_model(n=1)) and not takes(meta_model(n=0))
    m = meta_model()
    m.optimizer.param_groups[0]["name"] = "other"
    assert not takes(m)
    m = meta_model()
    m.optimizer.param_groups[1]["params"].append(torch.nn.Parameter(torch.empty(1, device="meta")))
    assert not takes(m)
    m = meta_model()
    m._rotation = torch.nn.Parameter(torch.empty(100, 4, device="meta"))                # not the optimizer's
    assert not takes(m)
    for attr, bad in (("_xyz", torch.empty(100, 3, device="meta", dtype=torch.float64)), ("_opacity", torch.empty(100, device="meta")),
                      ("_scaling", torch.empty(100, 6, device="meta")[:, ::2]), ("_features_rest", torch.empty(100, 15, 4, device="meta"))):
        m = meta_model(state=False)
        p = torch.nn.Parameter(bad)
        setattr(m, attr, p)
        next(g for g in m.optimizer.param_groups if C.ATTRS[g["name"]] == attr)["params"][0] = p
        assert not takes(m), attr
    m = meta_model()
    m.optimizer.state[m._xyz]["exp_avg"] = torch.empty(99, 3, device="meta")
    assert not takes(m)
    m = meta_model()
    m.optimizer.state[m._opacity] = {}
    assert not takes(m)
    for stat, bad in (("denom", torch.empty(100, device="meta")), ("xyz_gradient_accum", torch.empty(100, 1, device="meta", dtype=torch.float16))):
        m = meta_model()
        setattr(m, stat, bad)
        assert not takes(m), stat
    m = meta_model()
    del m.optimizer
    assert not takes(m)


def test_stats_kernel_takes_rule_by_rule():
    def args(n=100, cols=3, **k):
        vp = types.SimpleNamespace(grad=k.get("grad", torch.empty(n, cols, device="meta")))
        return meta_model(n), vp, k.get("filter", torch.empty(n, dtype=torch.bool, device="meta"))

    takes = lambda a, **k: D.stats_kernel_takes(*a, device_type="meta", **k)
    assert takes(args()) and takes(args(cols=2)) and takes(args(cols=4))
    assert not takes(args(), capturing=True) and not D.stats_kernel_takes(*args())
    assert not takes(args(cols=1)) and not takes(args(grad=None)) and not takes(args(grad=torch.empty(100, 6, device="meta")[:, ::2]))
    assert not takes(args(filter=torch.empty(100, dtype=torch.uint8, device="meta"))) and not takes(args(filter=torch.empty(99, dtype=torch.bool, device="meta")))
    assert not takes(args(filter=torch.empty(100, dtype=torch.bool)))
    m, vp, f = args()
    m.denom = torch.empty(100, device="meta")
    assert not takes((m, vp, f))


def test_a_call_nothing_takes_needs_the_reference_method():
    m = C.Model(C.random_tensors(4))
    del type(m).reference_densify_and_prune
    try:
        with pytest.raises(RuntimeError, match="reference_densify_and_prune"):
            D.densify_and_prune(m, THR, MIN_OP, 5.0, 20)
    finally:
        importlib.reload(C)


# --- the C ABI's refusals (no launch, no device) ---

def test_cabi_refusals_need_no_device():
    L, err = _lib.lib, _lib.last_error
    A = 4096
    assert L.gsr_densify_stats(0, None, 3, None, None, None, None, None, None) == 0
    assert L.gsr_densify_stats(-1, A, 3, A, A, A, None, None, None) == -1 and "n =" in err()
    assert L.gsr_densify_stats(1 << 31, A, 3, A, A, A, None, None, None) == -1 and "n =" in err()
    assert L.gsr_densify_stats(8, A, 1, A, A, A, None, None, None) == -1 and "grad_row_floats" in err()
    for k in range(4):
        ptrs = [A, A, A, A]
        ptrs[k] = None
        assert L.gsr_densify_stats(8, ptrs[0], 3, ptrs[1], ptrs[2], ptrs[3], None, None, None) == -1 and "null" in err()
    assert L.gsr_densify_stats(8, A, 3, A, A, A, A, None, None) == -1 and "null" in err()
    assert L.gsr_densify_stats(8, A + 2, 3, A, A, A, None, None, None) == -1 and "aligned" in err()
    assert L.gsr_densify_stats(8, A, 3, A, A, A, A + 1, A, None) == -1 and "aligned" in err()

    assert L.gsr_densify_plan_scratch_bytes(0) == 0 and L.gsr_densify_plan_scratch_bytes(-5) == 0 and L.gsr_densify_plan_scratch_bytes(1 << 31) == 0
    need = L.gsr_densify_plan_scratch_bytes(3_000_000)
    assert 3_000_000 <= need < 3_200_000 and need % 256 == 0
    plan = lambda n=100, ptrs=(A,) * 8, room=1 << 20: L.gsr_densify_plan(n, *ptrs[:4], THR, 0.05, MIN_OP, 1, 0.5, *ptrs[4:7], ptrs[7], room, None)
    assert plan(0, (None,) * 8) == 0
    assert plan(-1) == -1 and "n =" in err() and plan(1 << 31) == -1 and "n =" in err()
    for k in range(8):
        ptrs = [A] * 8
        ptrs[k] = None
        assert plan(ptrs=ptrs) == -1 and "null" in err()
        ptrs[k] = A + (2 if k < 7 else 128)
        assert plan(ptrs=ptrs) == -1 and "aligned" in err()
    assert plan(room=L.gsr_densify_plan_scratch_bytes(100) - 1) == -1 and "scratch" in err()

    T, P = _lib.DensifyTensor, _lib.DensifyPlan
    good_t = lambda **k: T(**{"src": A, "dst": A, "side": None, "floats_per_row": 3, "is_moment": 0, **k})
    good_p = lambda **k: P(**{"n_src": 100, "n_keep": 80, "n_front": 90, "n_out": 110, "n_split": 10, "src_of": A, "child_rows": A, "split_idx": A, **k})
    import ctypes
    call = lambda ts, p, n=None: L.gsr_densify_apply((T * max(len(ts), 1))(*ts), len(ts) if n is None else n, ctypes.byref(p), None)
    assert call([good_t()], good_p(), 0) == -1 and "count" in err()
    assert call([good_t()] * 19, good_p()) == -1 and "count" in err()
    assert L.gsr_densify_apply(None, 1, ctypes.byref(good_p()), None) == -1 and "null" in err()
    assert L.gsr_densify_apply((T * 1)(good_t()), 1, None, None) == -1 and "null" in err()
    for bad in (dict(n_src=-1), dict(n_keep=91), dict(n_front=111), dict(n_out=1 << 31), dict(n_out=111), dict(n_split=101), dict(n_src=1 << 31)):
        assert call([good_t()], good_p(**bad)) == -1 and "sizes" in err(), bad
    assert call([good_t()], good_p(n_keep=0, n_front=0, n_out=0, n_split=0)) == 0
    for k in ("src_of", "child_rows", "split_idx"):
        assert call([good_t()], good_p(**{k: None})) == -1 and "null" in err()
        assert call([good_t()], good_p(**{k: A + 2})) == -1 and "aligned" in err()
    assert call([good_t(dst=None)], good_p()) == -1 and "tensor 0: null" in err()
    assert call([good_t(), good_t(src=None)], good_p()) == -1 and "tensor 1: null" in err()
    assert call([good_t(floats_per_row=-1)], good_p()) == -1 and "floats_per_row" in err()
    for k in ("src", "dst", "side"):
        assert call([good_t(**{k: A + 1})], good_p()) == -1 and "aligned" in err()
    assert _lib.DENSIFY_MAX_TENSORS == 18 and ctypes.sizeof(T) == 32 and ctypes.sizeof(P) == 64
