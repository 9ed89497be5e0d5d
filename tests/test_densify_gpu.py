"""The densification kernels on the GPU against the reference-shaped method restated with torch ops on the same device
(tests/densify_cases.py), against torch's two lines for the statistics, and against the recorded runs of the reference."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from autovfx_amd import _lib
from autovfx_amd import densify as D
from autovfx_amd import optim as O

import densify_cases as C
from test_densify import FIXTURES, fixture_call, inject_samples, layout, model_from_fixture

pytestmark = pytest.mark.gpu
DEV = "cuda"
THR, MIN_OP, EXTENT = 0.0002, 0.005, 5.0


def run_both(base, mss, thr=THR, extent=EXTENT):
    a, b = C.twin(base), C.twin(base)
    torch.manual_seed(1)
    a.reference_densify_and_prune(thr, MIN_OP, extent, mss)
    rng = torch.cuda.get_rng_state()
    torch.manual_seed(1)
    assert D.kernel_takes(b, thr, MIN_OP, extent, mss) == (base._xyz.shape[0] >= 2)
    D.densify_and_prune(b, thr, MIN_OP, extent, mss)
    assert torch.equal(rng, torch.cuda.get_rng_state())
    want, got = C.snapshot(a), C.snapshot(b)
    C.assert_same(want, got)
    return got


SIZES = [(1, 3, 1), (63, 3, 2), (64, 3, 0), (65, 3, 1), (4097, 3, 2), (4097, 0, 1), (1_000_000, 3, 1), (3_000_000, 3, 1)]


@pytest.mark.parametrize("opt_cls", [torch.optim.Adam, O.Adam], ids=["torch_adam", "gsr_adam"])
@pytest.mark.parametrize("n, degree, steps", SIZES, ids=[f"{n}-d{d}-s{s}" for n, d, s in SIZES])
def test_equals_the_restated_method_bit_for_bit(n, degree, steps, opt_cls):
    if n >= 1_000_000 and opt_cls is O.Adam and n > 1_000_000:
        steps = 0                                                   # 3 M once with moments (torch's Adam), once without
    base = C.Model(C.random_tensors(n, degree, n % 1000, DEV), opt_cls)
    C.train_steps(base, steps)
    C.fill_stats(base, seed=n % 77)
    for mss in ((None, 20) if n <= 4097 else (20,)):
        got = run_both(base, mss)
        if n >= 63:
            assert got["xyz"].shape[0] != n and not got["max_radii2D"].any()


def test_values_on_the_bounds_and_large_radii():
    base = C.Model(C.random_tensors(5000, 3, 3, DEV))
    C.train_steps(base, 1)
    C.fill_stats(base)
    with torch.no_grad():
        base.denom[:] = 1.0
        base.xyz_gradient_accum[:2500] = torch.tensor(THR, dtype=torch.float32)      # exactly fl(thr)
        base.xyz_gradient_accum[2500:] = torch.nextafter(torch.tensor(THR, dtype=torch.float32), torch.tensor(0.0))
        bound = torch.tensor(0.01 * EXTENT, dtype=torch.float32)
        for k, b in enumerate((bound, torch.nextafter(bound, torch.tensor(1.0)), torch.nextafter(bound, torch.tensor(0.0)))):
            base._scaling[k::7, 0] = torch.log(b)
        base._opacity[::11] = torch.log(torch.tensor(MIN_OP / (1 - MIN_OP), dtype=torch.float32))
        base._scaling[5::13, 1] = torch.log(torch.tensor(0.1 * EXTENT, dtype=torch.float32))
        base.max_radii2D[:] = 1e6                                                      # zeroed before it is read: nobody is pruned for it
    for mss in (None, 20):
        got = run_both(base, mss)
        assert got["xyz"].shape[0] > 2500


def test_no_clones_no_splits_nothing_left():
    for shift, op in ((3.0, 0.0), (-3.0, 0.0), (0.0, -30.0)):
        base = C.Model(C.random_tensors(3000, 3, 4, DEV))
        C.fill_stats(base)
        with torch.no_grad():
            base._scaling += shift
            base._opacity += op
        got = run_both(base, 20)
        if op:
            assert got["xyz"].shape[0] == 0


@pytest.mark.parametrize("path", FIXTURES, ids=[p.split("_")[-1] for p in FIXTURES])
def test_recorded_reference_runs_on_the_gpu(path, monkeypatch):
    """Rows, order and every copied field bit-equal to the reference's CPU run; the two computed fields (children's xyz, scaling)
    cross from glibc's exp / log to the device's: both are compared with an fp64 evaluation, and the drop-in's largest error may be
    at most twice the fixture's own plus one ulp of the value, wherever the truth is finite; where it is not (ref_d: a scale of
    exp(-inf) = 0 has the children's log(0 / 1.6) = -inf), the fixture and the drop-in hold the same NaN or the same infinity."""
    z = np.load(path)
    host = model_from_fixture(z)
    inject_samples(monkeypatch, z)
    plan = D.plan_host(host.xyz_gradient_accum, host.denom, host._scaling.detach(), host._opacity.detach(), **D._bounds(host, *fixture_call(z)))
    sidx = plan["split_idx"].long()
    with torch.no_grad():
        child_rows = D._children(host, sidx, D._bounds(host, *fixture_call(z)))[2]   # the children the reference's last prune kept
    m = model_from_fixture(z, DEV)
    inject_samples(monkeypatch, z, DEV)
    assert D.kernel_takes(m, *fixture_call(z))
    D.densify_and_prune(m, *fixture_call(z))
    got = {k: v.cpu() for k, v in C.snapshot(m).items()}
    want = {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("out.")}
    assert want.keys() == got.keys()
    n_children = child_rows.numel()
    assert 2 * sidx.numel() == z["samples"].shape[0] and n_children > 0
    for key in want:
        assert want[key].shape == got[key].shape, key
        if key in ("xyz", "scaling"):
            front = want[key].shape[0] - n_children
            C.assert_same_tensor(want[key][:front], got[key][:front], key)
        else:
            C.assert_same_tensor(want[key], got[key], key)
    # fp64 truth of the children from the fixture's inputs and samples
    src = {k: torch.from_numpy(z["in." + k]).double() for k in ("xyz", "scaling", "rotation", "accum", "denom")}
    rots = D._build_rotation(src["rotation"][sidx]).repeat(2, 1, 1)
    truth = {"xyz": torch.bmm(rots, torch.from_numpy(z["samples"]).double().unsqueeze(-1)).squeeze(-1) + src["xyz"][sidx].repeat(2, 1),
             "scaling": torch.log(torch.exp(src["scaling"][sidx]).repeat(2, 1) / 1.6)}
    truth = {k: v[child_rows] for k, v in truth.items()}
    for key in ("xyz", "scaling"):
        t = truth[key]
        ulp = torch.abs(torch.nextafter(t.float(), torch.full_like(t.float(), float("inf"))) - t.float()).double()
        finite = t.isfinite()
        for name, kids in (("fixture", want[key][-n_children:].double()), ("drop-in", got[key][-n_children:].double())):
            assert torch.equal(kids.isnan(), t.isnan()) and torch.equal(kids[~finite & ~t.isnan()], t[~finite & ~t.isnan()]), (key, name)
        err_fixture = (want[key][-n_children:].double() - t).abs()[finite]
        err_ours = (got[key][-n_children:].double() - t).abs()[finite]
        print(f"{path.split('_')[-1]} {key}: largest error fixture {err_fixture.max():.3e} drop-in {err_ours.max():.3e}, {int((~finite).sum())} non-finite")
        assert bool((err_ours <= 2 * err_fixture.max() + ulp[finite]).all()), key
    if path.endswith("ref_d.npz"):
        assert not truth["scaling"].isfinite().all() and got["scaling"].isnan().any() and got["opacity"].isnan().any()


def stats_inputs(n, share, seed=0, cols=3):
    g = torch.Generator().manual_seed(seed)
    grad = torch.randn(n, cols, generator=g) * 1e-3
    f = torch.rand(n, generator=g) < share
    accum, denom = torch.rand(n, 1, generator=g), torch.randint(0, 5, (n, 1), generator=g).float()
    return grad.to(DEV), f.to(DEV), accum.to(DEV), denom.to(DEV)


@pytest.mark.parametrize("n", [1, 3, 4, 63, 64, 65, 4097, 1_000_003])
@pytest.mark.parametrize("share", [0.0, 0.2, 1.0])
def test_stats_equal_torchs_two_lines(n, share):
    for cols in (3, 2, 4):
        grad, f, accum, denom = stats_inputs(n, share, n, cols)
        if n > 8:
            grad[5, 0], grad[6, 1], grad[7, 0] = float("inf"), float("nan"), -float("inf")
            accum[3] = float("nan")
        m = C.Model(C.random_tensors(2, 0, 0, DEV))
        m.xyz_gradient_accum, m.denom = accum.clone(), denom.clone()
        vp = torch.zeros(n, cols, device=DEV, requires_grad=True)
        vp.grad = grad
        want = C.Model(C.random_tensors(2, 0, 0, DEV))
        want.xyz_gradient_accum, want.denom = accum.clone(), denom.clone()
        want.reference_add_densification_stats(vp, f)
        assert D.stats_kernel_takes(m, vp, f)
        versions = (m.xyz_gradient_accum._version, m.denom._version)
        D.add_densification_stats(m, vp, f)
        assert m.xyz_gradient_accum._version > versions[0] and m.denom._version > versions[1]
        C.assert_same({"a": want.xyz_gradient_accum, "d": want.denom}, {"a": m.xyz_gradient_accum, "d": m.denom})


def test_stats_with_radii_misaligned_views_and_no_host_synchronisation():
    n = 100_001
    grad, f, accum, denom = stats_inputs(n + 1, 0.3, 5)
    radii = torch.randint(0, 90, (n + 1,), device=DEV, dtype=torch.int32)
    max_radii = torch.rand(n + 1, device=DEV) * 60
    for off in (0, 1):                                                     # off = 1: every pointer 4-byte aligned only
        g, ff, a, d, r, mr = grad[off:off + n], f[off:off + n], accum[off:off + n].clone(), denom[off:off + n].clone(), radii[off:off + n], max_radii[off:off + n].clone()
        if off:
            a, d, mr = accum.clone()[off:off + n], denom.clone()[off:off + n], max_radii.clone()[off:off + n]
        wa, wd, wm = a.clone(), d.clone(), mr.clone()
        wa[ff] += torch.norm(g[ff, :2], dim=-1, keepdim=True)
        wd[ff] += 1
        wm[ff] = torch.max(wm[ff], r[ff].float())
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            D.accumulate_stats(g, ff, a, d, r, mr)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert torch.equal(wa, a) and torch.equal(wd, d) and torch.equal(wm, mr)


def test_apply_writes_every_element():
    """Outputs pre-filled with 0xFF bytes: the apply kernel leaves no element unwritten (degrees 3 and 0, with and without moments)."""
    real_empty = torch.empty

    def poisoned(*a, **k):
        t = real_empty(*a, **k)
        if t.is_cuda and t.dtype == torch.float32:
            t.view(torch.uint8).fill_(0xFF)
        return t

    for degree, steps in ((3, 1), (0, 0), (1, 1)):
        base = C.Model(C.random_tensors(7777, degree, 8, DEV))
        C.train_steps(base, steps)
        C.fill_stats(base)
        a, b = C.twin(base), C.twin(base)
        torch.manual_seed(2)
        a.reference_densify_and_prune(THR, MIN_OP, EXTENT, 20)
        torch.manual_seed(2)
        torch.empty = poisoned
        try:
            D.densify_and_prune(b, THR, MIN_OP, EXTENT, 20)
        finally:
            torch.empty = real_empty
        C.assert_same(C.snapshot(a), C.snapshot(b))


def plan_kernel_against_plan_host(base, ws, thr=THR, dense=0.01 * EXTENT):
    """One gsr_densify_plan call on the model's tensors: counts, both index lists, and nothing written behind them."""
    n = base._xyz.shape[0]
    want = D.plan_host(base.xyz_gradient_accum, base.denom, base._scaling.detach(), base._opacity.detach(), thr, dense, MIN_OP, ws)
    L = _lib.lib
    room = L.gsr_densify_plan_scratch_bytes(n)
    scratch = torch.empty(room, dtype=torch.uint8, device=DEV)
    src_of = torch.full((2 * n,), -7, dtype=torch.int32, device=DEV)
    split_idx = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    counts = torch.full((4,), -7, dtype=torch.int32, device=DEV)
    rc = L.gsr_densify_plan(n, base.xyz_gradient_accum.data_ptr(), base.denom.data_ptr(), base._scaling.data_ptr(), base._opacity.data_ptr(),
                            O._f32(thr), O._f32(dense), O._f32(MIN_OP), 0 if ws is None else 1, O._f32(ws or 0.0), src_of.data_ptr(),
                            split_idx.data_ptr(), counts.data_ptr(), scratch.data_ptr(), room, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib.last_error()
    k, c, s, z = counts.tolist()
    assert [k, c, s, z] == want["counts"].tolist()
    assert torch.equal(src_of[:k + c].cpu(), want["src_of"].cpu()) and torch.equal(split_idx[:s].cpu(), want["split_idx"].cpu())
    assert bool((src_of[k + c:] == -7).all()) and bool((split_idx[s:] == -7).all())
    return want


def test_plan_kernel_equals_plan_host():
    for n in (2, 1023, 1024, 1025, 262_145 + 77):
        base = C.Model(C.random_tensors(n, 0, n % 50, DEV))
        C.fill_stats(base)
        for ws in (None, 0.1 * EXTENT):
            plan_kernel_against_plan_host(base, ws)


@pytest.mark.parametrize("opt_cls", [torch.optim.Adam, O.Adam], ids=["torch_adam", "gsr_adam"])
def test_thirty_iterations_with_densification_match_the_restated_loop(opt_cls):
    base = C.Model(C.random_tensors(20_000, 3, 21, DEV), opt_cls)
    runs = []
    for ours in (False, True):
        m = C.twin(base)
        torch.manual_seed(5)
        for it in range(1, 31):
            C.train_steps(m, 1)
            n = m._xyz.shape[0]
            g = torch.Generator().manual_seed(it)
            vp = torch.zeros(n, 3, device=DEV, requires_grad=True)
            vp.grad = (torch.randn(n, 3, generator=g) * 3e-4).to(DEV)
            f = (torch.rand(n, generator=g) < 0.4).to(DEV)
            (D.add_densification_stats if ours else type(m).reference_add_densification_stats)(m, vp, f)
            if it % 10 == 0:
                (D.densify_and_prune if ours else type(m).reference_densify_and_prune)(m, THR, MIN_OP, EXTENT, 20 if it > 10 else None)
        runs.append((C.snapshot(m), torch.cuda.get_rng_state()))
    C.assert_same(runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1]) and runs[1][0]["xyz"].shape[0] > 20_000


# --- non-finite rows, runs of one class, the seams of the scan, apply and stats kernels ---

@pytest.mark.parametrize("mss", [None, 20])
@pytest.mark.parametrize("opt_cls", [torch.optim.Adam, O.Adam], ids=["torch_adam", "gsr_adam"])
def test_non_finite_rows_equal_the_restated_method(opt_cls, mss):
    """NaN and both infinities in the statistics, the scales and the opacities (densify_cases.inject_non_finite), moments present.
    At extent 100 the clone bound is exp(0), which the ``scaling.exp0`` rows sit on."""
    base, _ = C.non_finite_model(5000, 3, 1, device=DEV, opt_cls=opt_cls)
    for extent in (EXTENT, 100.0):
        got = run_both(base, mss, extent=extent)
        assert got["scaling"].isnan().any() and got["opacity"].isnan().any() and got["xyz"].shape[0] != 5000


def test_non_finite_rows_plan_kernel_equals_plan_host():
    """The plan kernel alone on the same rows.  With a threshold of 0, which ``kernel_takes`` never lets through to the kernels, g = 0
    passes the gradient tests and g = NaN would not: the one setting at which ``grads[grads.isnan()] = 0.0`` is visible in the plan."""
    base, rows = C.non_finite_model(5000, 3, 1, device=DEV)
    for thr, extent, ws in ((THR, EXTENT, False), (THR, EXTENT, True), (THR, 100.0, True), (0.0, EXTENT, False), (0.0, EXTENT, True)):
        want = plan_kernel_against_plan_host(base, 0.1 * extent if ws else None, thr, 0.01 * extent)
        assert all(c > 0 for c in want["counts"].tolist()[:3])
    r = torch.cat([rows[k] for k in ("accum.nan", "denom.0.accum0", "denom.nan", "denom.+inf.accum+inf")]).to(DEV)
    assert bool((want["clone"][r] | want["split"][r] | ~want["keep"][r]).all())   # at threshold 0 these rows are hot


RUN_N = 5000 + 37


@pytest.mark.parametrize("name", list(C.run_layouts(8)))
def test_runs_of_one_class_equal_the_restated_method(name):
    """Waves, quarter workgroups and whole workgroups of one class; all rows of one class; a class on the last wave or the two end rows
    only: ballots of all zeros and all ones, per-wave counts of 0 and 64, workgroup counts of 0 and 1024."""
    cls = layout(name, RUN_N)
    degree = 3 if name == "mod7" else 0
    base = C.rows_of_classes(cls, degree, seed=4, device=DEV, steps=1 if degree else 0)
    for mss in (None, 20):
        plan_kernel_against_plan_host(base, 0.1 * EXTENT if mss else None)
        assert run_both(base, mss)["xyz"].shape[0] == C.rows_left(cls, mss)


@pytest.mark.parametrize("name", ["scanA", "scanB", "scanC"])
def test_scan_carry_across_its_step_of_256_workgroups(name):
    n = 262_144 + 1024 + 5                                                  # 258 workgroups: two steps of the scan kernel
    cls = layout(name, n)
    base = C.rows_of_classes(cls, 0, seed=5, device=DEV)
    for mss in (None, 20):
        plan_kernel_against_plan_host(base, 0.1 * EXTENT if mss else None)
        assert run_both(base, mss)["xyz"].shape[0] == C.rows_left(cls, mss)


def run_poisoned(base, mss):
    """run_both with every fp32 output pre-filled with 0xFF bytes (as test_apply_writes_every_element does)."""
    real_empty = torch.empty

    def poisoned(*a, **k):
        t = real_empty(*a, **k)
        if t.is_cuda and t.dtype == torch.float32:
            t.view(torch.uint8).fill_(0xFF)
        return t

    a, b = C.twin(base), C.twin(base)
    torch.manual_seed(2)
    a.reference_densify_and_prune(THR, MIN_OP, EXTENT, mss)
    torch.manual_seed(2)
    torch.empty = poisoned
    try:
        D.densify_and_prune(b, THR, MIN_OP, EXTENT, mss)
    finally:
        torch.empty = real_empty
    C.assert_same(C.snapshot(a), C.snapshot(b))


@pytest.mark.parametrize("degree", [2, 1])
@pytest.mark.parametrize("name, rows", [("seam1047", 2047), ("seam1048", 2048), ("seam1049", 2049), ("only_children", 600), ("no_child", 0)])
def test_apply_at_chunk_ends_and_generic_row_widths(name, rows, degree):
    """f_rest of 24 and 9 floats (the apply kernel's generic width) with moments; results of 2047, 2048 and 2049 rows: at 2048 every
    tensor of every width ends on a chunk of 2048 floats; a result of children only (n_keep = 0) and one of no rows at all."""
    cls = layout(name, 0)
    base = C.rows_of_classes(cls, degree, seed=6, device=DEV, steps=1)
    assert base._features_rest[0].numel() == {2: 24, 1: 9}[degree]
    for mss in (None, 20):
        assert run_both(base, mss)["xyz"].shape[0] == rows == C.rows_left(cls, mss)
        run_poisoned(base, mss)


@pytest.mark.parametrize("radii, off", [(True, 0), (False, 0), (True, 1)], ids=["radii", "no_radii", "radii_offset_by_one"])
def test_stats_grid_stride_walk(radii, off):
    """More rows than one pass of the stats kernel's largest grid covers (2048 * 4 workgroups * 256 lanes * 4 rows = 8 388 608), against
    torch's boolean-index lines on the device; ``off`` = 1 starts every array one element in, which takes the scalar path."""
    n = 8_388_608 + 4099
    g = torch.Generator(device=DEV).manual_seed(9)
    grad = (torch.randn(n + 1, 3, device=DEV, generator=g) * 1e-3)[off:off + n]
    f = (torch.rand(n + 1, device=DEV, generator=g) < 0.3)[off:off + n]
    a = torch.rand(n + 1, 1, device=DEV, generator=g)[off:off + n]
    d = torch.randint(0, 5, (n + 1, 1), device=DEV, generator=g).float()[off:off + n]
    r = torch.randint(0, 90, (n + 1,), device=DEV, generator=g, dtype=torch.int32)[off:off + n]
    mr = (torch.rand(n + 1, device=DEV, generator=g) * 60)[off:off + n]
    assert all(t.is_contiguous() and (t.data_ptr() % 16 != 0) == bool(off) for t in (grad, a, d, r, mr)) and f.data_ptr() % 4 == off
    assert bool(f[8_388_608:].any()) and not bool(f[8_388_608:].all())
    wa, wd, wm = a.clone(), d.clone(), mr.clone()
    if not radii:
        r = mr = None
    wa[f] += torch.norm(grad[f, :2], dim=-1, keepdim=True)
    wd[f] += 1
    if radii:
        wm[f] = torch.max(wm[f], r[f].float())
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        D.accumulate_stats(grad, f, a, d, r, mr)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(wa, a) and torch.equal(wd, d) and (mr is None or torch.equal(wm, mr))
