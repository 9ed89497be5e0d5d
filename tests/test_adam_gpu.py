"""The fused Adam step (gsr_adam.hip through autovfx_amd.optim.Adam) on the GPU, held bit for bit to torch.optim.Adam as the
reference's training loops build it: the contraction of torch's foreach ops probed against numpy, then many steps over C3-sized groups
with odd sizes, special gradients, an lr schedule and the densification's state surgery between steps; version counters, no host
synchronisation, side streams, and a short training loop through install()'s render() and fused SSIM."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from autovfx_amd import _lib, optim as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
C3 = 3_000_000
SHAPES = {"xyz": (3,), "f_dc": (1, 3), "f_rest": (15, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,)}
LRS = {"xyz": 1.6e-4 * 5.0, "f_dc": 2.5e-3, "f_rest": 2.5e-3 / 20.0, "opacity": 0.05, "scaling": 5e-3, "rotation": 1e-3}


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# ---- what torch's foreach kernels compute: one rounding per op, or a fused multiply-add ----

def fma32(x, y, z):
    """fl32(x * y + z) with ONE rounding, in numpy: the product is exact in float64, the sum's float64 rounding error is recovered
    (two-sum) and decides the ties that a second rounding to float32 would otherwise break wrongly."""
    x, y, z = (np.asarray(t, np.float32).astype(np.float64) for t in (x, y, z))
    with np.errstate(all="ignore"):
        p = x * y
        s = p + z
        bp = s - z
        err = (p - bp) + (z - (s - bp))
        r = s.astype(np.float32)
        r64 = r.astype(np.float64)
        toward = np.nextafter(r, np.where(s > r64, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
        tie = np.isfinite(s) & np.isfinite(err) & (s != r64) & (s == (r64 + toward.astype(np.float64)) / 2) & (err != 0)
        other_side = (toward.astype(np.float64) > r64) == (err > 0)
        return np.where(tie & other_side, toward, r)


def probe_values(n, seed):
    g = np.random.default_rng(seed)
    return (g.standard_normal(n) * np.exp2(g.integers(-20, 20, n))).astype(np.float32)


def on_gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def test_foreach_ops_fuse_the_multiply_add():
    """The kernel writes steps 1, 2 and 4 of the update as fmas (gsr_adam.hip): each foreach op of torch's Adam must match the
    fused form and not the unfused one on this build.  A failure names the op whose contraction changed."""
    n = 1 << 20
    a, b, c = probe_values(n, 1), probe_values(n, 2), np.abs(probe_values(n, 3)) + np.float32(1e-3)
    found = {}
    # _foreach_lerp_(m, g, w): m + w (g - m) for a weight w < 0.5 (beta1 > 0.5, the only lerp the kernel takes)
    m, gr = on_gpu(a), on_gpu(b)
    torch._foreach_lerp_([m], [gr], 1 - 0.9)
    w32, diff = np.float32(1 - 0.9), b - a
    found["lerp"] = (m.cpu().numpy(), fma32(w32, diff, a), a + w32 * diff)
    # _foreach_addcmul_(v, g, g, c): v + c (g g)
    v, gr = on_gpu(np.abs(a)), on_gpu(b)
    torch._foreach_addcmul_([v], [gr], [gr], 1 - 0.999)
    c32 = np.float32(1 - 0.999)
    found["addcmul"] = (v.cpu().numpy(), fma32(c32, b * b, np.abs(a)), np.abs(a) + c32 * (b * b))
    # _foreach_addcdiv_(p, m, d, [a]): p + a (m / d)
    p, m, d = on_gpu(a), on_gpu(b), on_gpu(c)
    step = -1.6e-4 / (1 - 0.9 ** 3)
    torch._foreach_addcdiv_([p], [m], [d], [step])
    s32 = np.float32(step)
    found["addcdiv"] = (p.cpu().numpy(), fma32(s32, b / c, a), a + s32 * (b / c))
    # _foreach_div_(d, [s2]): a true division (no reciprocal)
    d = on_gpu(a)
    s2 = (1 - 0.999 ** 3) ** 0.5
    torch._foreach_div_([d], [s2])
    found["div"] = (d.cpu().numpy(), a / np.float32(s2), a * (np.float32(1) / np.float32(s2)))
    for name, (got, fused, plain) in found.items():
        assert np.array_equal(got.view(np.int32), fused.view(np.int32)), f"torch's {name} is not the form gsr_adam.hip uses"
        assert not np.array_equal(fused.view(np.int32), plain.view(np.int32)), f"the {name} probe cannot tell the forms apart"


# ---- bit equality with the reference's optimizer ----

def c3_groups(n, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    out = [{"params": [torch.nn.Parameter(torch.randn((n, *SHAPES[k]), generator=g, device=DEV))], "lr": LRS[k], "name": k}
           for k in SHAPES]
    for size in (1, 3, 5, 1023, 0):
        out.append({"params": [torch.nn.Parameter(torch.randn(size, generator=g, device=DEV))], "lr": 1e-2, "name": f"odd{size}"})
    base = torch.randn(MISALIGNED + 2, generator=g, device=DEV)
    out.append({"params": [torch.nn.Parameter(base[1:1 + MISALIGNED])], "lr": 3e-3, "name": "offset"})   # storage offset 4 bytes
    return out


MISALIGNED = 3 * 4096 + 5   # three full chunks and a tail, all on the kernel's element-by-element path


def offset_copy(t):
    """A copy of ``t`` at the same storage offset in a fresh buffer: a view 4 bytes into its allocation stays 4 bytes in."""
    buf = torch.empty(t.storage_offset() + t.numel(), dtype=t.dtype, device=t.device)
    out = buf[t.storage_offset():].view(t.shape)
    out.copy_(t.detach())
    return out


def twin(groups):
    return [{**gr, "params": [torch.nn.Parameter(offset_copy(p)) for p in gr["params"]]} for gr in groups]


@pytest.fixture
def launches(monkeypatch):
    """Every gsr_adam_step call as (count, w, b2, c, eps), the library still doing the work."""
    calls = []
    real = _lib.lib.gsr_adam_step

    def counting(tensors, count, w, b2, c, eps, stream):
        calls.append((count, w, b2, c, eps))
        return real(tensors, count, w, b2, c, eps, stream)

    monkeypatch.setattr(_lib.lib, "gsr_adam_step", counting)
    return calls


def nasty_grads(shape, gen):
    g = torch.randn(shape, generator=gen, device=DEV)
    flat = g.view(-1)
    n = flat.numel()
    if n >= 8:
        u = torch.rand(n, generator=gen, device=DEV)
        flat[u < 0.05] = 0.0
        flat[(u >= 0.05) & (u < 0.10)] *= 1e-21       # squares below the normal range
        flat[(u >= 0.10) & (u < 0.12)] *= 3e19        # squares that overflow
        flat[(u >= 0.12) & (u < 0.1202)] = float("inf")
        flat[(u >= 0.1202) & (u < 0.1204)] = float("-inf")
        flat[(u >= 0.1204) & (u < 0.1206)] = float("nan")
    return g


def expon_lr(step, lr_init=1.6e-4 * 5.0, lr_final=1.6e-6 * 5.0, max_steps=60):
    t = np.clip(step / max_steps, 0, 1)
    return np.exp(np.log(lr_init) * (1 - t) + np.log(lr_final) * t)


def swap_param(opt, group, new_param, new_state):
    old = group["params"][0]
    opt.state.pop(old, None)
    group["params"][0] = new_param
    if new_state is not None:
        opt.state[new_param] = new_state


def surgery(opt, kind, arg):
    """The densification's edits of an Adam, restated: keep rows by a mask, append zero-state rows, replace the opacity."""
    for group in opt.param_groups:
        if group["name"] not in SHAPES:
            continue
        p = group["params"][0]
        st = opt.state.get(p)
        if kind == "prune":
            new_p = torch.nn.Parameter(p.detach()[arg])
            new_st = None if st is None else {"step": st["step"], "exp_avg": st["exp_avg"][arg], "exp_avg_sq": st["exp_avg_sq"][arg]}
        elif kind == "cat":
            extra = arg[group["name"]]
            new_p = torch.nn.Parameter(torch.cat((p.detach(), extra), 0))
            new_st = None if st is None else {"step": st["step"],
                                              "exp_avg": torch.cat((st["exp_avg"], torch.zeros_like(extra)), 0),
                                              "exp_avg_sq": torch.cat((st["exp_avg_sq"], torch.zeros_like(extra)), 0)}
        else:
            if group["name"] != "opacity":
                continue
            new_p = torch.nn.Parameter(torch.minimum(p.detach(), torch.full_like(p, arg)))
            new_st = None if st is None else {"step": st["step"], "exp_avg": torch.zeros_like(new_p), "exp_avg_sq": torch.zeros_like(new_p)}
        swap_param(opt, group, new_p, new_st)


def compare(ref, ours, it):
    for gr, go in zip(ref.param_groups, ours.param_groups):
        pr, po = gr["params"][0], go["params"][0]
        assert same_bits(pr, po), (it, gr["name"], "param")
        sr, so = ref.state.get(pr), ours.state.get(po)
        assert (sr is None) == (so is None), (it, gr["name"])
        if sr is not None:
            assert torch.equal(sr["step"], so["step"]) and so["step"].device.type == "cpu"
            assert same_bits(sr["exp_avg"], so["exp_avg"]), (it, gr["name"], "exp_avg")
            assert same_bits(sr["exp_avg_sq"], so["exp_avg_sq"]), (it, gr["name"], "exp_avg_sq")


def test_bit_equal_to_torch_adam_over_many_steps_with_surgery(launches):
    ga = c3_groups(C3, 5)
    gb = twin(ga)
    offset = gb[-1]["params"][0]
    assert gb[-1]["name"] == "offset" and offset.data_ptr() % 16 == 4 and offset.numel() == MISALIGNED   # the tensor stepped
    ref = torch.optim.Adam(ga, lr=0.0, eps=1e-15)
    ours = O.Adam(gb, lr=0.0, eps=1e-15)
    for it in range(1, 56):
        for opt in (ref, ours):
            opt.param_groups[0]["lr"] = expon_lr(it)
        gen_a, gen_b = (torch.Generator(device=DEV).manual_seed(7000 + it) for _ in range(2))
        for gr_a, gr_b in zip(ref.param_groups, ours.param_groups):
            pa, pb = gr_a["params"][0], gr_b["params"][0]
            ga_, gb_ = nasty_grads(pa.shape, gen_a), nasty_grads(pb.shape, gen_b)
            skip = gr_a["name"] == ("rotation" if it % 2 else "odd5")        # one group without a gradient, as a frozen one
            pa.grad, pb.grad = (None, None) if skip else (ga_, gb_)
        assert O.kernel_takes(ours.param_groups, ours.state)
        ref.step()
        before = len(launches)
        ours.step()
        assert len(launches) == before + 1 and launches[-1][0] == 11   # every group with a gradient, one launch
        compare(ref, ours, it)
        n = ref.param_groups[0]["params"][0].shape[0]
        if it == 10:
            mask = torch.rand(n, generator=torch.Generator(device=DEV).manual_seed(11), device=DEV) > 0.1
            surgery(ref, "prune", mask)
            surgery(ours, "prune", mask)
        elif it == 20:
            gen = torch.Generator(device=DEV).manual_seed(12)
            extra = {k: torch.randn((1001, *SHAPES[k]), generator=gen, device=DEV) for k in SHAPES}
            surgery(ref, "cat", extra)
            surgery(ours, "cat", extra)
        elif it == 30:
            surgery(ref, "replace", -4.0)
            surgery(ours, "replace", -4.0)
        if it in (10, 20, 30):
            compare(ref, ours, it)
    assert ours.param_groups[0]["params"][0].shape[0] != C3
    assert ours.param_groups[-1]["params"][0] is offset and offset.data_ptr() % 16 == 4


@pytest.mark.parametrize("stepped,counts,offset_at", [(17, [16, 1], 17), (35, [16, 16, 3], 20)])
def test_more_tensors_than_one_launch_takes(launches, stepped, counts, offset_at):
    """A launch takes 16 tensors (ADAM_MAX_TENSORS); optim.py cuts a longer list into launches of 16.  17 and 35 single-tensor groups
    with a gradient, and one more without at index 3, so that the cut does not fall on parameter index 16: sizes 1, 3, 1023, 4096,
    4097 and 70 001 in turn, one tensor of numel 0, and after the first cut one parameter 4 bytes into its allocation.  The empty
    tensor has a gradient, so torch's _init_group hands it on and optim.py passes it as a descriptor of no chunks: it counts as one
    of a launch's tensors.  After each of 12 steps every p, exp_avg and exp_avg_sq has torch.optim.Adam's bits; the second and third
    launch step their own tensors (a launch that repeated the first 16 would leave the rest unstepped and step those twice), and
    their chunk numbering starts again at their first tensor."""
    assert _lib.ADAM_MAX_TENSORS == 16
    gen = torch.Generator(device=DEV).manual_seed(17)
    sizes = (1, 3, 1023, 4096, 4097, 70_001)
    ga = []
    for i in range(stepped + 1):
        if i == offset_at:
            p = torch.randn(MISALIGNED + 2, generator=gen, device=DEV)[1:1 + MISALIGNED]
        else:
            p = torch.randn(0 if i == 6 else sizes[i % len(sizes)], generator=gen, device=DEV)
        ga.append({"params": [torch.nn.Parameter(p)], "lr": 1e-3 * (1 + i), "name": f"t{i}"})
    gb = twin(ga)
    assert offset_at > 16 and gb[offset_at]["params"][0].data_ptr() % 16 == 4 and gb[6]["params"][0].numel() == 0
    numels = [gr["params"][0].numel() for i, gr in enumerate(gb) if i != 3]
    assert all(max(numels[cut:cut + 16]) > 4096 for cut in range(16, stepped, 16))   # a tensor of several chunks after every cut
    ref, ours = torch.optim.Adam(ga, lr=0.0, eps=1e-15), O.Adam(gb, lr=0.0, eps=1e-15)
    for it in range(1, 13):
        gen_a, gen_b = (torch.Generator(device=DEV).manual_seed(8000 + it) for _ in range(2))
        for i, (gr_a, gr_b) in enumerate(zip(ref.param_groups, ours.param_groups)):
            pa, pb = gr_a["params"][0], gr_b["params"][0]
            g_a, g_b = nasty_grads(pa.shape, gen_a), nasty_grads(pb.shape, gen_b)
            pa.grad, pb.grad = (None, None) if i == 3 else (g_a, g_b)
        assert O.kernel_takes(ours.param_groups, ours.state)
        ref.step()
        before = len(launches)
        ours.step()
        assert [c[0] for c in launches[before:]] == counts and sum(counts) == stepped, launches[before:]
        compare(ref, ours, it)
    assert ours.state.get(gb[3]["params"][0]) is None and same_bits(ga[3]["params"][0], gb[3]["params"][0])
    assert float(ours.state[gb[offset_at]["params"][0]]["step"]) == 12.0


def test_misaligned_gradient_or_moment_with_an_aligned_parameter():
    """The vector path needs all four pointers 16-byte aligned: an aligned parameter with a gradient, or with moments, 4 bytes into
    their allocations runs element by element, with torch's bits."""
    gen = torch.Generator(device=DEV).manual_seed(13)
    ga = [{"params": [torch.nn.Parameter(torch.randn(MISALIGNED, generator=gen, device=DEV))], "name": "grad_off"},
          {"params": [torch.nn.Parameter(torch.randn(MISALIGNED, generator=gen, device=DEV))], "name": "exp_avg_off"},
          {"params": [torch.nn.Parameter(torch.randn(MISALIGNED, generator=gen, device=DEV))], "name": "exp_avg_sq_off"}]
    gb = twin(ga)
    ref, ours = torch.optim.Adam(ga, lr=1e-2, eps=1e-15), O.Adam(gb, lr=1e-2, eps=1e-15)
    for it in range(12):
        for gr_a, gr_b in zip(ref.param_groups, ours.param_groups):
            g = nasty_grads((MISALIGNED,), gen)
            gr_a["params"][0].grad = g
            gb_ = torch.empty(MISALIGNED + 1, device=DEV)[1:] if gr_b["name"] == "grad_off" else torch.empty_like(g)
            gb_.copy_(g)
            gr_b["params"][0].grad = gb_
        if it == 1:   # moments moved 4 bytes into fresh allocations, same values
            for gr_b in ours.param_groups:
                key = gr_b["name"][:-4]
                if key in ("exp_avg", "exp_avg_sq"):
                    st = ours.state[gr_b["params"][0]]
                    moved = torch.empty(MISALIGNED + 1, device=DEV)[1:]
                    moved.copy_(st[key])
                    st[key] = moved
        for gr_b in ours.param_groups:
            p = gr_b["params"][0]
            assert p.data_ptr() % 16 == 0
            if gr_b["name"] == "grad_off":
                assert p.grad.data_ptr() % 16 == 4
            elif it >= 1:
                assert ours.state[p][gr_b["name"][:-4]].data_ptr() % 16 == 4
        assert O.kernel_takes(ours.param_groups, ours.state)
        ref.step()
        ours.step()
        compare(ref, ours, it)


def test_other_betas_and_eps_in_separate_launches(launches):
    """Groups with different betas and eps go out as one launch each; beta1 <= 0.5 (ATen's other lerp branch) is torch's step."""
    gen = torch.Generator(device=DEV).manual_seed(9)
    ga = [{"params": [torch.nn.Parameter(torch.randn(70_001, generator=gen, device=DEV))], "betas": (0.8, 0.95), "eps": 1e-6},
          {"params": [torch.nn.Parameter(torch.randn(4096 * 3, generator=gen, device=DEV))]}]
    gb = twin(ga)
    ref, ours = torch.optim.Adam(ga, lr=1e-2), O.Adam(gb, lr=1e-2)
    for it in range(20):
        for gr_a, gr_b in zip(ref.param_groups, ours.param_groups):
            g = nasty_grads(gr_a["params"][0].shape, gen)
            gr_a["params"][0].grad, gr_b["params"][0].grad = g, g.clone()
        assert O.kernel_takes(ours.param_groups, ours.state)
        ref.step()
        before = len(launches)
        ours.step()
        f32 = lambda x: float(np.float32(x))
        assert sorted(launches[before:]) == sorted([(1, f32(1 - 0.8), f32(0.95), f32(1 - 0.95), f32(1e-6)),
                                                    (1, f32(1 - 0.9), f32(0.999), f32(1 - 0.999), f32(1e-8))]), launches[before:]
        for i, (gr_a, gr_b) in enumerate(zip(ref.param_groups, ours.param_groups)):
            pa, pb = gr_a["params"][0], gr_b["params"][0]
            for name, x, y in (("param", pa, pb), ("exp_avg", ref.state[pa]["exp_avg"], ours.state[pb]["exp_avg"]),
                               ("exp_avg_sq", ref.state[pa]["exp_avg_sq"], ours.state[pb]["exp_avg_sq"])):
                bad = (bits(x) != bits(y)).nonzero()
                assert bad.numel() == 0, (it, i, name, bad[:4].tolist(), x[bad[:4, 0]].tolist(), y[bad[:4, 0]].tolist())
    for betas in ((0.3, 0.95), (0.5, 0.95), (1.2, 0.95)):   # (param_groups may be edited past the constructor's checks)
        ours.param_groups[0]["betas"] = betas
        assert not O.kernel_takes(ours.param_groups, ours.state)
    before = len(launches)
    for gr_a, gr_b in zip(ref.param_groups, ours.param_groups):
        g = nasty_grads(gr_a["params"][0].shape, gen)
        gr_a["params"][0].grad, gr_b["params"][0].grad = g, g.clone()
    ref.param_groups[0]["betas"] = ours.param_groups[0]["betas"] = (0.3, 0.95)
    ref.step()
    ours.step()   # torch's own step: no launch
    assert len(launches) == before
    for gr_a, gr_b in zip(ref.param_groups, ours.param_groups):
        assert same_bits(gr_a["params"][0], gr_b["params"][0])


def small_pair(seed=3, n=50_000):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    ga = [{"params": [torch.nn.Parameter(torch.randn((n, *SHAPES[k]), generator=gen, device=DEV))], "lr": LRS[k], "name": k}
          for k in SHAPES]
    return ga, twin(ga)


def feed(groups, it):
    gen = torch.Generator(device=DEV).manual_seed(100 + it)
    for gr in groups:
        p = gr["params"][0]
        p.grad = torch.randn(p.shape, generator=gen, device=DEV)


def test_version_counters_go_up():
    _, gb = small_pair()
    ours = O.Adam(gb, lr=0.0, eps=1e-15)
    feed(gb, 0)
    ours.step()
    for it in range(1, 3):
        feed(gb, it)
        before = [(p._version, ours.state[p]["exp_avg"]._version, ours.state[p]["exp_avg_sq"]._version)
                  for p in (gr["params"][0] for gr in gb)]
        ours.step()
        after = [(p._version, ours.state[p]["exp_avg"]._version, ours.state[p]["exp_avg_sq"]._version)
                 for p in (gr["params"][0] for gr in gb)]
        for b, a in zip(before, after):
            assert all(y > x for x, y in zip(b, a)), (b, a)


def test_geometry_reuse_sees_the_step():
    """The binding reuses a call's geometry for the next call only while the geometry tensors keep their version: a step between
    two calls must make the second one recompute, as with torch's in-place Adam."""
    from diff_gaussian_rasterization import _C
    from autovfx_amd import scenes
    from helpers import settings_for
    cloud, cam = scenes.config_c1(P=3000, seed=21), scenes.c1_camera(250, 130)
    c = cloud.to(DEV)
    st = settings_for(cam, DEV, (0.2, 0.4, 0.1), 1.0, cloud.sh_degree)
    e = torch.Tensor([])
    xyz = torch.nn.Parameter(c.means3D.clone())
    opt = O.Adam([xyz], lr=0.05)
    colors = torch.rand((cloud.P, 3), generator=torch.Generator(device=DEV).manual_seed(3), device=DEV)
    args = lambda colors_, sh: (st.bg, xyz, colors_, c.opacities, c.scales, c.rotations, 1.0, e, st.viewmatrix, st.projmatrix,
                                st.tanfovx, st.tanfovy, st.image_height, st.image_width, sh, st.sh_degree, st.campos, False, False)
    xyz.grad = torch.randn(xyz.shape, generator=torch.Generator(device=DEV).manual_seed(4), device=DEV)
    try:
        with torch.no_grad():
            _C.set_geometry_cache(True)
            _C.rasterize_gaussians(*args(e, c.shs))
            hits = _C.cache_stats["hits"]
            _C.rasterize_gaussians(*args(colors, e))     # control: nothing in between, the geometry is reused
            assert _C.cache_stats["hits"] == hits + 1
            _C.rasterize_gaussians(*args(e, c.shs))
            opt.step()                                   # moves every mean by about lr
            misses = _C.cache_stats["misses"]
            reused = _C.rasterize_gaussians(*args(colors, e))[1].clone()
            assert _C.cache_stats["misses"] == misses + 1
            _C.set_geometry_cache(False)
            fresh = _C.rasterize_gaussians(*args(colors, e))[1].clone()
    finally:
        _C.set_geometry_cache(None)
    assert same_bits(reused, fresh)


def test_no_host_synchronisation_and_side_streams():
    ga, gb = small_pair(4)
    gc = twin(ga)
    ref, ours, side = torch.optim.Adam(ga, lr=0.0, eps=1e-15), O.Adam(gb, lr=0.0, eps=1e-15), O.Adam(gc, lr=0.0, eps=1e-15)
    stream = torch.cuda.Stream()
    for it in range(4):
        feed(ga, it)
        feed(gb, it)
        feed(gc, it)
        ref.step()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            ours.step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            side.step()
        torch.cuda.current_stream().wait_stream(stream)
        torch.cuda.synchronize()
        for x, y, z in zip(ga, gb, gc):
            assert same_bits(x["params"][0], y["params"][0]) and same_bits(x["params"][0], z["params"][0])


def test_training_loop_matches_torch_adam_bit_for_bit():
    """The reference's iteration through install()'s pieces: render() with grad, 0.8 L1 + 0.2 (1 - ssim), backward, step,
    zero_grad(set_to_none=True), with deterministic gradient sums; the loss goes down and the parameters are torch's Adam's."""
    from autovfx_amd import renderer, ssim as S
    from autovfx_amd.cameras import orbit_cameras
    from test_raw_autograd_gpu import PARAMS, leaves
    from test_raw_gpu import raw_model
    cam = orbit_cameras(12, 192, 120)[4].to(DEV)
    bg = torch.zeros(3, device=DEV)
    target = torch.rand((4, 120, 192), generator=torch.Generator(device=DEV).manual_seed(21), device=DEV)

    def loop(cls):
        m = leaves(raw_model(8_000, 404, nasty=False))
        opt = cls([{"params": [getattr(m, k)], "lr": 5e-3, "name": k} for k in PARAMS], lr=0.0, eps=1e-15)
        losses = []
        for _ in range(12):
            img = renderer.render(cam, m, renderer.PipelineParams, bg)["render"]
            loss = 0.8 * (img - target).abs().mean() + 0.2 * (1.0 - S.ssim(img, target))
            loss.backward()
            opt.step()
            opt.zero_grad(set_to_none=True)
            losses.append(float(loss.detach()))
        return losses, [getattr(m, k).detach().clone() for k in PARAMS]

    before = _lib.get_option(_lib.OPT_BACKWARD_DETERMINISTIC)
    _lib.set_option(_lib.OPT_BACKWARD_DETERMINISTIC, 1)
    try:
        la, pa = loop(torch.optim.Adam)
        lb, pb = loop(O.Adam)
    finally:
        _lib.set_option(_lib.OPT_BACKWARD_DETERMINISTIC, before)
    assert lb[-1] < lb[0], lb
    assert la == lb
    for x, y in zip(pa, pb):
        assert same_bits(x, y)


def test_a_refused_launch_leaves_the_step_counters_alone(monkeypatch):
    """The counters move after the launches: a launch that fails raises and leaves ``step`` where it was."""
    _, gb = small_pair(5, 10_000)
    ours = O.Adam(gb, lr=1e-3)
    feed(gb, 0)
    ours.step()
    before = [float(ours.state[gr["params"][0]]["step"]) for gr in gb]
    params = [gr["params"][0].detach().clone() for gr in gb]
    monkeypatch.setattr(_lib.lib, "gsr_adam_step", lambda *a: -1)
    feed(gb, 1)
    with pytest.raises(RuntimeError, match="gsr_adam_step failed"):
        ours.step()
    assert [float(ours.state[gr["params"][0]]["step"]) for gr in gb] == before == [1.0] * len(gb)
    assert all(same_bits(x, gr["params"][0]) for x, gr in zip(params, gb))
