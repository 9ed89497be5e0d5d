"""gsr_backward_raw / the differentiable raw render path (VERDICT round 3, items 3d and "missing" 5): with autograd on,
``render()`` makes ONE rasterizer call from the model's raw tensors and differentiates it with the activations' chain rule
inside the per-Gaussian kernel.  Second path: the reference's structure run through PyTorch autograd on the same GPU -- exp /
sigmoid / normalize / cat / get_normal in PyTorch, two ``GaussianRasterizer`` calls (``renderer.RAW_AUTOGRAD = False``).
Forward values must be bit-identical.  Gradients of both paths are held to the truth-based bar of tests/test_backward_gpu.py in
all three of its modes (float atomics, GSR_OPT_BACKWARD_DETERMINISTIC, depth slabs), whatever the loss reads:

* truth = the fp64 oracle's gradients with respect to the activated parameters, chained through exp / sigmoid / normalize / cat
  by float64 autograd; the reference's fp32 sample = the CPU oracle's fp32 gradients chained by float32 autograd (what the
  reference's own training step computes);
* the normal maps come from a second pass over the same lists whose colours are the view normals: the CPU oracle runs that pass
  with ``colors_precomp`` = those colours, and autograd carries its colour gradients back through ``get_normal * 0.5 + 0.5`` to
  the quaternion, with the minimum axis and the flip taken as fp32 took them on the GPU (``raw_oracles``);
* the per-pixel post-processing of the normal maps (normalize, pseudo normals) is PyTorch fp32 and not under test: the oracles get
  the per-pixel gradients the library actually received.

The two paths are also compared with each other under GSR_OPT_BACKWARD_DETERMINISTIC, where both are pure functions of the
inputs.  Bar: max |a - b| <= 2e-4 * max|b| + 1e-6 per gradient tensor.  The binding itself (``rasterize_gaussians_raw`` /
``rasterize_gaussians_raw_backward``) is driven directly with seeded per-pixel gradients for all four images.
"""
import numpy as np
import pytest
import torch

from autovfx_amd import _lib, renderer
from autovfx_amd import gaussian_model as gm
from autovfx_amd.cameras import orbit_cameras
from oracle import cpu_oracle

from helpers import assert_gradients_vs_truth, decode_scratch, report_row
from test_backward_gpu import MODES, assert_forward_state, assert_same_bits
from test_oracle_backward import pixel_grads
from test_raw_gpu import RENDER_KEYS, call_raw, raw_model, torch_activated

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL, ABS = 2e-4, 1e-6
PARAMS = ("_xyz", "_scaling", "_rotation", "_opacity", "_features_dc", "_features_rest")


def leaves(m):
    for k in PARAMS:
        setattr(m, k, getattr(m, k).detach().clone().requires_grad_(True))
    return m


def weights(shape_hw, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    H, W = shape_hw
    r = lambda *s: torch.randn(*s, device=DEV, generator=g) / (H * W)
    return {"render": r(4, H, W), "depth": r(H, W) * 0.1, "normal": r(H, W, 3), "pseudo_normal": r(H, W, 3) * 0.01}


def set_mode(mode):
    """The library options of one mode: test_backward_gpu.MODES -- "atomic" (a full forward call, float atomics), "deterministic",
    "slabs" (the forward an inference call cut into small depth slabs, GSR_OPT_GRAD_SLABS) -- or "default", the library's own
    options (float atomics; a grad-mode forward is a slab call with the default slab sizes).  restore_options() undoes it."""
    _lib.set_option(_lib.OPT_BACKWARD_DETERMINISTIC, 1 if mode == "deterministic" else 0)
    _lib.set_option(_lib.OPT_GRAD_SLABS, 0 if mode == "atomic" else 1)
    if mode == "slabs":
        _lib.set_option(_lib.OPT_SLABS, 0)
        _lib.set_option(_lib.OPT_SLAB_FIRST, 6)
        _lib.set_option(_lib.OPT_SLAB_MIN_REST, 0)


def restore_options():
    for opt, value in ((_lib.OPT_BACKWARD_DETERMINISTIC, 0), (_lib.OPT_GRAD_SLABS, 1), (_lib.OPT_SLABS, 2), (_lib.OPT_SLAB_FIRST, 400),
                       (_lib.OPT_SLAB_MIN_REST, 3000000), (_lib.OPT_TILE_CULL, 1)):
        _lib.set_option(opt, value)


def run(m, cam, bg, wts, raw_autograd, keys, mode="deterministic"):
    saved = renderer.RAW_AUTOGRAD
    renderer.RAW_AUTOGRAD = raw_autograd
    set_mode(mode)
    try:
        for k in PARAMS:
            getattr(m, k).grad = None
        out = renderer.render(cam, m, renderer.PipelineParams, bg)
        loss = sum((out[k] * wts[k]).sum() for k in keys)
        loss.backward()
        torch.cuda.synchronize()
        grads = {k: getattr(m, k).grad.clone() if getattr(m, k).grad is not None else None for k in PARAMS}
        grads["viewspace_points"] = out["viewspace_points"].grad.clone() if out["viewspace_points"].grad is not None else None
        return {k: out[k].detach().clone() for k in RENDER_KEYS}, grads
    finally:
        renderer.RAW_AUTOGRAD = saved
        restore_options()


def view_normal_decisions(m, cam):
    """The discrete decisions of ``get_normal(dir) * 0.5 + 0.5`` as fp32 took them on the GPU -- which column of the rotation is the
    minimum axis (argsort of the scales, general_utils.get_minimum_axis) and whether it was flipped towards the camera
    (flip_align_view) -- and the fp32 colours themselves (bit-identical to the in-kernel ones: tests/test_raw_gpu.py)."""
    with torch.no_grad():
        a = torch_activated(m, cam)
        column = torch.argsort(a["scales"], dim=-1)[:, 0]
        xyz = m.get_xyz
        d = xyz - cam.camera_center.repeat(xyz.shape[0], 1)
        _, keep = gm.flip_align_view(gm.get_minimum_axis(a["scales"], a["rotations"]), d / d.norm(dim=1, keepdim=True))
        sign = torch.where(keep[:, 0], 1.0, -1.0)
    return column.cpu(), sign.cpu(), a["normals"].cpu()


def view_normal_colours(rotations, column, sign):
    """``n = sign * build_rotation(rotations)[:, :, column]``, then ``n / |n| * 0.5 + 0.5``, differentiable in ``rotations`` (the
    normalised quaternions) in their own dtype; the decisions come from view_normal_decisions."""
    R = gm.build_rotation(rotations)
    n = torch.gather(R, 2, column[:, None, None].expand(-1, 3, 1)).squeeze(2) * sign.to(R.dtype)[:, None]
    return n / n.norm(dim=1, keepdim=True) * 0.5 + 0.5


def activated_kwargs(m, cam, bg):
    """The CPU oracle's arguments for one rasterizer call of the reference's structure, without its colours: the activated
    parameters as the model's getters produce them on this GPU (the same bits the fused kernels compute), the camera, ``bg``."""
    cpu = lambda t: t.detach().cpu()
    with torch.no_grad():
        act = dict(means3D=cpu(m.get_xyz), opacities=cpu(m.get_opacity), scales=cpu(m.get_scaling), rotations=cpu(m.get_rotation))
    return dict(act, bg=cpu(torch.as_tensor(bg)).numpy(), width=int(cam.image_width), height=int(cam.image_height),
                viewmatrix=cpu(cam.world_view_transform), projmatrix=cpu(cam.full_proj_transform), campos=cpu(cam.camera_center),
                tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, sh_degree=m.active_sh_degree)


def raw_oracles(m, cam, bg, dL_dcolor=None, dL_dalpha=None, dL_ddepth=None, dL_dnormal_img=None):
    """(reference fp32 sample, fp64 truth) of the gradients with respect to the six RAW tensors and ``viewspace_points``, given the
    per-pixel gradients of the colour [3,H,W], alpha [1,H,W] and depth [1,H,W] images (pass 1) and of the normal image [3,H,W]
    (pass 2); None = zeros, and without a normal gradient there is no second pass.  The CPU oracle differentiates each pass with
    respect to the activated parameters -- the fp32 tensors the model's getters produce on this GPU, the same bits the fused
    kernels compute; pass 2 has ``colors_precomp`` = the view-normal colours and no depth or alpha gradient -- and autograd carries
    the sum of both passes through the activations (gaussian_model.py:95-128) and pass 2's colour gradients through get_normal,
    in float32 for the reference's sample and in float64 for the truth.  Both passes see the same ``means2D`` (the reference
    hands the same tensor to both calls): ``viewspace_points`` gets the sum."""
    H, W = int(cam.image_height), int(cam.image_width)
    cpu = lambda t: t.detach().cpu()
    img = lambda t, c: np.zeros((c, H, W), np.float32) if t is None else \
        np.ascontiguousarray(cpu(torch.as_tensor(t)).reshape(c, H, W).numpy(), dtype=np.float32)
    base = activated_kwargs(m, cam, bg)
    with torch.no_grad():
        shs = cpu(m.get_features)
    passes = [dict(base, shs=shs, dL_dcolor=img(dL_dcolor, 3), dL_dalpha=img(dL_dalpha, 1), dL_ddepth=img(dL_ddepth, 1))]
    if dL_dnormal_img is not None:
        column, sign, colours = view_normal_decisions(m, cam)
        passes.append(dict(base, colors_precomp=colours, dL_dcolor=img(dL_dnormal_img, 3), dL_dalpha=img(None, 1), dL_ddepth=img(None, 1)))
    out = []
    for fn, dt in ((cpu_oracle.backward, torch.float32), (cpu_oracle.backward_f64, torch.float64)):
        grads = [fn(**kw) for kw in passes]
        up = lambda k, shape: sum(torch.as_tensor(np.asarray(g[k])).to(dt).reshape(shape) for g in grads)
        raw = {k: cpu(getattr(m, k)).to(dt).requires_grad_(True) for k in PARAMS}
        rot = torch.nn.functional.normalize(raw["_rotation"])
        acts = [raw["_xyz"], torch.exp(raw["_scaling"]), rot, torch.sigmoid(raw["_opacity"]),
                torch.cat((raw["_features_dc"], raw["_features_rest"]), dim=1)]
        ups = [up(k, a.shape) for k, a in zip(("dL_dmeans3D", "dL_dscales", "dL_drotations", "dL_dopacity"), acts)]
        ups.append(torch.as_tensor(np.asarray(grads[0]["dL_dsh"])).to(dt).reshape(acts[4].shape))
        if len(grads) == 2:
            acts.append(view_normal_colours(rot, column, sign))
            ups.append(torch.as_tensor(np.asarray(grads[1]["dL_dcolors"])).to(dt).reshape(acts[5].shape))
        g = torch.autograd.grad(acts, [raw[k] for k in PARAMS], ups, allow_unused=True)
        d = {k: (torch.zeros_like(raw[k]) if v is None else v).detach().numpy() for k, v in zip(PARAMS, g)}
        d["viewspace_points"] = up("dL_dmeans2D", grads[0]["dL_dmeans2D"].shape).numpy()
        out.append(d)
    return out


def compare(name, got, want):
    worst = {}
    for k, b in want.items():
        a = got[k]
        if b is None:
            assert a is None or float(a.abs().max()) == 0.0, f"{name}: {k} should carry no gradient"
            continue
        assert a is not None and a.shape == b.shape, f"{name}: {k} has no gradient (or the wrong shape)"
        if b.numel() == 0:
            continue
        scale, err = float(b.abs().max()), float((a - b).abs().max())
        worst[k] = err / max(scale, 1e-30)
        assert err <= REL * scale + ABS, f"{name}: {k} max abs err {err:.3e} vs scale {scale:.3e}"
    report_row("rawgrad:" + name, **worst)


def compare_with_truth(name, m, cam, bg, wts, keys, fused, unfused, mode):
    """Both paths against the truth for a loss over ``render`` (and ``depth``) with the weights ``wts``."""
    w = wts["render"]
    ref32, truth = raw_oracles(m, cam, bg, dL_dcolor=w[:3], dL_dalpha=w[3:4], dL_ddepth=wts["depth"] if "depth" in keys else None)
    for tag, got in (("fused", fused), ("structure", unfused)):
        got = {k: v.cpu().numpy() for k, v in got.items() if v is not None}
        assert_gradients_vs_truth(f"raw:{name}:{tag}:{mode}", got, ref32, truth, tuple(got))


UPSTREAM_KEYS = ("dL_dcolor", "dL_ddepth", "dL_dalpha", "dL_dnormal_img")


def record_upstreams(monkeypatch):
    """Wrap the binding's two backward entry points: every call appends what it was handed for the images -- ``("raw", colour,
    depth, alpha, normal)`` from the fused path's one call, ``("pass1" | "pass2", colour, depth, alpha)`` from the structure path's
    two (pass 2: the call whose ``colors_precomp`` are the view normals).  Returns the list."""
    from diff_gaussian_rasterization import _C
    seen = []
    keep = lambda t: None if t is None else t.detach().clone()
    raw_backward, backward = _C.rasterize_gaussians_raw_backward, _C.rasterize_gaussians_backward

    def raw_recorded(*a, **kw):
        seen.append(("raw",) + tuple(keep(t) for t in a[13:17]))
        return raw_backward(*a, **kw)

    def recorded(*a, **kw):
        seen.append(("pass2" if a[3].numel() else "pass1",) + tuple(keep(t) for t in a[12:15]))
        return backward(*a, **kw)

    monkeypatch.setattr(_C, "rasterize_gaussians_raw_backward", raw_recorded)
    monkeypatch.setattr(_C, "rasterize_gaussians_backward", recorded)
    return seen


def upstreams(seen, H, W):
    """The per-pixel gradients one ``render()`` backward handed to the binding (record_upstreams), as raw_oracles' keyword
    arguments: float32 arrays, zeros for an image of pass 1 that got none, None for the normal image if it got none."""
    got = dict.fromkeys(UPSTREAM_KEYS)
    kinds = [r[0] for r in seen]
    assert kinds in (["raw"], ["pass1"], ["pass2"], ["pass2", "pass1"], ["pass1", "pass2"]), kinds
    for kind, *images in seen:
        if kind == "pass2":
            assert images[1] is None and images[2] is None, "the normal pass's depth and alpha images reach no loss"
            got["dL_dnormal_img"] = images[0]
        else:
            got.update(zip(UPSTREAM_KEYS, images))
    arr = lambda t, c: np.zeros((c, H, W), np.float32) if t is None else t.cpu().numpy().reshape(c, H, W)
    return {"dL_dcolor": arr(got["dL_dcolor"], 3), "dL_ddepth": arr(got["dL_ddepth"], 1), "dL_dalpha": arr(got["dL_dalpha"], 1),
            "dL_dnormal_img": None if got["dL_dnormal_img"] is None else arr(got["dL_dnormal_img"], 3)}


def same_upstreams(a, b):
    return all((a[k] is None) == (b[k] is None) and (a[k] is None or np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)))
               for k in UPSTREAM_KEYS)


PATHS = (("fused", True), ("structure", False))


@pytest.mark.parametrize("keys", [("render",), ("render", "depth"), ("normal",), ("render", "depth", "normal", "pseudo_normal")])
def test_raw_autograd_matches_pytorch_autograd_through_the_reference_structure(keys, monkeypatch):
    """The losses AutoVFX trains with read ``render`` only (scene_representation.py:495-520); the others make sure every
    output the dictionary offers is differentiable with the right values: depth, the normal map (second per-pixel pass +
    chain through get_normal / build_rotation / F.normalize), pseudo normals (through depth).  Both paths are held to the truth
    in every mode of the library; the truth is fed the per-pixel gradients the binding received (the same bits in every mode,
    because the images are), so the PyTorch post-processing of the normal maps stays outside the bar."""
    from diff_gaussian_rasterization import _C
    cam = orbit_cameras(12, 256, 160)[7].to(DEV)
    bg = torch.tensor([0.2, 0.4, 0.1], device=DEV)
    m = leaves(raw_model(25_000, 101, nasty=False))
    wts = weights((160, 256), 3)
    seen = record_upstreams(monkeypatch)
    results = {}
    for mode in ("deterministic", "atomic", "slabs"):
        for path, raw_autograd in PATHS:
            seen.clear()
            out, grads = run(m, cam, bg, wts, raw_autograd, keys, mode=mode)
            if mode == "slabs":
                assert len(_C.last_layout()["slab_pairs"]) >= 2, "the slab mode should cut this scene into depth slabs"
            results[path, mode] = out, grads, upstreams(seen, 160, 256)
    fused_out, fused, _ = results["fused", "deterministic"]
    ref_out, ref, _ = results["structure", "deterministic"]
    for k in RENDER_KEYS:
        assert torch.equal(fused_out[k], ref_out[k]), f"forward {k} differs"
    compare("+".join(keys), fused, ref)
    if "render" in keys:
        assert float(fused["_features_rest"].abs().sum()) > 0 and float(fused["viewspace_points"].abs().sum()) > 0
    oracles = {}
    for (path, mode), (out, grads, ups) in results.items():
        for k in RENDER_KEYS:
            assert torch.equal(out[k], fused_out[k]), f"{path}:{mode}: forward {k} differs"
        assert same_upstreams(ups, results[path, "deterministic"][2]), f"{path}:{mode}: the binding got other per-pixel gradients"
        if path not in oracles:
            reuse = [o for p, o in oracles.items() if same_upstreams(ups, results[p, "deterministic"][2])]
            oracles[path] = reuse[0] if reuse else raw_oracles(m, cam, bg, **ups)
        ref32, truth = oracles[path]
        got = {k: v.cpu().numpy() for k, v in grads.items() if v is not None}
        assert_gradients_vs_truth(f"raw:{'+'.join(keys)}:{path}:{mode}", got, ref32, truth, tuple(got))


# ---- the binding itself: rasterize_gaussians_raw(want_normal=True) / rasterize_gaussians_raw_backward with seeded per-pixel
# gradients for all four images, every mode, the subsets of images a loss can leave without a gradient
UPSTREAM_SETS = {"all": ("dL_dcolor", "dL_ddepth", "dL_dalpha", "dL_dnormal_img"), "normal": ("dL_dnormal_img",),
                 "colour+normal": ("dL_dcolor", "dL_dnormal_img")}
GRAD_KEYS = PARAMS + ("viewspace_points",)


def binding_scene(scene):
    """(model, camera, background) of a binding case.  ``wide``: the scene of the render() test above, background showing behind
    the cloud (the second pass's background term is not zero); ``ragged``: an image of partial tiles, SH degree 1, white;
    ``heavy``: a trained-scene-like cloud (scenes.config_heavy, 200 k) as raw parameters -- log scales, opacity logits, the
    quaternions un-normalised -- at 960x540, where nearly every pixel saturates and stops early."""
    if scene == "wide":
        return raw_model(25_000, 101, nasty=False), orbit_cameras(12, 256, 160)[7].to(DEV), (0.2, 0.4, 0.1)
    if scene == "heavy":
        from autovfx_amd import scenes
        return raw_model(0, 5, cloud=scenes.config_heavy(P=200_000), nasty=False), orbit_cameras(200, 960, 540)[3].to(DEV), (0.2, 0.4, 0.1)
    return raw_model(6_000, 131, sh_degree=1, M=4, nasty=False), orbit_cameras(12, 131, 77)[4].to(DEV), (1.0, 1.0, 1.0)


def binding_upstreams(cam, upstream):
    g = pixel_grads(cam, 21)
    g["dL_dnormal_img"] = np.random.default_rng(22).standard_normal((3, cam.image_height, cam.image_width)).astype(np.float32)
    return {k: g[k] if k in UPSTREAM_SETS[upstream] else None for k in UPSTREAM_KEYS}


_BINDING_ORACLES = {}


def binding_oracles(key, m, cam, bg, ups):
    """raw_oracles of one (scene, upstream set), computed once for every mode and culling setting."""
    if key not in _BINDING_ORACLES:
        _BINDING_ORACLES.clear()
        _BINDING_ORACLES[key] = raw_oracles(m, cam, bg, **ups)
    return _BINDING_ORACLES[key]


def binding_run(m, cam, bg, ups, mode, cull):
    """One forward (a full call; with "slabs" an inference call in small depth slabs) and its raw backward, the way _RasterizeRaw
    makes them, with the forward's decoded scratch."""
    from diff_gaussian_rasterization import _C
    H, W, P = int(cam.image_height), int(cam.image_width), int(m._xyz.shape[0])
    set_mode(mode)
    _lib.set_option(_lib.OPT_TILE_CULL, 1 if cull else 0)
    try:
        n, color, depth, alpha, radii, geom, binning, image, normal = call_raw(m, cam, bg, inference=mode == "slabs")
        torch.cuda.synchronize()
        lay = _C.last_layout()
        fwd = {"slab_pairs": lay["slab_pairs"]} if mode == "slabs" else decode_scratch(lay, geom, binning, image, P, W, H)
        t = lambda k: None if ups[k] is None else torch.from_numpy(ups[k]).to(DEV)
        g2d, gxyz, gls, grot, gop, gdc, grest = _C.rasterize_gaussians_raw_backward(
            bg, m._xyz, m._scaling, m._rotation, m._opacity, m._features_dc, m._features_rest, radii, 1.0, cam.world_view_transform,
            cam.full_proj_transform, cam.tanfovx, cam.tanfovy, t("dL_dcolor"), t("dL_ddepth"), t("dL_dalpha"), t("dL_dnormal_img"),
            m.active_sh_degree, cam.camera_center, geom, n, binning, image, alpha, False)
        torch.cuda.synchronize()
    finally:
        restore_options()
    grads = dict(zip(GRAD_KEYS, (gxyz, gls, grot, gop, gdc, grest, g2d)))
    hip = {"color": color, "depth": depth, "alpha": alpha, "normal": normal, "radii": radii, **grads}
    hip = {k: v.cpu().numpy() for k, v in hip.items()}
    hip.update(fwd=fwd, cull=cull, mode=mode)
    return hip


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("upstream", list(UPSTREAM_SETS))
@pytest.mark.parametrize("scene,cull", [("wide", True), ("ragged", True), ("ragged", False), ("heavy", True)])
def test_binding_backward_with_the_normal_pass_matches_the_truth(scene, cull, upstream, mode):
    """gsr_backward_raw with dL_dpix_normal: the second per-pixel pass (colour sums to accumulator slots 10 - 12, geometry sums
    added to 4 - 9; in deterministic mode its own records) and the chain of slots 10 - 12 through get_normal to the quaternion.
    Forward state first -- radii bit-exact, the colour / depth / alpha images and the normal image within the forward tolerance
    of the CPU oracle (whose normal image is a pass with colors_precomp = the view-normal colours) -- then every raw gradient and
    means2D's against the two-pass truth (``heavy``: on a saturated scene).  A missing image gradient (None) drops its terms: pass 1 runs with a zero colour
    gradient for "normal", without its depth and alpha terms for "normal" and "colour+normal"."""
    from test_parity_gpu import FLIP_PPM, RGB_TOL
    m, cam, bg = binding_scene(scene)
    bg_t = torch.tensor(bg, device=DEV)
    ups = binding_upstreams(cam, upstream)
    ref32, truth = binding_oracles((scene, upstream), m, cam, bg_t, ups)
    name = f"rawbind:{scene}:{upstream}:{'cull' if cull else 'nocull'}:{mode}"
    hip = binding_run(m, cam, bg_t, ups, mode, cull)
    kw = activated_kwargs(m, cam, bg_t)
    fref = cpu_oracle.forward(intermediates=True, shs=m.get_features.detach().cpu(), **kw)
    assert_forward_state(name, hip, fref)
    nref = cpu_oracle.forward(colors_precomp=view_normal_decisions(m, cam)[2], **kw)
    err = np.abs(hip["normal"].astype(np.float64) - nref["color"].astype(np.float64))
    bad = int((err > RGB_TOL).sum())
    assert bad <= int(np.ceil(FLIP_PPM * 1e-6 * fref["alpha"].size)), f"{name}: normal image off on {bad} px (max {err.max():.3e})"
    if scene == "heavy":   # the opposite property: the walks start inside the lists and the stop decides what is differentiated
        assert float((hip["alpha"] > 0.999).mean()) >= 0.95, f"{name}: the heavy scene should saturate"
    else:
        assert float(hip["alpha"].min()) < 0.5, f"{name}: the background should show: the second pass's background term is tested"
    if mode == "slabs":
        assert len(hip["fwd"]["slab_pairs"]) >= 2, f"{name}: the slab mode should cut this scene into depth slabs"
    assert_gradients_vs_truth(name, hip, ref32, truth, GRAD_KEYS)
    if mode == "deterministic":
        assert_same_bits(name, hip, binding_run(m, cam, bg_t, ups, mode, cull), GRAD_KEYS)


def test_raw_autograd_with_degenerate_parameters():
    """Tied scales, near-zero and huge quaternions, saturated opacity logits (the `nasty` cases of tests/test_raw_gpu.py):
    gradients through the clamp of F.normalize, sigmoid's flat ends and the argmin's tie rule still match autograd.  This case
    stays a comparison of the two paths in deterministic mode: its ill-conditioning is in the activations' chain (1 / |q| of
    1e4 and more), and cpu_oracle.fp32_noise, a yardstick for the rasterizer's per-Gaussian sums, does not bound that chain."""
    cam = orbit_cameras(12, 208, 120)[2].to(DEV)
    bg = torch.zeros(3, device=DEV)
    m = leaves(raw_model(12_000, 202, nasty=True))
    wts = weights((120, 208), 9)
    keys = ("render", "normal")
    fused_out, fused = run(m, cam, bg, wts, True, keys)
    ref_out, ref = run(m, cam, bg, wts, False, keys)
    for k in RENDER_KEYS:
        assert torch.equal(fused_out[k], ref_out[k]), f"forward {k} differs"
    compare("nasty", fused, ref)


@pytest.mark.parametrize("degree,M", [(0, 1), (1, 4), (2, 9), (3, 16)])
def test_raw_autograd_sh_layouts(degree, M):
    """_features_rest of every width the reference's models carry ([P,0,3] ... [P,15,3]): the two halves of dL_dsh land in
    the right tensors (LDS-staged store for M = 16, direct stores otherwise)."""
    cam = orbit_cameras(12, 160, 96)[degree].to(DEV)
    bg = torch.tensor([0.5, 0.5, 0.5], device=DEV)
    m = leaves(raw_model(6_000, 300 + degree, sh_degree=degree, M=M, nasty=False))
    wts = weights((96, 160), degree)
    _, fused = run(m, cam, bg, wts, True, ("render",))
    _, ref = run(m, cam, bg, wts, False, ("render",))
    compare(f"sh{degree}", fused, ref)
    assert fused["_features_rest"].shape == (6_000, M - 1, 3) and fused["_features_dc"].shape == (6_000, 1, 3)


def test_training_loop_through_render_lowers_the_loss():
    """A few Adam steps on the raw tensors through render(), as training_3DGS_for_inpainting does: the loss goes down and the
    result equals the same loop run through the reference structure to within optimisation noise."""
    cam = orbit_cameras(12, 192, 120)[4].to(DEV)
    bg = torch.zeros(3, device=DEV)
    target = torch.rand(4, 120, 192, device=DEV)

    def loop(raw_autograd):
        m = leaves(raw_model(8_000, 404, nasty=False))
        opt = torch.optim.Adam([getattr(m, k) for k in PARAMS], lr=5e-3)
        saved = renderer.RAW_AUTOGRAD
        renderer.RAW_AUTOGRAD = raw_autograd
        losses = []
        try:
            for _ in range(10):
                out = renderer.render(cam, m, renderer.PipelineParams, bg)
                loss = (out["render"] - target).abs().mean()
                opt.zero_grad(set_to_none=True)
                loss.backward()
                opt.step()
                losses.append(float(loss.detach()))
        finally:
            renderer.RAW_AUTOGRAD = saved
        return losses

    a, b = loop(True), loop(False)
    assert a[-1] < a[0] and abs(a[-1] - b[-1]) < 2e-3 * abs(b[0]), (a, b)


def test_c3_full_size_iteration_gradients():
    """BASELINE configs[2] at full size: one training-style iteration through render(), fused raw path against the reference
    structure."""
    from autovfx_amd import scenes
    cam = orbit_cameras(800, 1920, 1080)[400].to(DEV)
    bg = torch.zeros(3, device=DEV)
    m = leaves(raw_model(0, 2, cloud=scenes.config_c3(), nasty=False))
    wts = {"render": torch.randn(4, 1080, 1920, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)) / (1080 * 1920)}
    fused_out, fused = run(m, cam, bg, wts, True, ("render",))
    ref_out, ref = run(m, cam, bg, wts, False, ("render",))
    for k in ("render", "depth", "radii"):
        assert torch.equal(fused_out[k], ref_out[k]), k
    compare("c3_full", fused, ref)
    compare_with_truth("c3_full", m, cam, bg, wts, ("render",), fused, ref, "deterministic")
    _, again = run(m, cam, bg, wts, True, ("render",))
    for k, v in fused.items():   # GSR_OPT_BACKWARD_DETERMINISTIC at BASELINE configs[2]: the same bits twice
        assert v is None or torch.equal(v, again[k]), f"{k}: two deterministic runs differ"
    # the default mode: float atomics, and (GSR_OPT_GRAD_SLABS) the forward an inference call in two depth slabs whose segments the
    # backward walks -- same images bit for bit, gradients against the same truth
    slab_out, slab_fused = run(m, cam, bg, wts, True, ("render",), mode="default")
    from diff_gaussian_rasterization import _C
    assert len(_C.last_layout()["slab_pairs"]) == 2, "C3 in grad mode should be cut into two depth slabs"
    for k in ("render", "depth", "radii"):
        assert torch.equal(slab_out[k], ref_out[k]), k
    _, slab_ref = run(m, cam, bg, wts, False, ("render",), mode="default")
    compare_with_truth("c3_full", m, cam, bg, wts, ("render",), slab_fused, slab_ref, "atomic+slabs")
