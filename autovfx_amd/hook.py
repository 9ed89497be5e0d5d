"""``autovfx_amd.install()``: put the MI355X render path behind an UNCHANGED AutoVFX process.

AutoVFX reaches the rasterizer through two imports (paths under the reference tree):

* ``from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer``
  (``sugar/gaussian_splatting/gaussian_renderer/__init__.py:16``, ``sugar/sugar_scene/sugar_model.py:9``) -- served by the
  ``diff_gaussian_rasterization`` package at the root of this repository once that root is on ``sys.path``;
* ``from sugar.gaussian_splatting.gaussian_renderer import render`` (``scene_representation.py:24``,
  ``extract/extract_object.py:14``; ``from gaussian_renderer import render`` in ``sugar/gaussian_splatting/train.py:16`` /
  ``render.py:17``; ``from gaussian_splatting.gaussian_renderer import render as gs_render`` in
  ``sugar/sugar_scene/gs_model.py:7``) -- the per-frame function, whose PyTorch preparation costs more than the rasterizer.

``install()`` makes both resolve here:

1. the repository root goes to the front of ``sys.path`` (so ``diff_gaussian_rasterization`` is this one);
2. a module named ``...blend_all`` (``blender/blend_all.py``, imported at ``scene_representation.py:13``) gets its ``blend_frames``
   replaced by ``autovfx_amd.compositor.blend_frames`` (same arguments, same files in and out; PIL's resizes and the per-pixel
   composite run on the GPU);
3. a module named ``...scene_representation`` gets ``SceneRepresentation.render_from_3DGS`` (the frame loop, ``:337-447``) replaced
   by ``autovfx_amd.frame_loop.render_from_3DGS``: same arguments and files; inserted objects are loaded once instead of once per
   frame, several frames are in flight, the four files of a frame are built on the GPU;
4. a module named ``...sugar_model`` gets ``SuGaR.render_image_gaussian_rasterizer`` (two rasterizer calls over the same geometry) run with
   the binding's geometry reuse switched on for its duration: the second call costs one blend launch, same bits;
5. a module named ``...render_panorama`` (``sugar/gaussian_splatting/render_panorama.py``) gets its ``render_panorama`` replaced by
   ``autovfx_amd.panorama.render_panorama`` (same arguments, files and return value; the six faces in flight, the cube-to-equirect
   resample and the PNG files on the GPU);
6. every module named ``...gaussian_renderer`` gets its ``render`` replaced by ``autovfx_amd.renderer.render`` (same signature, same
   result dictionary), and every already-imported module that holds the original function under any name
   (``from ... import render [as gs_render]``) is rebound too;
7. a module named ``...loss_utils`` that defines ``ssim``, ``_ssim`` and ``create_window`` (``utils/loss_utils.py``, its SuGaR copy
   ``sugar_utils/loss_utils.py``) gets its ``ssim`` replaced by ``autovfx_amd.ssim.drop_in(<the original>)``: the fused HIP
   forward and backward where they apply, the original for every other call; already-imported modules holding it under any name
   (``train.py``, ``metrics.py``, the SuGaR trainers, ``scene_representation``) are rebound;
8. a module named ``...gaussian_model`` whose ``GaussianModel`` defines both ``training_setup`` and ``replace_tensor_to_optimizer``
   (the reference's ``scene/gaussian_model.py``, used by ``train.py`` and the inpainting re-train; not this package's
   ``autovfx_amd.gaussian_model``) gets ``training_setup`` wrapped: after the original built ``self.optimizer``, a plain
   ``torch.optim.Adam`` is replaced by ``autovfx_amd.optim.Adam`` over the same parameter groups and defaults (one HIP launch per
   step, torch's bits; the state is still empty there, so ``restore()`` loads into it as before); torch and the library are
   imported at the first call, not at patch time;
9. the same class, when it also defines ``densification_postfix``, ``prune_points`` and ``cat_tensors_to_optimizer``, gets
   ``add_densification_stats`` (``:415-417``, every iteration) and ``densify_and_prune`` (``:399-413``) replaced by
   ``autovfx_amd.densify``'s: one HIP launch for the statistics, and a plan, one host read of three counts and one launch that writes
   the six new parameters and twelve new moments instead of four rewrites of the model -- the reference's values, order, generator
   state and optimizer surgery bit for bit; a call the kernels do not take exactly (a CPU model, ``max_grad <= 0``, other layouts)
   runs ``GaussianModel.reference_<name>``.  The inline ``max_radii2D`` line of the loops cannot be reached by a hook and stays.
   torch and the library are imported at the first call.

10. a module named ``...knn`` that defines ``knn_points`` and ``knn_gather`` (``pytorch3d/ops/knn.py``; this repository ships no
    ``pytorch3d``) gets its ``knn_points`` replaced by ``autovfx_amd.knn.drop_in(<the original>)``: the HIP search for CUDA float32
    ``[N, P, 3]`` calls with ``K <= 16`` (SuGaR's neighbour searches, ``sugar_model.py:233``, ``:899``, ``:914``, ``:1213``, gradients
    included), the original for every other call (the 2-D one of ``sugar_extractors/refined_mesh.py:147``); ``pytorch3d.ops.knn_points``
    and every module that did ``from pytorch3d.ops import knn_points`` are rebound.

11. the same ``...sugar_model`` module, when its ``SuGaR`` defines ``compute_density``, ``get_field_values``, ``get_beta`` and
    ``get_covariance``, gets the first two (``sugar_model.py:1216-1239``, ``:1118-1187``: the density field of the regulariser, 1 M samples
    x 16 neighbours per iteration, and of the mesh extraction) replaced by ``autovfx_amd.field``'s drop-ins: inputs built as the
    reference builds them, the gather / 3x3 product / ``exp`` / sum over the neighbours and their backward in two HIP kernels, what
    follows the sum in the reference's arithmetic; ``return_sdf_grad=True``, CPU tensors and other dtypes run
    ``SuGaR.reference_<name>``.  torch and the library are imported at the first call.

12. the same class, when it defines ``get_covariance`` and ``compute_density``, gets ``compute_level_surface_points_from_camera_fast``
    (``sugar_model.py:1719-1954``, once per training camera in ``sugar_extractors/coarse_mesh.py``) replaced by ``autovfx_amd.levelset``'s
    drop-in: the depth render, the unprojection and the neighbour lists as the reference builds them, then the 21-sample ray march, the
    crossings of every level and the normals in one HIP kernel; the flat-Gaussian variants, ``just_use_depth_as_level``, ``use_gaussian_depth``, a CPU model,
    more than 32 samples, 8 levels or 64 neighbours run ``SuGaR.reference_compute_level_surface_points_from_camera_fast``, decided
    before ``torch.randperm`` is consumed.  torch and the library are imported at the first call.

13. a module named ``..._C`` that defines both ``rasterize_meshes`` and ``rasterize_meshes_backward`` (``pytorch3d._C``; this repository
    ships no ``pytorch3d``, and its own ``diff_gaussian_rasterization._C`` and ``simple_knn._C`` define neither) gets its
    ``rasterize_meshes`` replaced by ``autovfx_amd.meshraster.drop_in(<the original>)``: the HIP z-buffer for CUDA float32 faces at
    ``blur_radius == 0`` with up to 16 faces per pixel that need no gradient (the ``MeshRasterizer`` of SuGaR's mesh extraction,
    ``sugar_extractors/coarse_mesh.py:216-227``, ``sugar_model.py:1341``, ``:1568``, ``:1798``, ``:2541-2598``, ``metrics.py:283-290``), the
    original for every other call.  pytorch3d's Python looks the operator up on ``_C`` at every call, so nothing is rebound, and its
    ``clip_faces``, bin heuristics and ``convert_clipped_rasterization_to_original_faces`` run as they are.  The leaf name makes
    the hook's loader wrapper pass every ``*._C`` imported after ``install()`` through (``torch._C`` among them): it delegates to the real
    loader and the ``needs`` keep the patch off (tests/test_meshraster.py loads ``torch._C`` that way; other packages' ``_C`` are not tested).

14. the same ``..._C`` module, when it defines both ``face_areas_normals_forward`` and ``face_areas_normals_backward``, gets the pair replaced
    by ``autovfx_amd.meshattrs.drop_in_face_areas_normals_forward`` / ``_backward(<the original>)``: the HIP kernels for CUDA float32
    ``[V, 3]`` vertices with int64 ``[F, 3]`` faces on one device (``Meshes.faces_normals_packed()`` under ``SuGaR.quaternions``,
    ``sugar_model.py:425-452``, several times per iteration of ``sugar_trainers/refine.py`` and differentiated into the vertices;
    ``SuGaR.get_normals``, ``:835``; ``sugar_extractors/refined_mesh.py:134``), the originals for every other call.  pytorch3d's
    ``_MeshFaceAreasNormals`` stays as it is: it looks both operators up on ``_C`` at call time.

15. the same module, when it defines both ``interpolate_face_attributes_forward`` and ``interpolate_face_attributes_backward``, gets that
    pair replaced by ``autovfx_amd.meshattrs.drop_in_interpolate_face_attributes_forward`` / ``_backward(<the original>)``: the HIP
    kernels for int64 fragments (``[P]``, as pytorch3d's Python flattens them, or ``[N, H, W, K]``) with CUDA float32 barycentrics and ``[F, 3, D]`` attributes (every shader and
    ``TexturesUV.sample_textures``: the texture extraction, ``refined_mesh.py:194-197``, ``sugar_model.py:2595-2596``;
    ``metrics.py:274-290``), the originals for every other call.  A ``_C`` with only one operator of a pair keeps that pair.

16. a module named ``...mesh_normal_consistency`` that defines ``mesh_normal_consistency`` (``pytorch3d/loss/mesh_normal_consistency.py``)
    gets that function replaced by ``autovfx_amd.meshloss.drop_in(<the original>)``: the fused HIP loss and its backward for one CUDA
    float32 mesh with int64 faces (``sugar_trainers/refine.py:829-830``, every iteration of the refinement), the original for every
    other call (batches, CPU meshes, an empty mesh).  The module is patched right after its body ran, so ``pytorch3d.loss``'s own
    ``from .mesh_normal_consistency import mesh_normal_consistency`` already binds the replacement; when ``install()`` runs after the
    import, ``pytorch3d.loss`` and every module that did ``from pytorch3d.loss import mesh_normal_consistency`` are rebound.

17. the same ``...sugar_model`` module, when it defines both ``extract_texture_image_and_uv_from_gaussians`` and ``SuGaR``, gets that function
    (``sugar_model.py:2398-2614``, the last step before the textured ``.obj``) replaced by ``autovfx_amd.texture.drop_in(<the original>)``:
    the UV atlas with the reference's values, the initial fill in one HIP pass, and per training camera the reference's render and
    ``MeshRasterizer`` followed by two HIP launches on the fragments -- no shader, no index map, no ``nonzero``; ``texture_with_gaussian_renders=False``,
    a CPU model, ``square_size`` outside 4..32, more than 8 Gaussians per triangle and calls under autograd run the original.
    ``sugar_extractors/refined_mesh.py:9`` imports the function by name, so modules that already hold it are rebound.

18. the same ``SuGaR`` class, when it has ``surface_mesh`` and ``get_covariance``, gets the getters of its properties ``points``,
    ``scaling`` and ``quaternions`` (``sugar_model.py:376-391``, ``:408-423``, ``:425-452``: each read once per
    ``render_image_gaussian_rasterizer`` call of the refinement and differentiated into the vertices, ``_scales`` and ``_quaternions``)
    replaced by ``autovfx_amd.bound.drop_in_points`` / ``_scaling`` / ``_quaternions(<the original getter>)``: for a model bound to a
    surface mesh, one fused HIP launch per access with only that output wanted, one more for its backward, no host synchronisation
    (the reference's ``matrix_to_quaternion`` ends in a ``nonzero``); an unbound model, ``editable=True``, a ``scale_activation`` that is not
    ``torch.exp``, a CPU model, other dtypes and graph capture run the original getter.  The target is a ``property``: it is replaced by
    ``property(<ours>, original.fset, original.fdel)``, and ``SuGaR.reference_<name>`` is the original property.  torch and the library
    are imported at the first access.  The geometry-reuse wrapper of item 4 is unaffected.

Items 2-18 are the rows of ``_TARGETS``, applied by ``_patch`` to every matching module, whether it was imported before
``install()`` or after (a ``sys.meta_path`` hook).  Each replaced attribute keeps the reference's original next to it as
``reference_<attr>`` on the module or class (``<module>.reference_render``, ``SceneRepresentation.reference_render_from_3DGS``, ...).
``uninstall()`` undoes every patch in reverse.

Nothing else of the reference is touched: the rest of its ``GaussianModel``, cameras, scene editing and I/O run as they are.  With
autograd off, ``render`` reads the model's six raw parameter tensors and activates them inside the HIP kernels
(``gsr_forward_raw``); with autograd on it keeps the reference's structure (PyTorch activations, two rasterizer calls).

Opt-in without touching AutoVFX's sources: put ``<repo>/integration`` and ``<repo>`` on ``PYTHONPATH`` and set
``AUTOVFX_AMD_INSTALL=1``; ``integration/sitecustomize.py`` then calls ``install()`` at interpreter start (the hook itself
imports neither torch nor the HIP library until a target module is actually imported).
"""
from __future__ import annotations

import functools
import importlib.abc
import os
import sys
import types
from typing import Callable, List, NamedTuple, Optional, Tuple

_REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_installed: Optional["_RendererHook"] = None
patched_modules: List[str] = []          # names of the modules patched by items 2-7 and 10-18 (introspection / tests)
patched_models: List[str] = []           # names of the modules whose ``GaussianModel.training_setup`` was wrapped (item 8)
_strict = True                           # install(strict=...): may a failure to load the render path break the importing process?
_gave_up = False                         # lenient mode: a replacement could not be loaded once; patch nothing more
_undo: List[tuple] = []                  # (owner, attr, original, replacement, importer slots rebound), one per patch, in order


def _load(module: str, name: str):
    """``from .<module> import <name>`` (the same ``__import__`` call): imports torch and loads libgsr_hip.so, so it only runs
    once a target module really appears."""
    return getattr(__import__(module, globals(), None, (name,), 1), name)


def _mark(fn: Callable) -> Callable:
    """A replacement built around one original: it is "already ours" at the next ``install()``, and ``uninstall()`` gives every
    holder of it the original back (it can only have come from that one patch)."""
    fn._autovfx_amd_wrapped = True
    return fn


def _could_not_load(what: str, e: Exception) -> None:
    """Strict: ``e`` surfaces where the module was imported.  Lenient (the start-up hook, integration/sitecustomize.py, promised
    never to break the process): one stderr line, the reference's code stays, nothing is patched again in this process.  That is
    not a quiet fallback for rendering -- the reference's render() imports ``diff_gaussian_rasterization``, which is this
    repository's package and raises when the HIP library cannot be loaded -- it only lets a process that imports the module
    without ever rendering (a data-preparation helper on a machine without a GPU) live."""
    global _gave_up
    if _strict:
        raise e
    _gave_up = True
    sys.stderr.write(f"[autovfx_amd] {what} could not be loaded ({e!r}); not retried in this process\n")


def _with_geometry_reuse(original: Callable) -> Callable:
    """``SuGaR.render_image_gaussian_rasterizer`` (sugar/sugar_scene/sugar_model.py:1960-2230, BASELINE configs[3]) rasterizes the same
    geometry twice -- colours at :2141, the per-Gaussian normals as colours at :2174 -- with nothing in between that writes to the
    positions, scales, rotations or the camera.  The method itself stays the reference's; it is merely run with the binding's
    geometry reuse switched ON for its duration (``diff_gaussian_rasterization._C.set_geometry_cache``: off by default because a
    write that bypasses PyTorch's version counters between two calls would be invisible to it -- here the code between the two calls
    is known): the second call then blends its colours over the first call's lists, one launch instead of a whole pipeline, same
    bits."""
    @functools.wraps(original)
    def render_image_gaussian_rasterizer(self, *args, **kwargs):
        from diff_gaussian_rasterization import _C
        before = _C.geometry_cache_enabled()
        _C.set_geometry_cache(True)
        try:
            return original(self, *args, **kwargs)
        finally:
            _C.set_geometry_cache(before)

    return _mark(render_image_gaussian_rasterizer)


def _with_fused_adam(original: Callable) -> Callable:
    """``GaussianModel.training_setup`` (gaussian_model.py:159-177) runs as it is, then a plain ``torch.optim.Adam`` in
    ``self.optimizer`` becomes autovfx_amd.optim.Adam over the same groups."""
    @functools.wraps(original)
    def training_setup(self, *args, **kwargs):
        out = original(self, *args, **kwargs)
        if _gave_up:
            return out
        try:
            from .optim import from_torch_adam   # imports torch and loads libgsr_hip.so: at the first call, not at patch time
        except Exception as e:
            _could_not_load(f"{original.__module__}.{original.__qualname__} keeps torch's Adam: the fused step", e)
            return out
        self.optimizer = from_torch_adam(self.optimizer)
        return out

    return _mark(training_setup)


def _with_hip_densify(name: str) -> Callable:
    """make() for ``GaussianModel.add_densification_stats`` / ``densify_and_prune``: the method of that name in autovfx_amd.densify,
    imported (torch, libgsr_hip.so) at the first call; it runs ``reference_<name>`` itself for the calls its kernels do not take."""
    def make(original: Callable) -> Callable:
        @functools.wraps(original)
        def method(self, *args, **kwargs):
            if _gave_up:
                return original(self, *args, **kwargs)
            try:
                ours = _load("densify", name)
            except Exception as e:
                _could_not_load(f"{original.__module__}.{original.__qualname__} left as the reference's: the HIP densification", e)
                return original(self, *args, **kwargs)
            return ours(self, *args, **kwargs)

        return _mark(method)

    return make


def _with_hip_sugar_method(name: str, module: str = "field", what: str = "the HIP density field") -> Callable:
    """make() for a ``SuGaR`` method or property getter with a drop-in of its own (``compute_density`` / ``get_field_values`` in ``field``,
    ``compute_level_surface_points_from_camera_fast`` in ``levelset``, ``points`` / ``scaling`` / ``quaternions`` in ``bound``): ``autovfx_amd.<module>.drop_in_<name>(original)``, built (torch, libgsr_hip.so) at the first call; it runs ``original`` itself for
    the calls its kernels do not take."""
    def make(original: Callable) -> Callable:
        built = []

        @functools.wraps(original)
        def method(self, *args, **kwargs):
            if not built:
                if _gave_up:
                    return original(self, *args, **kwargs)
                try:
                    built.append(_load(module, "drop_in_" + name)(original))
                except Exception as e:
                    _could_not_load(f"{original.__module__}.{original.__qualname__} left as the reference's: {what}", e)
                    return original(self, *args, **kwargs)
            return built[0](self, *args, **kwargs)

        return _mark(method)

    return make


def _with_mesh_attrs(name: str) -> Callable:
    """make() for one operator of ``pytorch3d._C`` that ``autovfx_amd.meshattrs`` replaces: ``drop_in_<name>(original)``, built (torch,
    libgsr_hip.so) when the patch is made, like the mesh rasterizer's."""
    return lambda original: _mark(_load("meshattrs", "drop_in_" + name)(original))


class _Target(NamedTuple):
    leaf: str                            # the last component of the module's name
    cls: Optional[str]                   # the class in the module that owns ``attr``; None: the module itself
    attr: str                            # what is replaced (a property: its getter); the original stays as ``reference_<attr>`` on the owner
    make: Callable                       # make(original) -> the replacement; raises when torch or the library cannot be loaded
    what: str                            # the lenient stderr line: "<module>.<attr> left as the reference's: <what> could not be loaded"
    needs: Tuple[str, ...] = ()          # names that must all be callable, or properties, in the owner's own namespace
    rebind: bool = False                 # also rebind already-imported modules that hold the original
    record: List[str] = patched_modules


_TARGETS = (
    # item 2: blender/blend_all.py, its blend_frames() is called at scene_representation.py:232
    _Target("blend_all", None, "blend_frames", lambda original: _load("compositor", "blend_frames"), "the GPU compositor"),
    # item 3: scene_representation.py, SceneRepresentation.render_from_3DGS is the frame loop (:337-447)
    _Target("scene_representation", "SceneRepresentation", "render_from_3DGS", lambda original: _load("frame_loop", "render_from_3DGS"),
            "the frame loop"),
    # item 4: sugar/sugar_scene/sugar_model.py, SuGaR.render_image_gaussian_rasterizer calls the rasterizer twice (:2141,2174)
    _Target("sugar_model", "SuGaR", "render_image_gaussian_rasterizer", _with_geometry_reuse, "the geometry reuse"),
    # item 5: sugar/gaussian_splatting/render_panorama.py, render_panorama() (:100-145), imported directly by its users
    _Target("render_panorama", None, "render_panorama", lambda original: _load("panorama", "render_panorama"), "the panorama path"),
    # item 6: the per-frame render() of every caller
    _Target("gaussian_renderer", None, "render", lambda original: _load("renderer", "render"), "the MI355X render path", rebind=True),
    # item 7: utils/loss_utils.py, sugar_utils/loss_utils.py, ssim() (:33-62) of every training loop's loss
    _Target("loss_utils", None, "ssim", lambda original: _mark(_load("ssim", "drop_in")(original)), "the fused SSIM",
            needs=("ssim", "_ssim", "create_window"), rebind=True),
    # item 8: scene/gaussian_model.py, GaussianModel.training_setup builds the training loops' Adam (:159-177)
    _Target("gaussian_model", "GaussianModel", "training_setup", _with_fused_adam, "the fused Adam step",
            needs=("training_setup", "replace_tensor_to_optimizer"), record=patched_models),
    # item 9: the same class's densification (:399-417), rewritten around the optimizer surgery it must reproduce
    _Target("gaussian_model", "GaussianModel", "add_densification_stats", _with_hip_densify("add_densification_stats"),
            "the HIP densification", needs=("densification_postfix", "prune_points", "cat_tensors_to_optimizer"), record=patched_models),
    _Target("gaussian_model", "GaussianModel", "densify_and_prune", _with_hip_densify("densify_and_prune"), "the HIP densification",
            needs=("densification_postfix", "prune_points", "cat_tensors_to_optimizer"), record=patched_models),
    # item 10: pytorch3d/ops/knn.py, knn_points() of SuGaR's neighbour searches (sugar_model.py:233, :899, :914, :1213)
    _Target("knn", None, "knn_points", lambda original: _mark(_load("knn", "drop_in")(original)), "the HIP k-nearest-neighbour search",
            needs=("knn_points", "knn_gather"), rebind=True),
    # item 11: sugar/sugar_scene/sugar_model.py, SuGaR's density field (:1118-1187, :1216-1239)
    _Target("sugar_model", "SuGaR", "compute_density", _with_hip_sugar_method("compute_density"), "the HIP density field",
            needs=("compute_density", "get_field_values", "get_beta", "get_covariance")),
    _Target("sugar_model", "SuGaR", "get_field_values", _with_hip_sugar_method("get_field_values"), "the HIP density field",
            needs=("compute_density", "get_field_values", "get_beta", "get_covariance")),
    # item 12: the same class's ray march of the coarse mesh extraction (:1719-1954)
    _Target("sugar_model", "SuGaR", "compute_level_surface_points_from_camera_fast",
            _with_hip_sugar_method("compute_level_surface_points_from_camera_fast", "levelset", "the HIP level-surface ray march"),
            "the HIP level-surface ray march", needs=("get_covariance", "compute_density")),
    # item 13: pytorch3d/_C, rasterize_meshes() under every MeshRasterizer (sugar_extractors/coarse_mesh.py:216-227); looked up at call time
    _Target("_C", None, "rasterize_meshes", lambda original: _mark(_load("meshraster", "drop_in")(original)), "the HIP mesh rasterizer",
            needs=("rasterize_meshes", "rasterize_meshes_backward")),
    # item 14: pytorch3d/_C, the pair under Meshes.faces_normals_packed() (SuGaR.quaternions, sugar_model.py:425-452)
    *(_Target("_C", None, name, _with_mesh_attrs(name), "the HIP face areas and normals",
              needs=("face_areas_normals_forward", "face_areas_normals_backward"))
      for name in ("face_areas_normals_forward", "face_areas_normals_backward")),
    # item 15: pytorch3d/_C, the pair under every shader and texture sampler (refined_mesh.py:194-197, metrics.py:274-290)
    *(_Target("_C", None, name, _with_mesh_attrs(name), "the HIP face-attribute interpolation",
              needs=("interpolate_face_attributes_forward", "interpolate_face_attributes_backward"))
      for name in ("interpolate_face_attributes_forward", "interpolate_face_attributes_backward")),
    # item 16: pytorch3d/loss/mesh_normal_consistency.py, the regulariser of sugar_trainers/refine.py:829-830
    _Target("mesh_normal_consistency", None, "mesh_normal_consistency", lambda original: _mark(_load("meshloss", "drop_in")(original)),
            "the HIP mesh normal consistency loss", needs=("mesh_normal_consistency",), rebind=True),
    # item 17: sugar/sugar_scene/sugar_model.py, the texture of the refined mesh (:2398-2614), imported by name at refined_mesh.py:9
    _Target("sugar_model", None, "extract_texture_image_and_uv_from_gaussians", lambda original: _mark(_load("texture", "drop_in")(original)),
            "the HIP texture bake", needs=("extract_texture_image_and_uv_from_gaussians", "SuGaR"), rebind=True),
    # item 18: the same class's properties that turn the bound surface mesh into Gaussians (:376-391, :408-423, :425-452)
    *(_Target("sugar_model", "SuGaR", name, _with_hip_sugar_method(name, "bound", "the HIP bound Gaussians"), "the HIP bound Gaussians",
              needs=("surface_mesh", "get_covariance"))
      for name in ("points", "scaling", "quaternions")),
)


def _target(name: str) -> Tuple[_Target, ...]:
    """The rows for a module of that name; this package's own modules (``autovfx_amd.gaussian_model``) are never targets."""
    if name.startswith("autovfx_amd."):
        return ()
    return tuple(t for t in _TARGETS if name == t.leaf or name.endswith("." + t.leaf))


def _is_ours(value) -> bool:
    return getattr(value, "_autovfx_amd_wrapped", False) or (getattr(value, "__module__", None) or "").startswith("autovfx_amd")


def _rebind(original, ours, skip: Optional[types.ModuleType] = None) -> List[Tuple[dict, str]]:
    """Every imported module but ``skip`` that holds ``original`` under some name gets ``ours`` instead; returns those slots."""
    slots = []
    for other in list(sys.modules.values()):
        d = getattr(other, "__dict__", None)
        if not isinstance(d, dict) or other is skip:
            continue
        for key, value in list(d.items()):
            if value is original:
                d[key] = ours
                slots.append((d, key))
    return slots


def _patch(module: types.ModuleType) -> None:
    """Apply every row of ``module``'s name whose ``needs`` hold to it, and log what was done for ``uninstall()``."""
    for t in _target(module.__name__):
        _patch_row(module, t)


def _patch_row(module: types.ModuleType, t: _Target) -> None:
    if _gave_up:
        return
    owner = module if t.cls is None else module.__dict__.get(t.cls)
    if t.cls is not None and not isinstance(owner, type):
        return
    d = vars(owner)
    original = d.get(t.attr)
    getter = isinstance(original, property)          # a property target: its fget is what make() wraps
    if original is None or _is_ours(original.fget if getter else original) or \
            not all(callable(d.get(k)) or isinstance(d.get(k), property) for k in t.needs):
        return
    try:
        ours = property(t.make(original.fget), original.fset, original.fdel) if getter else t.make(original)
    except Exception as e:   # torch absent, libgsr_hip.so not built / stale ABI, a GPU-less helper that inherited the environment
        where = module.__name__ if t.cls is None else f"{module.__name__}.{t.cls}"
        _could_not_load(f"{where}.{t.attr} left as the reference's: {t.what}", e)
        return
    setattr(owner, "reference_" + t.attr, original)
    setattr(owner, t.attr, ours)
    _undo.append((owner, t.attr, original, ours, _rebind(original, ours, module) if t.rebind else []))
    if module.__name__ not in t.record:
        t.record.append(module.__name__)


class _PatchingLoader(importlib.abc.Loader):
    def __init__(self, inner):
        self._inner = inner

    def create_module(self, spec):
        return self._inner.create_module(spec) if hasattr(self._inner, "create_module") else None

    def exec_module(self, module):
        self._inner.exec_module(module)
        _patch(module)

    def __getattr__(self, name):   # get_code, get_source, is_package, ... for tools that ask the loader
        return getattr(self._inner, name)


class _RendererHook(importlib.abc.MetaPathFinder):
    """Finds a module named after a row of ``_TARGETS`` with the regular finders and wraps its loader so that the row is applied
    right after the module body ran."""

    def find_spec(self, fullname, path=None, target=None):
        if not _target(fullname):
            return None
        for finder in sys.meta_path:
            if finder is self or not hasattr(finder, "find_spec"):
                continue
            spec = finder.find_spec(fullname, path, target)
            if spec is not None and spec.loader is not None:
                spec.loader = _PatchingLoader(spec.loader)
                return spec
        return None


def install(path: bool = True, strict: bool = True) -> None:
    """Idempotent.  ``path=False`` leaves ``sys.path`` alone (the caller arranged for ``diff_gaussian_rasterization``).
    ``strict`` (default): a replacement that cannot be loaded -- no torch, libgsr_hip.so missing or of another ABI -- raises from
    the import of the target module, loudly, where it happens.  ``strict=False`` is for the interpreter start-up hook
    (integration/sitecustomize.py: every Python process of the machine runs it): one line on stderr, the module keeps the
    reference's code, no second attempt in that process."""
    global _installed, _strict, _gave_up
    _strict = bool(strict)
    if strict:
        _gave_up = False
    if path and (not sys.path or sys.path[0] != _REPO_ROOT):
        if _REPO_ROOT in sys.path:
            sys.path.remove(_REPO_ROOT)
        sys.path.insert(0, _REPO_ROOT)
    stale = sys.modules.get("diff_gaussian_rasterization")
    if stale is not None and not os.path.abspath(getattr(stale, "__file__", "") or "").startswith(_REPO_ROOT):
        raise RuntimeError(f"diff_gaussian_rasterization is already imported from {getattr(stale, '__file__', '?')}: call "
                           "autovfx_amd.install() before anything imports the rasterizer")
    if _installed is None:
        _installed = _RendererHook()
        sys.meta_path.insert(0, _installed)
    for name, module in list(sys.modules.items()):
        if module is not None and _target(name):
            _patch(module)


def uninstall() -> None:
    """Remove the import hook and undo every patch ``install`` made, last first: the original goes back on its owner and into
    the importer slots that were rebound and still hold the replacement, and ``reference_<attr>`` is deleted (meant for tests)."""
    global _installed, _strict, _gave_up
    if _installed is not None and _installed in sys.meta_path:
        sys.meta_path.remove(_installed)
    _installed = None
    _strict, _gave_up = True, False
    while _undo:
        owner, attr, original, ours, slots = _undo.pop()
        setattr(owner, attr, original)
        if "reference_" + attr in vars(owner):
            delattr(owner, "reference_" + attr)
        for d, key in slots:
            if d.get(key) is ours:
                d[key] = original
        if getattr(ours, "_autovfx_amd_wrapped", False):   # built for this original alone (``_mark``): any holder got it from here
            _rebind(ours, original)
    patched_modules.clear()
    patched_models.clear()
