"""ctypes loader for libgsr_hip.so, the C-ABI rasterizer declared in include/gsr.h.

There is deliberately no fallback: if the shared library is missing or does not export the full
ABI, importing this module raises, and so does every package that depends on it
(``diff_gaussian_rasterization``).  Build the library with ``python -m autovfx_amd.build``.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

# PyTorch first, always: its wheel carries its own libamdhip64 / libhsa-runtime64, and the library below asks the loader for
# "libamdhip64.so.7" by name.  Loaded after torch it binds to the runtime torch already brought in -- one HIP runtime in the
# process, so torch's stream handles and allocations mean the same thing on both sides.  Loaded BEFORE torch it would pull in the
# system's runtime, torch's own would follow, and the mixture fails at the first call ("no ROCm-capable device is detected").
import torch  # noqa: F401  (import order matters, see above)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GSR_LIB", os.path.join(_HERE, "lib", "libgsr_hip.so"))

ALLOC_FN = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p)

# enum mirrors of include/gsr.h
GEOM_SLOTS = ("raster", "rgb", "splat_bins", "internal_radii", "depth_order", "point_offsets", "listed", "view_normals")
BIN_SLOTS = ("point_list", "tile_keys")
IMG_SLOTS = ("ranges", "n_contrib")
STAGES = ("preprocess", "depth_sort", "scan", "duplicate", "tile_sort", "ranges", "blend", "colour")
ABI_VERSION = 20


class PngFileInfo(ctypes.Structure):
    """``GsrPngFileInfo`` (gsr.h)."""
    _fields_ = [("width", ctypes.c_int), ("height", ctypes.c_int), ("channels", ctypes.c_int), ("scanline_bytes", ctypes.c_size_t)]


class ExrFileInfo(ctypes.Structure):
    """``GsrExrFileInfo`` (gsr.h)."""
    _fields_ = [("width", ctypes.c_int), ("height", ctypes.c_int), ("bytes_per_line", ctypes.c_int), ("lines_per_block", ctypes.c_int),
                ("channel_at", ctypes.c_int), ("channel_bytes", ctypes.c_int), ("channel_is_half", ctypes.c_int), ("compression", ctypes.c_int),
                ("n_blocks", ctypes.c_int), ("blocks_bytes", ctypes.c_size_t),
                ("channel", ctypes.c_char * 32)]


class PngUnfilterJob(ctypes.Structure):
    """``GsrPngUnfilterJob`` (gsr.h)."""
    _fields_ = [("scanlines", ctypes.c_void_p), ("width", ctypes.c_int), ("height", ctypes.c_int), ("channels", ctypes.c_int),
                ("out_rgba", ctypes.c_void_p), ("scratch", ctypes.c_void_p)]
class AdamTensor(ctypes.Structure):
    """``GsrAdamTensor`` (gsr.h)."""
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p), ("exp_avg_sq", ctypes.c_void_p),
                ("numel", ctypes.c_int64), ("step_size", ctypes.c_float), ("bias2_sqrt", ctypes.c_float)]


ADAM_MAX_TENSORS = 16


class DensifyTensor(ctypes.Structure):
    """``GsrDensifyTensor`` (gsr.h)."""
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("side", ctypes.c_void_p), ("floats_per_row", ctypes.c_int32),
                ("is_moment", ctypes.c_int32)]


class DensifyPlan(ctypes.Structure):
    """``GsrDensifyPlan`` (gsr.h)."""
    _fields_ = [("n_src", ctypes.c_int64), ("n_keep", ctypes.c_int64), ("n_front", ctypes.c_int64), ("n_out", ctypes.c_int64),
                ("n_split", ctypes.c_int64), ("src_of", ctypes.c_void_p), ("child_rows", ctypes.c_void_p), ("split_idx", ctypes.c_void_p)]


DENSIFY_MAX_TENSORS = 18
MAX_SLABS = 8
FORWARD_INFERENCE = 1

OPT_TILE_CULL = 0
OPT_SLABS = 1
OPT_SLAB_FIRST = 2
OPT_DEFER_COLOUR = 3
OPT_SLAB_MIN_REST = 4
OPT_RADIX_RANK = 5           # 0 ballots, 1 verified LDS adds, 2 (default) those where the per-device self-test passed, 3 test hook
OPT_RADIX_RANK_ACTIVE = 6    # read-only: what the current device uses (1 verified LDS adds, 0 ballots)
OPT_BLEND_ORDER = 8          # 1 (default): large images are blended longest tile list first inside each XCD's band
OPT_DEPTH_DROP = 7           # 1 (default): Gaussians that emit nothing leave the depth sort in its first pass
OPT_BACKWARD_DETERMINISTIC = 10  # 1: per-Gaussian gradient sums in a fixed order (same bits on every run); default 0: float atomics
OPT_GRAD_SLABS = 11              # 1 (default): a grad-mode forward may be an inference call (depth slabs, deferred colours); the backward walks the slabs
OPT_RADIX_RANK_FALLBACKS = 9 # read-only: tiles on the current device whose LDS-add ranks failed the order check (re-ranked with ballots)


class RawParams(ctypes.Structure):
    """``gsr_raw_params`` (include/gsr.h): device pointers of a model's six raw parameter tensors."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("xyz", "log_scales", "rotations", "opacity_logits", "features_dc", "features_rest")]


class GsrLibraryError(ImportError):
    pass


# ---- every function include/gsr.h declares: name -> (restype, argtypes), in the header's order ----------------------------------------
_i, _u, _u32, _i64, _f, _sz = ctypes.c_int, ctypes.c_uint, ctypes.c_uint32, ctypes.c_int64, ctypes.c_float, ctypes.c_size_t
_p, _s = ctypes.c_void_p, ctypes.c_char_p    # _p: device float* / int* travel as integers (tensor.data_ptr()); _s: host bytes


def _array(ctype, n):
    """A host array of ``n`` values, passed with ``ctypes.byref``: ``ctype name[n]`` in the header."""
    return ctypes.POINTER(ctype * n)


_arenas = [ALLOC_FN, _p, ALLOC_FN, _p, ALLOC_FN, _p]   # geom_alloc geom_user binning_alloc binning_user image_alloc image_user
_camera = [_p, _p, _p, _f, _f]                         # viewmatrix projmatrix cam_pos tan_fovx tan_fovy
_forward = _arenas + [
    _i, _i, _i,                                        # P D M
    _p, _i, _i,                                        # background width height
    _p, _p, _p, _p, _p, _f, _p, _p,                    # means3D shs colors_precomp opacities scales scale_modifier rotations cov3D_precomp
    *_camera, _i,                                      # ... prefiltered
    _p, _p, _p, _p]                                    # out_color out_depth out_alpha radii
_forward_extra = _forward + [_p, _p, _u, _i, _p]       # extra_features out_extra flags debug stream
_forward_raw = _arenas + [
    _i, _i, _i,                                        # P D M
    _p, _i, _i,                                        # background width height
    ctypes.POINTER(RawParams), _f,                     # raw scale_modifier
    *_camera, _i,                                      # ... prefiltered
    _p, _p, _p, _p, _p, _u, _i, _p]                    # out_color out_depth out_alpha radii out_normal flags debug stream
_png_dims = [_i, _i, _i]                               # width height channels
_frame_files = [_p, _p, _p, _p, _f, _p, _i, _i,        # color alpha depth normal depth_scale turbo_lut width height
                _p, _p, _p, _p, _p]                    # png_rgba png_depth_preview png_normal npy_plane work
_field_inputs = [_i64, _i, _i64, _p, _p, _p, _p, _p, _p, _f]   # n K P x idx centers M strengths min_scaling density_factor
_placed = [_p, _p, _p, _p, _p, _p, _p]                 # out_means3D out_scales out_rotations out_opacities out_shs out_min_axis stream
_backward_head = [_i, _i, _i, _i, _p, _i, _i]          # P D M R background width height
_backward_arenas = [_p, _p, _p, _p]                    # radii geom_buffer binning_buffer image_buffer

SIGNATURES = {
    # the forward pass
    "gsr_forward": (_i, _forward + [_i, _p]),          # ... debug stream
    "gsr_forward_extra": (_i, _forward_extra),
    "gsr_forward_begin": (_p, _forward_extra),
    "gsr_forward_finish": (_i, [_p]),                  # call
    "gsr_forward_ready": (_i, [_p]),
    "gsr_forward_cancel": (None, [_p]),
    "gsr_forward_raw": (_i, _forward_raw),
    "gsr_forward_raw_begin": (_p, _forward_raw),
    "gsr_mark_visible": (_i, [_i, _p, _p, _p, _p, _p]),                # P means3D viewmatrix projmatrix present stream
    "gsr_blend": (_i, [_p, _p, _p, _i, _i, _p, _p, _p, _p, _p, _p]),   # geom binning image width height features background out_color out_depth out_alpha stream
    # the compositor and the frame files
    "gsr_composite": (_i, [_i, _i] + [_p] * 12 + [_p]),                # width height bg_c o_c o_d s_c s_d o_s_c o_gs_c o_gs_d s_f_c s_f_d s_f_c_pre out stream
    "gsr_pack_rgba8": (_i, [_p, _p, _p, _i, _i, _p]),                  # color alpha rgba8 width height stream
    "gsr_png_size": (_sz, _png_dims),
    "gsr_png_room": (_sz, _png_dims),
    "gsr_frame_files": (_i, _frame_files + [_p]),                      # ... stream
    "gsr_png_encode": (_i, [_p, _i, _i, _i, _i, _p, _p]),              # pixels width height channels planar out stream
    "gsr_png_deflate_max_size": (_sz, _png_dims),
    "gsr_png_deflate_room": (_sz, _png_dims),
    "gsr_png_deflate_scratch": (_sz, _png_dims),
    "gsr_png_encode_deflate": (_i, [_p, _i, _i, _i, _i, _p, _p, _p, _p]),   # pixels width height channels planar out scratch out_len stream
    "gsr_frame_files_deflate": (_i, _frame_files + [_p, _p, _p]),      # ... png_scratch png_lengths stream
    "gsr_cube_to_equirect": (_i, [ctypes.POINTER(_p), _i, _i, ctypes.POINTER(_p),   # faces face_size channels depth_faces
                                  _p, _p, _p, _i, _i, _p, _p, _p, _p]),             # grid_u grid_v grid_ceil height width out out_u8 out_depth stream
    "gsr_resize_rgba8_bilinear": (_i, [_p, _i, _i, _p, _i, _i, _p, _p]),   # src src_width src_height dst dst_width dst_height tmp stream
    "gsr_resize_f32_nearest": (_i, [_p, _i, _i, _p, _i, _i, _p]),          # src src_width src_height dst dst_width dst_height stream
    # the compositor's input files
    "gsr_png_unfilter_scratch": (_sz, [_i, _i]),                       # width height
    "gsr_png_unfilter": (_i, [_p, _i, _i, _i, _p, _p, _p]),            # scanlines width height channels out_rgba scratch stream
    "gsr_png_unfilter_batch": (_i, [_i, _p, _p]),                      # count jobs stream
    "gsr_exr_unpack_channel": (_i, [_p, _i, _i, _i, _i, _i, _p, _p]),  # blocks height bytes_per_line lines_per_block channel_at channel_bytes plane stream
    "gsr_upload": (_i, [_p, _s, _sz, _p]),                             # device_dst host_src bytes stream
    "gsr_png_file_probe": (_i, [_s, _sz, _p]),                         # file file_bytes info
    "gsr_png_file_inflate": (_i, [_s, _sz, _p, _sz]),                  # file file_bytes scanlines scanline_bytes
    "gsr_exr_file_probe": (_i, [_s, _sz, _s, _p]),                     # file file_bytes channel info
    "gsr_exr_file_inflate": (_i, [_s, _sz, _s, _p, _sz]),              # file file_bytes channel blocks blocks_bytes
    "gsr_exr_file_pack": (_i, [_s, _sz, _s, _p, _sz, _p, _p]),         # file file_bytes channel packed packed_room jobs packed_bytes
    "gsr_inflate_zlib_blocks": (_i, [_p, _p, _p, _i, _p, _p, _p]),     # streams out jobs count status any_error stream
    "gsr_selftest_inflate_host": (_i, [_s, _sz, _p, _sz]),             # zlib_stream stream_bytes out out_bytes
    # sorting and nearest neighbours
    "gsr_radix_scratch_bytes": (_sz, [_u32, _i]),                      # n bits
    "gsr_radix_sort_pairs": (_i, [_u32, _i, _p, _p, _p, _p, _i, _p,    # n bits keys keys_alt vals vals_alt iota_payload scratch
                                  _sz, ctypes.POINTER(_i), _p]),       # scratch_bytes sorted_in_alt stream
    "gsr_knn3_scratch_bytes": (_sz, [_u32]),                           # n
    "gsr_knn3_mean_dist": (_i, [_u32, _p, _p, _p, _sz, _p]),           # n points out scratch scratch_bytes stream
    "gsr_knn_points_scratch_bytes": (_sz, [_i64, _i64, _i]),           # n1 n2 same
    "gsr_knn_points": (_i, [_i64, _p, _i64, _p, _i, _p, _p, _p, _sz, _p]),   # n1 p1 n2 p2 K dists idx scratch scratch_bytes stream
    "gsr_closest_tri_plan_bytes": (_sz, [_i64]),                       # F
    "gsr_closest_tri_plan_scratch_bytes": (_sz, [_i64]),               # F
    "gsr_closest_tri_plan": (_i, [_i64, _p, _i64, _p, _p, _sz, _p, _sz, _p]),   # V verts F faces plan plan_bytes scratch scratch_bytes stream
    "gsr_closest_tri_query": (_i, [_i64, _p, _p, _sz, _p, _p, _p, _p]),         # n points plan plan_bytes face_idx sq_dist closest stream
    "gsr_ray_first_hit": (_i, [_i64, _p, _p, _p, _sz, _p, _p, _p, _p]),         # n origins dirs plan plan_bytes face_idx t bary stream
    # training: the density field, SSIM, Adam, densification
    "gsr_field_scratch_bytes": (_sz, [_i64]),                          # P
    "gsr_field_forward": (_i, _field_inputs + [_p, _p, _p, _p, _sz, _p]),            # ... density opacities beta scratch scratch_bytes stream
    "gsr_field_backward": (_i, _field_inputs + [_p, _p, _p, _p, _p, _p, _sz, _p]),   # ... g_density g_opacities g_beta dx accum scratch scratch_bytes stream
    "gsr_level_surface": (_i, [_i64, _i, _i64, _i, _i, _p, _p, _p, _p, _p, _p, _p, _f,   # n K P S L origins dirs stds idx centers M strengths density_factor
                               _p, _array(_f, 8), _p, _p, _p, _p, _p, _p, _sz, _p]),     # range levels hit t points normals densities scratch scratch_bytes stream
    "gsr_mesh_raster_plan_bytes": (_sz, [_i64, _i64, _i, _i]),         # F N H W
    "gsr_mesh_raster_pair_bytes": (_sz, [_i64]),                       # pairs
    "gsr_mesh_raster_count": (_i, [_i64, _i64, _p, _p, _p, _i, _i, _i, _p, _sz, ctypes.POINTER(_i64), _p]),   # F N face_verts first num H W cull plan plan_bytes pair_total stream
    "gsr_mesh_raster": (_i, [_i64, _i64, _p, _p, _p, _p, _i, _i, _f, _i, _i, _i, _i,   # F N face_verts first num neighbour H W blur_radius K perspective clip cull
                             _p, _sz, _i64, _p, _sz, _p, _p, _p, _p, _p]),             # plan plan_bytes pair_total pairs pair_bytes pix_to_face zbuf bary_coords dists stream
    "gsr_face_areas_normals": (_i, [_i64, _i64, _p, _p, _p, _p, _p]),                        # V F verts faces areas normals stream
    "gsr_face_areas_normals_backward": (_i, [_i64, _i64, _p, _p, _p, _p, _p, _p]),           # V F verts faces grad_areas grad_normals grad_verts stream
    "gsr_interp_face_attrs": (_i, [_i64, _i64, _i, _p, _p, _p, _p, _p]),                     # P F D pix_to_face bary attrs out stream
    "gsr_interp_face_attrs_backward": (_i, [_i64, _i64, _i, _p, _p, _p, _p, _p, _p, _p]),    # P F D pix_to_face bary attrs grad_out grad_bary grad_attrs stream
    "gsr_bound_gaussians": (_i, [_i64, _i64, _i, _p, _p, _p, _p, _p, _p, _i, _p, _p, _p, _p]),   # V F G verts faces bary complex log_scales thickness standardize points scaling quaternions stream
    "gsr_bound_gaussians_backward": (_i, [_i64, _i64, _i, _p, _p, _p, _p, _p, _i, _p, _p, _p, _p, _p, _p, _p]),   # V F G verts faces bary complex log_scales standardize g_points g_scaling g_quaternions grad_verts grad_complex grad_log_scales stream
    "gsr_texture_texels": (_i, [_i64, _i64, _i, _p, _p, _p, _p, _p, _p]),                    # P F T pix_to_face bary zbuf face_uvs texel stream
    "gsr_texture_bake_view": (_i, [_i64, _i64, _i, _p, _p, _p, _p, _p, _i64, _p, _p, _p, _p]),   # P F T pix_to_face bary zbuf face_uvs rgb rgb_stride tex count owner stream
    "gsr_texture_fill": (_i, [_i64, _i64, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p]),   # V F G A S n verts faces centers inv_scaled_rot features texel_offset texel_bary tex stream
    "gsr_normal_consistency_plan_scratch_bytes": (_sz, [_i64]),        # F
    "gsr_normal_consistency_plan": (_i, [_i64, _i64, _p, _p, _p, _p, _p, _sz, _p]),   # V F faces order partners pairs scratch scratch_bytes stream
    "gsr_normal_consistency_scratch_bytes": (_sz, [_i64]),             # F
    "gsr_normal_consistency_forward": (_i, [_i64, _i64, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),   # V F verts faces order partners pairs loss terms_or_null scratch scratch_bytes stream
    "gsr_normal_consistency_backward": (_i, [_i64, _i64, _p, _p, _p, _p, _p, _p, _p, _p]),           # V F verts faces order partners pairs grad_loss grad_verts stream
    "gsr_ssim_scratch_bytes": (_sz, [_i, _i, _i, _i]),                 # n c h w
    "gsr_ssim_forward": (_i, [_i, _i, _i, _i, _p, _p, _p, _i, _p, _p, _p, _sz, _p]),   # n c h w x y window11 per_image out coef_or_null scratch scratch_bytes stream
    "gsr_ssim_backward": (_i, [_i, _i, _i, _i, _p, _p, _p, _p, _i, _p, _p, _p]),       # n c h w x y coef window11 per_image grad_out grad_x stream
    "gsr_adam_step": (_i, [ctypes.POINTER(AdamTensor), _i, _f, _f, _f, _f, _p]),       # tensors count w b2 c eps stream
    "gsr_densify_stats": (_i, [_i64, _p, _i, _p, _p, _p, _p, _p, _p]),   # n grad grad_row_floats filter accum denom radii max_radii stream
    "gsr_densify_plan_scratch_bytes": (_sz, [_i64]),                   # n
    "gsr_densify_plan": (_i, [_i64, _p, _p, _p, _p, _f, _f, _f, _i, _f,   # n accum denom scaling opacity max_grad dense_bound min_opacity ws_test ws_bound
                              _p, _p, _p, _p, _sz, _p]),                  # src_of split_idx counts scratch scratch_bytes stream
    "gsr_densify_apply": (_i, [ctypes.POINTER(DensifyTensor), _i, ctypes.POINTER(DensifyPlan), _p]),   # tensors count plan stream
    # render()'s elementwise work, dynamic scenes, self-tests
    "gsr_view_normals": (_i, [_i, _p, _p, _p, _p, _p]),                # P means3D axis cam_pos colors stream
    "gsr_normal_maps": (_i, [_i, _i, _p, _p, _p, _f, _f, _f, _f, _p, _p, _p]),   # width height normal_rgb depth c2w fx fy cx cy normal pseudo_normal stream
    "gsr_place_object": (_i, [_i, _p, _p, _p, _p, _p, _i, _array(_f, 21)] + _placed),   # n xyz rotation_raw log_scale opacity shs M placement ...
    "gsr_place_object_subset": (_i, [_i, _p, _p, _p, _p, _p, _p, _i, _array(_f, 21)] + _placed),   # m subset xyz rotation_raw log_scale opacity shs M placement ...
    "gsr_selftest_exp": (_i, [_u32, _u32, _p, _p]),                    # first_bits count device_mismatches stream
    "gsr_selftest_lds_atomic_order": (_i, [_u32, _u32, _u32, _p, _p]),   # workgroups rounds seed device_mismatches stream
    # the backward pass
    "gsr_backward": (_i, _backward_head + [
        _p, _p, _p, _p, _f, _p, _p,                    # means3D shs colors_precomp scales scale_modifier rotations cov3D_precomp
        *_camera, *_backward_arenas,
        _p, _p, _p, _p,                                # accum_alphas dL_dpix dL_dpix_depth dL_dpix_alpha
        _p, _p, _p, _p, _p, _p, _p, _p, _p, _p,        # dL_dmean2D conic opacity color depth mean3D cov3D sh scale rot
        _p, _i, _p]),                                  # accum_scratch debug stream
    "gsr_backward_raw": (_i, _backward_head + [
        ctypes.POINTER(RawParams), _f,                 # raw scale_modifier
        *_camera, *_backward_arenas,
        _p, _p, _p, _p, _p,                            # accum_alphas dL_dpix dL_dpix_depth dL_dpix_alpha dL_dpix_normal
        _p, _p, _p, _p, _p, _p, _p,                    # dL_dmean2D xyz log_scales rotations opacity_logits features_dc features_rest
        _p, _i, _p]),                                  # accum_scratch debug stream
    # introspection
    "gsr_last_geom_offsets": (_i, [_array(_sz, len(GEOM_SLOTS))]),
    "gsr_last_binning_offsets": (_i, [_array(_sz, len(BIN_SLOTS))]),
    "gsr_last_image_offsets": (_i, [_array(_sz, len(IMG_SLOTS))]),
    "gsr_last_pair_counts": (_i, [_array(_u32, 2)]),
    "gsr_last_slab_pairs": (_i, [_array(_u32, MAX_SLABS)]),
    # options, timing, identity
    "gsr_set_option": (_i, [_i, _i]),                  # option value
    "gsr_plan_slabs": (_i, [_u32, _i, _i, _array(_u32, MAX_SLABS)]),   # live_pairs width height cuts
    "gsr_get_option": (_i, [_i]),
    "gsr_set_stage_timing": (None, [_i]),              # enable
    "gsr_get_stage_times": (_i, [_array(_f, len(STAGES))]),
    "gsr_get_call_times": (_i, [ctypes.POINTER(_f), _i]),   # ms capacity
    "gsr_get_backward_times": (_i, [_array(_f, 2)]),
    "gsr_last_error": (_s, []),
    "gsr_abi_version": (_i, []),
    "gsr_target_arch": (_s, []),
}
SYMBOLS = tuple(SIGNATURES)


def _load() -> ctypes.CDLL:
    if not os.path.exists(LIB_PATH):
        raise GsrLibraryError(
            f"{LIB_PATH} not found: the HIP rasterizer is not built. Run `python -m autovfx_amd.build` "
            "(needs hipcc; cross-compiles for gfx950 without a GPU). There is no CPU fallback.")
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # e.g. libamdhip64.so missing
        raise GsrLibraryError(f"could not load {LIB_PATH}: {e}") from e
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    if missing:
        raise GsrLibraryError(f"{LIB_PATH} does not export {missing}; rebuild it")
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    if lib.gsr_abi_version() != ABI_VERSION:
        raise GsrLibraryError(f"{LIB_PATH} has ABI {lib.gsr_abi_version()}, this binding expects {ABI_VERSION}")
    return lib


lib = _load()

# A/B from the shell, (variable, option, accepted values); unset or anything else = the library default.  GSR_RADIX_RANK: 0 forces the
# ballot rank of the radix sort, 1 the verified LDS adds, 2 (the default) = those where the per-device self-test passed, 3 = with an
# injected inversion (test hook).  GSR_BACKWARD_DETERMINISTIC=1: the same gradient bits on every run (include/gsr.h).
ENV_OPTIONS = (("GSR_RADIX_RANK", OPT_RADIX_RANK, ("0", "1", "2", "3")),
               ("GSR_BLEND_ORDER", OPT_BLEND_ORDER, ("0", "1")),
               ("GSR_DEPTH_DROP", OPT_DEPTH_DROP, ("0", "1")),
               ("GSR_GRAD_SLABS", OPT_GRAD_SLABS, ("0", "1")),
               ("GSR_BACKWARD_DETERMINISTIC", OPT_BACKWARD_DETERMINISTIC, ("0", "1")))
for _var, _option, _allowed in ENV_OPTIONS:
    if os.environ.get(_var, "") in _allowed:
        lib.gsr_set_option(_option, int(os.environ[_var]))


def last_error() -> str:
    return lib.gsr_last_error().decode("utf-8", "replace")


# ---- the one call path into the library ---------------------------------------------------------------------------------------
def stream_ptr(device) -> ctypes.c_void_p:
    """torch's current HIP stream on ``device``, as the ``void* stream`` every launching entry point ends in."""
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    """Device pointer of a tensor, or NULL for None and for the reference's "empty tensor means absent"."""
    return None if t is None or t.numel() == 0 else t.data_ptr()


def capturing() -> bool:
    """Is the current stream capturing a graph?  Never initialises the GPU: a process that has not touched it captures nothing."""
    return torch.cuda.is_initialized() and torch.cuda.is_current_stream_capturing()


def failure(name: str, rc) -> RuntimeError:
    """What every failed library call raises: the entry point, what it returned and the library's own words."""
    return RuntimeError(f"{name} failed ({rc}): {last_error()}")


def check(name: str, rc: int) -> None:
    if rc != 0:
        raise failure(name, rc)


def call(name: str, *args, device=None) -> None:
    """One ``int``-status entry point: looked up by name at call time, ``stream_ptr(device)`` appended when a device is given, a
    non-zero status raised with the library's message."""
    if device is not None:
        args += (stream_ptr(device),)
    check(name, getattr(lib, name)(*args))


def scratch(name: str, *size_args, device):
    """``(uint8 tensor, nbytes)`` of device scratch sized by the ``gsr_*_scratch_bytes`` query ``name``."""
    nbytes = int(getattr(lib, name)(*size_args))
    return torch.empty(nbytes, dtype=torch.uint8, device=device), nbytes


def offsets(kind: str) -> dict:
    names, fn = {"geom": (GEOM_SLOTS, lib.gsr_last_geom_offsets), "binning": (BIN_SLOTS, lib.gsr_last_binning_offsets),
                 "image": (IMG_SLOTS, lib.gsr_last_image_offsets)}[kind]
    arr = (ctypes.c_size_t * len(names))()
    if fn(ctypes.byref(arr)) != 0:
        raise RuntimeError(last_error())
    return dict(zip(names, (int(v) for v in arr)))


def pair_counts() -> dict:
    arr = (ctypes.c_uint32 * 2)()
    if lib.gsr_last_pair_counts(ctypes.byref(arr)) != 0:
        raise RuntimeError(last_error())
    return {"num_rendered": int(arr[0]), "live_pairs": int(arr[1])}


def slab_pairs() -> list:
    """Pairs in the list of each depth slab of this thread's last forward call (waits for that call's stream)."""
    arr = (ctypes.c_uint32 * MAX_SLABS)()
    n = lib.gsr_last_slab_pairs(ctypes.byref(arr))
    if n < 0:
        raise RuntimeError(last_error())
    return [int(arr[i]) for i in range(n)]


def plan_slabs(live_pairs: int, width: int, height: int) -> list:
    """Inclusive pair offsets at which an inference call with that many live pairs would cut its depth slabs under the
    current options ([] = one slab).  Host logic only."""
    arr = (ctypes.c_uint32 * MAX_SLABS)()
    n = lib.gsr_plan_slabs(int(live_pairs), int(width), int(height), ctypes.byref(arr))
    if n < 0:
        raise RuntimeError(last_error())
    return [int(arr[i]) for i in range(n - 1)]


def set_option(option: int, value: int) -> None:
    if lib.gsr_set_option(int(option), int(value)) != 0:
        raise RuntimeError(last_error())


def get_option(option: int) -> int:
    return int(lib.gsr_get_option(int(option)))


def set_stage_timing(enable: bool) -> None:
    lib.gsr_set_stage_timing(1 if enable else 0)


def call_times_ms(capacity: int = 256) -> list:
    """Device milliseconds (first kernel to last) of this thread's most recent timed calls, newest first."""
    arr = (ctypes.c_float * capacity)()
    n = lib.gsr_get_call_times(arr, capacity)
    if n < 0:
        raise RuntimeError(last_error())
    return [float(arr[i]) for i in range(n)]


def backward_times_ms() -> dict:
    """Mean milliseconds of gsr_backward's two kernels over the calls since ``set_stage_timing(True)`` (process-wide)."""
    arr = (ctypes.c_float * 2)()
    n = lib.gsr_get_backward_times(ctypes.byref(arr))
    if n < 0:
        raise RuntimeError(last_error())
    return {"render_backward": float(arr[0]), "preprocess_backward": float(arr[1]), "calls": int(n)}


def stage_times_ms() -> dict:
    """Mean per-stage milliseconds over the calls since ``set_stage_timing(True)``; key ``calls``
    holds how many calls were averaged."""
    arr = (ctypes.c_float * len(STAGES))()
    n = lib.gsr_get_stage_times(ctypes.byref(arr))
    if n < 0:
        raise RuntimeError(last_error())
    out = dict(zip(STAGES, (float(v) for v in arr)))
    out["calls"] = int(n)
    return out
