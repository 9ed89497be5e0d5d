"""The C-ABI shared library: loads without a GPU, exports every symbol include/gsr.h declares,
agrees with the Python mirrors of its enums, and rejects bad calls without touching a device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "gsr.h")).read()


def declared_functions():
    return re.findall(r"GSR_API\s+[\w\s\*]+?\b(gsr_\w+)\s*\(", HEADER)


def enum_members(name):
    body = re.search(r"typedef enum " + name + r"\s*\{(.*?)\}", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [m for m in re.findall(r"\b(GSR_\w+)\b", body)]


def test_header_declares_the_reference_entry_points():
    fns = declared_functions()
    for must in ("gsr_forward", "gsr_mark_visible", "gsr_backward", "gsr_last_error"):
        assert must in fns
    # every entry point cites the reference interface it replaces
    for cite in ("rasterizer.h:31-55", "rasterizer.h:24-29", "rasterizer.h:57-90", "rasterize_points.cu:36-119"):
        assert cite in HEADER


def test_library_exports_every_declared_symbol():
    from autovfx_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    fns = declared_functions()
    assert sorted(fns) == sorted(_lib.SYMBOLS)
    for f in fns:
        assert hasattr(lib, f), f"{f} not exported"
    assert _lib.lib.gsr_abi_version() == int(re.search(r"#define GSR_ABI_VERSION (\d+)", HEADER).group(1))
    assert _lib.lib.gsr_target_arch() == b"gfx950"


def test_enum_mirrors_match_header():
    from autovfx_amd import _lib
    to_name = lambda members, prefix: tuple(m[len(prefix):].lower() for m in members if not m.endswith("NUM_SLOTS") and m != "GSR_STAGE_NUM")
    assert to_name(enum_members("gsr_geom_slot"), "GSR_GEOM_") == tuple(s.lower() for s in _lib.GEOM_SLOTS)
    assert to_name(enum_members("gsr_binning_slot"), "GSR_BIN_") == _lib.BIN_SLOTS
    assert to_name(enum_members("gsr_image_slot"), "GSR_IMG_") == _lib.IMG_SLOTS
    assert to_name(enum_members("gsr_stage"), "GSR_STAGE_") == _lib.STAGES


def test_options_are_host_state_with_the_documented_defaults():
    """gsr_option (include/gsr.h): the binding's OPT_* mirror the enum, every option reads back its documented default [n],
    set / get round-trip without a device, the read-only and range rules hold."""
    from autovfx_amd import _lib
    members = [m for m in enum_members("gsr_option") if m != "GSR_OPT_NUM"]
    for i, m in enumerate(members):
        assert getattr(_lib, "OPT_" + m[len("GSR_OPT_"):]) == i, m
    # the default stands in brackets at the start of each option's comment
    body = HEADER[HEADER.index("typedef enum gsr_option"):HEADER.index("} gsr_option;")]
    defaults = [int(x) for x in re.findall(r"/\* \[(\d+)\]", body)]
    settable = [m for m in members if m not in ("GSR_OPT_RADIX_RANK_ACTIVE", "GSR_OPT_RADIX_RANK_FALLBACKS")]
    assert len(defaults) == len(settable), (defaults, settable)
    for m, want in zip(settable, defaults):
        assert _lib.get_option(getattr(_lib, "OPT_" + m[len("GSR_OPT_"):])) == want, m
    for opt, other in ((_lib.OPT_DEPTH_DROP, 0), (_lib.OPT_BLEND_ORDER, 0), (_lib.OPT_SLAB_FIRST, 123)):
        was = _lib.get_option(opt)
        _lib.set_option(opt, other)
        assert _lib.get_option(opt) == other
        _lib.set_option(opt, was)
    assert _lib.lib.gsr_set_option(_lib.OPT_RADIX_RANK_ACTIVE, 1) != 0 and "read-only" in _lib.last_error()
    assert _lib.lib.gsr_set_option(_lib.OPT_RADIX_RANK_FALLBACKS, 0) != 0 and "read-only" in _lib.last_error()
    assert _lib.lib.gsr_set_option(_lib.OPT_RADIX_RANK, 4) != 0
    assert _lib.lib.gsr_set_option(len(members), 0) != 0 and _lib.lib.gsr_set_option(-1, 0) != 0


def test_argument_errors_do_not_need_a_device():
    from autovfx_amd import _lib
    L = _lib.lib
    bw_tail = [None, None, None, None, 1.0, None, None,   # means3D shs colors scales mod rotations cov3D
               None, None, None, 0.5, 0.5] + [None] * 19 + [0, None]
    assert L.gsr_backward(-1, 0, 0, 0, None, 8, 8, *bw_tail) == -1
    assert L.gsr_backward(0, 0, 0, 0, None, 8, 8, *bw_tail) == 0      # P == 0: nothing to do
    assert L.gsr_backward(4, 0, 0, 0, None, 8, 8, *bw_tail) == -1 and "null" in _lib.last_error()
    assert L.gsr_view_normals(-1, None, None, None, None, None) == -1
    assert L.gsr_view_normals(0, None, None, None, None, None) == 0
    assert L.gsr_view_normals(5, None, None, None, None, None) == -1 and "null" in _lib.last_error()
    assert L.gsr_normal_maps(0, 4, None, None, None, 1.0, 1.0, 0.0, 0.0, None, None, None) == -1
    assert L.gsr_normal_maps(4, 4, None, None, None, 1.0, 1.0, 0.0, 0.0, None, None, None) == -1
    assert L.gsr_radix_sort_pairs(5, 0, None, None, None, None, 0, None, 0, None, None) == -1      # bits out of range
    assert L.gsr_radix_sort_pairs(0, 8, None, None, None, None, 0, None, 0, None, None) == 0       # nothing to sort
    assert L.gsr_radix_sort_pairs(5, 8, None, None, None, None, 0, None, 0, None, None) == -1
    assert L.gsr_radix_scratch_bytes(4096, 32) == (256 * 4 + 256 + 4) * 4 and L.gsr_radix_scratch_bytes(4097, 13) == (256 * 4 + 256 + 4) * 4
    assert L.gsr_selftest_exp(0, 1, None, None) == -1
    assert L.gsr_mark_visible(-1, None, None, None, None, None) == -1
    assert L.gsr_mark_visible(0, None, None, None, None, None) == 0
    null_cb = ctypes.cast(None, _lib.ALLOC_FN)
    args = [null_cb, None, null_cb, None, null_cb, None]
    tail = [None] * 4 + [0, None]
    # P == 0 returns 0 before anything else is looked at (rasterize_points.cu:83)
    assert L.gsr_forward(*args, 0, 3, 16, None, 64, 64, None, None, None, None, None, 1.0, None, None, None, None,
                         None, 0.5, 0.5, 0, *tail) == 0
    assert L.gsr_forward(*args, 5, 3, 16, None, 0, 64, None, None, None, None, None, 1.0, None, None, None, None,
                         None, 0.5, 0.5, 0, *tail) == -1
    assert L.gsr_forward(*args, 5, 3, 16, None, 64, 64, None, None, None, None, None, 1.0, None, None, None, None,
                         None, 0.5, 0.5, 0, *tail) == -1
    assert "null" in _lib.last_error()
    # the two-feature variant: same checks, plus its own two pointers
    tail_extra = [None] * 4 + [None, None, 0, 0, None]          # ... extra_features, out_extra, flags, debug, stream
    assert L.gsr_forward_extra(*args, 0, 3, 16, None, 64, 64, None, None, None, None, None, 1.0, None, None, None, None,
                               None, 0.5, 0.5, 0, *tail_extra) == 0
    assert L.gsr_forward_extra(*args, 5, 3, 16, None, 64, 64, None, None, None, None, None, 1.0, None, None, None, None,
                               None, 0.5, 0.5, 0, *([None] * 4 + [4096, None, 0, 0, None])) == -1
    assert "extra" in _lib.last_error()                           # the two extra pointers come together or not at all
    assert L.gsr_forward_extra(*args, 5, 3, 16, None, 64, 64, None, None, None, None, None, 1.0, None, None, None, None,
                               None, 0.5, 0.5, 0, *([None] * 4 + [None, None, 0x80, 0, None])) == -1   # unknown flag ...
    assert "null" in _lib.last_error() or "flags" in _lib.last_error()   # ... or the null callbacks, whichever is seen first
    # the split call: a failed begin returns NULL and says why; finish refuses a NULL handle; cancel accepts one
    assert L.gsr_forward_begin(*args, 5, 3, 16, None, 64, 64, None, None, None, None, None, 1.0, None, None, None, None,
                               None, 0.5, 0.5, 0, *tail_extra) is None
    assert "null" in _lib.last_error()
    assert L.gsr_forward_finish(None) == -1 and "handle" in _lib.last_error()
    L.gsr_forward_cancel(None)
    h = L.gsr_forward_begin(*args, 0, 3, 16, None, 64, 64, None, None, None, None, None, 1.0, None, None, None, None,
                            None, 0.5, 0.5, 0, *tail_extra)
    assert h and L.gsr_forward_finish(h) == 0                        # P == 0: a handle with nothing queued


def test_missing_library_fails_loudly(tmp_path, monkeypatch):
    import importlib
    import sys
    monkeypatch.setenv("GSR_LIB", str(tmp_path / "nope.so"))
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k.startswith(("autovfx_amd._lib", "diff_gaussian_rasterization"))}
    import autovfx_amd
    monkeypatch.delattr(autovfx_amd, "_lib", raising=False)   # `from autovfx_amd import _lib` must re-import
    try:
        with pytest.raises(ImportError, match="no CPU fallback"):
            importlib.import_module("autovfx_amd._lib")
        with pytest.raises(ImportError):
            importlib.import_module("diff_gaussian_rasterization")
    finally:
        for k in list(sys.modules):
            if k.startswith(("autovfx_amd._lib", "diff_gaussian_rasterization")):
                sys.modules.pop(k)
        sys.modules.update(saved)


def test_cpu_tensors_are_rejected_not_silently_handled():
    import torch
    from autovfx_amd import scenes
    from diff_gaussian_rasterization import GaussianRasterizer
    from helpers import settings_for
    c = scenes.config_c1(P=4)
    rast = GaussianRasterizer(settings_for(scenes.c1_camera(16, 16), "cpu"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rast(c.means3D, torch.zeros_like(c.means3D), c.opacities, shs=c.shs, scales=c.scales, rotations=c.rotations)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rast.markVisible(c.means3D)


def declarations():
    """name -> (return type, parameter count) of every function the header declares, comments stripped."""
    text = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"GSR_API\s+([\w\s\*]+?)\b(gsr_\w+)\s*\(([^)]*)\)\s*;", text):
        params = params.strip()
        out[name] = (re.sub(r"\s*\*", "*", " ".join(ret.split())), 0 if params == "void" else len(params.split(",")))
    return out


def test_signature_lengths_match_the_header():
    from autovfx_amd import _lib
    decl = declarations()
    assert sorted(decl) == sorted(declared_functions()) == sorted(_lib.SIGNATURES)
    for name, (_ret, count) in decl.items():
        assert len(_lib.SIGNATURES[name][1]) == count, name
        assert len(getattr(_lib.lib, name).argtypes) == count, name


def test_return_types_match_the_header():
    from autovfx_amd import _lib
    ctype_of = {"size_t": ctypes.c_size_t, "const char*": ctypes.c_char_p, "void*": ctypes.c_void_p, "void": None, "int": ctypes.c_int}
    for name, (ret, _count) in declarations().items():
        assert _lib.SIGNATURES[name][0] is ctype_of[ret], (name, ret)
        assert getattr(_lib.lib, name).restype is ctype_of[ret], (name, ret)


def test_check_raises_with_the_status_and_the_library_message():
    from autovfx_amd import _lib
    _lib.check("gsr_x", 0)
    assert _lib.lib.gsr_set_option(-1, 0) != 0
    why = _lib.last_error()
    assert why
    with pytest.raises(RuntimeError) as e:
        _lib.check("gsr_x", -1)
    assert "gsr_x failed (-1)" in str(e.value) and why in str(e.value)


def test_call_looks_the_function_up_at_call_time(monkeypatch):
    from autovfx_amd import _lib
    monkeypatch.setattr(_lib.lib, "gsr_adam_step", lambda *a: -1)
    with pytest.raises(RuntimeError, match=r"gsr_adam_step failed \(-1\)"):
        _lib.call("gsr_adam_step", None, 0, 0.0, 0.0, 0.0, 0.0, None)


def _null_faces():
    return (ctypes.c_void_p * 6)()


# One refusal per validation path of the entry points that live beside their kernels and have no device-free refusal test in a
# file of their own: (id, function, arguments, status, gsr_last_error()).  Every call stops at an argument check, before any launch.
REFUSALS = [
    ("mark_visible-size", "gsr_mark_visible", (-1, None, None, None, None, None), -1, "P < 0"),
    ("mark_visible-null", "gsr_mark_visible", (3, None, None, None, None, None), -1, "null pointer"),
    ("composite-size", "gsr_composite", (0, 4) + (None,) * 13, -1, "bad image size 0x4"),
    ("composite-null", "gsr_composite", (4, 4) + (None,) * 13, -1, "null required layer"),
    ("pack_rgba8-size", "gsr_pack_rgba8", (None, None, None, 0, 4, None), -1, "bad image size 0x4"),
    ("pack_rgba8-null", "gsr_pack_rgba8", (None, None, None, 4, 4, None), -1, "null pointer"),
    ("view_normals-size", "gsr_view_normals", (-1, None, None, None, None, None), -1, "bad size P=-1"),
    ("normal_maps-size", "gsr_normal_maps", (0, 4, None, None, None, 1.0, 1.0, 0.0, 0.0, None, None, None), -1, "bad image size 0x4"),
    ("normal_maps-null", "gsr_normal_maps", (4, 4, None, None, None, 1.0, 1.0, 0.0, 0.0, None, None, None), -1, "null pointer"),
    ("place_object-size", "gsr_place_object", (-1,) + (None,) * 5 + (1, None) + (None,) * 7, -1, "bad size n=-1"),
    ("place_object-null", "gsr_place_object", (3,) + (None,) * 5 + (1, None) + (None,) * 7, -1, "null pointer"),
    ("place_object_subset-null", "gsr_place_object_subset", (2,) + (None,) * 6 + (1, None) + (None,) * 7, -1, "null subset"),
    ("selftest_exp", "gsr_selftest_exp", (0, 1, None, None), -1, "bad selftest arguments"),
    ("radix_sort-bits", "gsr_radix_sort_pairs", (5, 0, None, None, None, None, 0, None, 0, None, None), -1, "bad key width bits=0"),
    ("radix_sort-null", "gsr_radix_sort_pairs", (5, 8, None, None, None, None, 0, None, 0, None, None), -1, "null pointer"),
    ("selftest_lds", "gsr_selftest_lds_atomic_order", (0, 1, 1, None, None), -1, "bad selftest arguments"),
    ("resize_rgba8-size", "gsr_resize_rgba8_bilinear", (None, 0, 4, None, 4, 4, None, None), -1, "bad image size 0x4 -> 4x4"),
    ("resize_rgba8-null", "gsr_resize_rgba8_bilinear", (None, 8, 8, None, 4, 4, None, None), -1, "null pointer"),
    ("resize_f32-size", "gsr_resize_f32_nearest", (None, 4, 4, None, 4, -2, None), -1, "bad image size 4x4 -> 4x-2"),
    ("frame_files-size", "gsr_frame_files", (None,) * 4 + (1.0, None, 0, 4) + (None,) * 6, -1, "bad image size 0x4"),
    ("frame_files_deflate-null", "gsr_frame_files_deflate", (None,) * 4 + (1.0, None, 4, 4) + (None,) * 8, -1, "null pointer"),
    ("png_encode-channels", "gsr_png_encode", (None, 4, 4, 5, 0, None, None), -1,
     "gsr_png_encode: 4x4 with 5 channels cannot be encoded (3 or 4 channels, < 2 GB)"),
    ("png_encode-null", "gsr_png_encode", (None, 4, 4, 3, 0, None, None), -1, "null pointer"),
    ("png_encode_deflate-channels", "gsr_png_encode_deflate", (None, 4, 4, 2, 0, None, None, None, None), -1,
     "gsr_png_encode_deflate: 4x4 with 2 channels cannot be encoded (3 or 4 channels, < 2 GB)"),
    ("png_unfilter-width", "gsr_png_unfilter", (None, 5000, 4, 4, None, None, None), -1,
     "gsr_png_unfilter: job 0: 5000x4 with 4 channels is not supported (8-bit RGB / RGBA, at most 4096 pixels wide)"),
    ("png_unfilter-null", "gsr_png_unfilter", (None, 8, 4, 3, None, None, None), -1, "gsr_png_unfilter: job 0: null pointer"),
    ("png_unfilter_batch-list", "gsr_png_unfilter_batch", (-1, None, None), -1, "gsr_png_unfilter_batch: bad job list"),
    ("exr_unpack-layout", "gsr_exr_unpack_channel", (None, 0, 8, 1, 0, 2, None, None), -1,
     "gsr_exr_unpack_channel: bad layout (height 0, 8 bytes per line, 1 lines per block, channel at 0 + 2)"),
    ("exr_unpack-null", "gsr_exr_unpack_channel", (None, 4, 8, 1, 0, 2, None, None), -1, "null pointer"),
    ("inflate_zlib_blocks-count", "gsr_inflate_zlib_blocks", (None, None, None, -1, None, None, None), -1,
     "gsr_inflate_zlib_blocks: bad arguments"),
    ("png_file_probe-null", "gsr_png_file_probe", (None, 0, None), -1, "null pointer"),
    ("exr_file_pack-null", "gsr_exr_file_pack", (b"x", 1, None, None, 0, None, None), -1, "null pointer"),
    ("selftest_inflate_host-null", "gsr_selftest_inflate_host", (None, 0, None, 0), -1, "null pointer"),
    ("cube_to_equirect-width", "gsr_cube_to_equirect", (None, 8, 3, None, None, None, None, 8, 12, None, None, None, None), -1,
     "gsr_cube_to_equirect: the width (12) must be a positive multiple of 8"),
    ("cube_to_equirect-null", "gsr_cube_to_equirect", (None, 8, 3, None, None, None, None, 8, 16, None, None, None, None), -1,
     "null pointer"),
]


@pytest.mark.parametrize("name,args,status,message", [pytest.param(*c[1:], id=c[0]) for c in REFUSALS])
def test_refusals_keep_their_status_and_text(name, args, status, message):
    """The texts were recorded from the library before the entry points moved out of gsr_api.hip: a refusal from any unit
    sets the one message gsr_last_error() returns."""
    from autovfx_amd import _lib
    assert _lib.lib.gsr_set_option(-1, 0) == -1 and _lib.last_error() == "unknown option -1"   # a known message to overwrite
    assert getattr(_lib.lib, name)(*args) == status
    assert _lib.last_error() == message


def test_a_refusal_on_another_thread_keeps_its_own_message():
    """The message buffer is per thread and lives in one unit: a refusal from gsr_kernels.hip on a second thread is read back
    there, and the first thread still reads the refusal it got from gsr_radix.hip."""
    import threading
    from autovfx_amd import _lib
    assert _lib.lib.gsr_radix_sort_pairs(5, 0, None, None, None, None, 0, None, 0, None, None) == -1
    seen = {}

    def other():
        seen["before"] = _lib.last_error()
        seen["status"] = _lib.lib.gsr_pack_rgba8(None, None, None, 0, 4, None)
        seen["after"] = _lib.last_error()

    t = threading.Thread(target=other)
    t.start()
    t.join()
    assert seen == {"before": "", "status": -1, "after": "bad image size 0x4"}
    assert _lib.last_error() == "bad key width bits=0"
