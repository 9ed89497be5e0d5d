"""autovfx_amd.texture without a GPU: the numpy contract (atlas, a pixel's texel, one view, the fill) against independent restatements of
the reference, the hook's row on a stub ``sugar_model``, and what the C entry points refuse."""
import ctypes
import sys
import types

import numpy as np
import pytest
import torch

import texture_cases as TC
from autovfx_amd import texture

F32 = np.float32


# ---- the atlas ----
@pytest.mark.parametrize("S", (4, 10))
@pytest.mark.parametrize("F", (1, 2, 3, 7, 8, 5001))
def test_atlas_host_against_the_restatement(F, S):
    got, want = texture.atlas_host(F, S), TC.atlas_restated(F, S)
    verts_uv, faces_uv, T, A, offs, bary = got
    n = S * (S - 1) // 2
    assert (T, A) == (want[2], want[3]) and T == S * A and A * A > F // 2
    assert verts_uv.shape == (6 * A * A, 2) and verts_uv.dtype == np.float32
    assert faces_uv.shape == (F, 3) and faces_uv.dtype == np.int64
    assert offs.shape == (2, n, 2) and offs.dtype == np.int32 and bary.shape == (2, n, 3) and bary.dtype == np.float32
    for g, w in zip((verts_uv, faces_uv, offs, bary), (want[0], want[1], want[4], want[5])):
        assert np.array_equal(g, w)
    owned = TC.owned_texels(F, S, A, offs).reshape(-1)
    assert owned.min() >= 0 and owned.max() < T * T and np.unique(owned).size == owned.size       # every face's texels are its own


@pytest.mark.parametrize("S", (4, 10))
def test_atlas_torch_equals_atlas_host(S):
    for F in (1, 8, 5001):
        got, want = texture.atlas(F, S, "cpu"), texture.atlas_host(F, S)
        assert got[2:4] == want[2:4]
        for g, w in zip((got[0], got[1], got[4], got[5]), (want[0], want[1], want[4], want[5])):
            assert g.dtype == torch.from_numpy(w).dtype and np.array_equal(g.numpy(), w)


@pytest.mark.parametrize("S", (4, 10))
@pytest.mark.parametrize("F", (1, 2, 3, 7, 8, 5001))
def test_table_barycentrics_at_the_corner_texels(F, S):
    """Where a table's barycentrics are a unit vector, the texel is a UV corner of the face or its neighbour: the first corner exactly;
    in the bottom table the second one texel to the left and the third one texel up; the top table weighs the face's third UV corner with
    its second barycentric (one texel to the right) and the second with its third (one texel down).  These are the reference's values
    (sugar_model.py:2463-2468 against :2497-2510): its tables are not the exact inverse of its UV layout."""
    verts_uv, faces_uv, T, A, offs, bary = texture.atlas_host(F, S)
    expect = {0: ((0, (0, 0)), (1, (-1, 0)), (2, (0, 1))), 1: ((0, (0, 0)), (2, (1, 0)), (1, (0, -1)))}
    for f in sorted({0, F // 2, F - 1}):
        sq = f >> 1
        origin = np.asarray([sq // A, sq % A]) * S
        corners = np.rint(verts_uv[faces_uv[f]] * F32(T)).astype(np.int64) - origin               # the UV corners, in texels of the square
        for k, (corner, step) in enumerate(expect[f & 1]):
            unit = np.nonzero((bary[f & 1] == np.eye(3, dtype=F32)[k]).all(axis=1))[0]
            assert unit.size == 1
            assert tuple(offs[f & 1, unit[0]]) == tuple(corners[corner] + np.asarray(step)), (f, k)


# ---- a pixel's texel ----
def grid_sample_chain(uv, T):
    """uv [P, 2] -> (row, col) by torch on the CPU: the flipped index map sampled with ``nearest``, ``border``, ``align_corners=True``."""
    index_map = torch.cartesian_prod(torch.arange(T), torch.arange(T)).reshape(T, T, 2).float()[None]
    maps = torch.flip(index_map.permute(0, 3, 1, 2), [2])
    grid = (torch.from_numpy(uv) * 2.0 - 1.0).reshape(1, -1, 1, 2)
    out = torch.nn.functional.grid_sample(maps, grid, mode="nearest", align_corners=True, padding_mode="border")
    return out[0, :, :, 0].round().long().numpy().T


@pytest.mark.parametrize("T", (30, 57, 1000))
def test_texels_of_pixels_host_against_grid_sample(T):
    g = np.random.default_rng(T)
    P = 20000
    uv = g.uniform(-0.2, 1.2, (P, 2)).astype(F32)
    half = ((g.integers(0, T, (P // 4, 2)) + 0.5) / (T - 1)).astype(F32)        # texel coordinates at, or an ulp from, a half-integer
    uv[: P // 4] = half
    uv[P // 4: P // 2] = np.nextafter(half, F32(2) * g.integers(0, 2, half.shape).astype(F32))
    # one face per pixel whose three UV corners are the pixel's uv: any barycentrics that are exact keep it
    pix = np.arange(P, dtype=np.int64)
    face_uvs = np.repeat(uv[:, None, :], 3, axis=1)
    bary = np.tile(np.asarray([0.5, 0.25, 0.25], F32), (P, 1))
    got = texture.texels_of_pixels_host(pix, bary, np.ones(P, F32), face_uvs, T)
    want = grid_sample_chain(uv, T)
    assert np.array_equal(got, want[:, 0] * T + want[:, 1])
    assert len(np.unique(got)) > min(P, T * T) // 4


def test_invalid_pixels_have_no_texel():
    face_uvs = np.asarray([[[0.1, 0.1], [0.9, 0.1], [0.5, 0.9]]] * 2, F32)
    pix = np.asarray([0, 1, -1, 2, 0, 0, 0, 0, 1], np.int64)
    zbuf = np.asarray([1, 1, 1, 1, 0, -1, np.nan, 2, np.inf], F32)
    bary = np.tile(np.asarray([0.2, 0.3, 0.5], F32), (9, 1))
    bary[7, 1] = np.nan
    got = texture.texels_of_pixels_host(pix, bary, zbuf, face_uvs, 16)
    assert (got[[2, 3, 4, 5, 6, 7]] == -1).all() and (got[[0, 1, 8]] >= 0).all() and got[0] == got[1] == got[8]


# ---- one view ----
def one_face_view(pixels):
    """A view whose pixels all see face 0 of a two-face atlas at chosen uv: (pix, bary, zbuf, face_uvs, T, texel of each pixel)."""
    face_uvs, T = TC.face_uvs_of(2, 10)
    bary = np.asarray(pixels, F32)
    pix, zbuf = np.zeros(len(pixels), np.int64), np.ones(len(pixels), F32)
    return pix, bary, zbuf, face_uvs, T, texture.texels_of_pixels_host(pix, bary, zbuf, face_uvs, T)


def test_bake_view_host_collisions_first_visits_sums_and_invalid_pixels():
    corners = np.eye(3, dtype=F32)
    pix, bary, zbuf, face_uvs, T, texel = one_face_view([corners[0], corners[1], corners[0], corners[2], corners[0], corners[1]])
    assert texel[0] == texel[2] == texel[4] and texel[1] == texel[5] and len({texel[0], texel[1], texel[3]}) == 3
    rgb = np.arange(18, dtype=F32).reshape(6, 3) + 1
    fill = np.full((T, T, 3), F32(0.5))
    fill.reshape(-1, 3)[texel[0]] = np.nan         # a NaN fill is dropped on the first visit like any other (difference 4)
    tex, count = texture.bake_view_host(fill, np.zeros((T, T), F32), rgb, pix, bary, zbuf, face_uvs)
    flat = tex.reshape(-1, 3)
    # collisions go to the lowest pixel, and a first visit drops the fill
    assert np.array_equal(flat[texel[0]], rgb[0]) and np.array_equal(flat[texel[1]], rgb[1]) and np.array_equal(flat[texel[3]], rgb[3])
    assert count.sum() == 3 and (count.reshape(-1)[texel[[0, 1, 3]]] == 1).all()
    untouched = np.ones(T * T, bool)
    untouched[texel] = False
    assert np.array_equal(flat[untouched], fill.reshape(-1, 3)[untouched], equal_nan=True)
    # a second view on one of the texels sums in order
    tex2, count2 = texture.bake_view_host(tex, count, rgb[::-1], pix[:1], bary[:1], zbuf[:1], face_uvs)
    assert np.array_equal(tex2.reshape(-1, 3)[texel[0]], rgb[0] + rgb[5]) and count2.reshape(-1)[texel[0]] == 2
    assert np.array_equal(tex2.reshape(-1, 3)[texel[1]], rgb[1])
    # invalid pixels touch nothing
    bad_pix = np.asarray([-1, 2, 0, 0, 0], np.int64)
    bad_z = np.asarray([1, 1, 0, -3, np.nan], F32)
    tex3, count3 = texture.bake_view_host(tex2, count2, rgb[:5], bad_pix, bary[:5], bad_z, face_uvs)
    assert np.array_equal(tex3, tex2, equal_nan=True) and np.array_equal(count3, count2)


# ---- the fill ----
@pytest.mark.parametrize("F,G,S", ((1, 1, 4), (2, 3, 10), (3, 6, 4), (257, 3, 10), (257, 6, 4), (5001, 1, 10), (5001, 6, 10)))
def test_fill_host_against_the_reference_restatement(F, G, S):
    verts, faces, centers, M, features = TC.fill_case(F, G, seed=F + G)
    _, _, T, A, offs, bary = texture.atlas_host(F, S)
    got, q = texture.fill_host(verts, faces, centers, M, features, offs, bary, A, S, return_q=True)
    t = torch.tensor
    want = TC.fill_restated(t(verts), t(faces), t(centers), t(M), t(features), t(offs), t(bary), A, S).numpy()
    # compared: the texels whose two best q differ by more than 1e-5 relative (all of them at G = 1), and every texel no face owns
    if G > 1:
        two = np.sort(q, axis=-1)[..., :2]
        clear = (two[..., 1] - two[..., 0]) > 1e-5 * two[..., 1]
    else:
        clear = np.ones(q.shape[:2], bool)
    assert clear.mean() >= 0.99
    compare = np.ones(T * T, bool)
    compare[TC.owned_texels(F, S, A, offs)[~clear]] = False
    assert np.array_equal(got.reshape(-1, 3)[compare], want.reshape(-1, 3)[compare])
    owned = np.zeros(T * T, bool)
    owned[TC.owned_texels(F, S, A, offs).reshape(-1)] = True
    assert (got.reshape(-1, 3)[~owned] == 0.5).all()


def test_fill_host_nan_q_and_out_of_range_faces():
    F, G, S = 4, 3, 4
    verts, faces, centers, M, features = (a.copy() for a in TC.fill_case(F, G, seed=5))
    _, _, T, A, offs, bary = texture.atlas_host(F, S)
    centers[1 * G + 1, 0] = np.nan                 # face 1: the first NaN q wins, here Gaussian 1 ...
    centers[1 * G + 2, 2] = np.nan                 # ... not Gaussian 2
    faces[2, 1] = verts.shape[0]                   # face 2 writes nothing
    faces[3, 0] = -1                               # nor does face 3
    got = texture.fill_host(verts, faces, centers, M, features, offs, bary, A, S).reshape(-1, 3)
    owned = TC.owned_texels(F, S, A, offs)
    assert np.array_equal(got[owned[1]], np.tile(features[1 * G + 1] * F32(texture.SH_C0) + F32(0.5), (owned.shape[1], 1)))
    assert (got[owned[2]] == 0.5).all() and (got[owned[3]] == 0.5).all() and (got[owned[0]] != 0.5).any()


# ---- the hook's row ----
def _stub_module(calls, name="stubtexture.sugar_model"):
    mod = types.ModuleType(name)

    def extract_texture_image_and_uv_from_gaussians(rc, square_size=10, n_sh=-1, texture_with_gaussian_renders=True):
        if square_size < 3:
            raise ValueError("square_size must be >= 3")
        calls.append((square_size, n_sh, texture_with_gaussian_renders))
        return "reference texture"

    mod.extract_texture_image_and_uv_from_gaussians = extract_texture_image_and_uv_from_gaussians
    mod.SuGaR = type("SuGaR", (), {})
    return mod


def test_install_and_uninstall_on_a_stub_sugar_model():
    import autovfx_amd
    from autovfx_amd import hook
    calls = []
    mod = _stub_module(calls)
    importer = types.ModuleType("stubtexture.refined_mesh")
    original = importer.extract_texture_image_and_uv_from_gaussians = mod.extract_texture_image_and_uv_from_gaussians
    bare = types.ModuleType("stubtexture_bare.sugar_model")              # no SuGaR beside the function: not the reference's module
    bare.extract_texture_image_and_uv_from_gaussians = lambda rc: "untouched"
    kept = bare.extract_texture_image_and_uv_from_gaussians
    for m in (mod, importer, bare):
        sys.modules[m.__name__] = m
    try:
        autovfx_amd.install(path=False)
        ours = mod.extract_texture_image_and_uv_from_gaussians
        assert ours is not original and mod.reference_extract_texture_image_and_uv_from_gaussians is original and ours.fallback is original
        assert importer.extract_texture_image_and_uv_from_gaussians is ours                       # refined_mesh.py:9 imports it by name
        assert bare.extract_texture_image_and_uv_from_gaussians is kept
        assert mod.__name__ in hook.patched_modules
        # refused calls reach the original with the caller's arguments: a CPU model, no Gaussian renders, square sizes outside 4..32
        cpu = TC.StubModel(F=3, G=2, S=4, views=1, H=8, W=8, seed=1, device="cpu")
        with torch.no_grad():
            assert ours(cpu, square_size=4) == "reference texture"
            assert ours(cpu, 10, 2, False) == "reference texture"
            assert ours(cpu, square_size=3, n_sh=1) == "reference texture"
            with pytest.raises(ValueError, match="square_size must be >= 3"):
                ours(cpu, square_size=2)
        assert ours(cpu) == "reference texture"                                                   # autograd on
        assert calls == [(4, -1, True), (10, 2, False), (3, 1, True), (10, -1, True)] and cpu.render_calls == []
    finally:
        autovfx_amd.uninstall()
        for m in (mod, importer, bare):
            sys.modules.pop(m.__name__, None)
    assert mod.extract_texture_image_and_uv_from_gaussians is original and importer.extract_texture_image_and_uv_from_gaussians is original
    assert not hasattr(mod, "reference_extract_texture_image_and_uv_from_gaussians")


def test_direct_calls_say_why_not():
    face_uvs, T = TC.face_uvs_of(2, 4)
    pix, bary, zbuf = torch.zeros(4, dtype=torch.int64), torch.zeros(4, 3), torch.ones(4)
    uv = torch.tensor(face_uvs)
    with pytest.raises(ValueError, match="must be on a GPU"):
        texture.texels_of_pixels(pix, bary, zbuf, uv, T)
    with pytest.raises(ValueError, match="must be a torch.Tensor"):
        texture.texels_of_pixels(pix.numpy(), bary, zbuf, uv, T)
    with pytest.raises(ValueError, match="must be on a GPU"):
        texture.bake_view(torch.zeros(T, T, 3), torch.zeros(T, T), texture.new_owner(T, "cpu"), torch.zeros(4, 3), pix, bary, zbuf, uv)
    verts, faces, centers, M, features = (torch.tensor(a) for a in TC.fill_case(2, 2, seed=0))
    _, _, _, A, offs, wts = texture.atlas(2, 4, "cpu")
    with pytest.raises(ValueError, match="must be on a GPU"):
        texture.fill(verts, faces, centers, M, features, offs, wts, A, 4)
    with pytest.raises(ValueError, match="square_size"):
        texture.atlas(2, 3, "cpu")


# ---- what the C entry points refuse (before any launch: no device needed) ----
def test_c_abi_refusals():
    from autovfx_amd import _lib
    L = _lib.lib
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    views = {"gsr_texture_texels": lambda **k: L.gsr_texture_texels(k.get("P", 4), k.get("F", 2), k.get("T", 8), k.get("pix", p), k.get("bary", p),
                                                                     k.get("zbuf", p), k.get("uv", p), k.get("out", p), None),
             "gsr_texture_bake_view": lambda **k: L.gsr_texture_bake_view(k.get("P", 4), k.get("F", 2), k.get("T", 8), k.get("pix", p), k.get("bary", p),
                                                                           k.get("zbuf", p), k.get("uv", p), k.get("rgb", p), k.get("stride", 3),
                                                                           k.get("tex", p), k.get("count", p), k.get("owner", p), None)}
    for name, call in views.items():
        for bad, word in ((dict(P=-1), "negative"), (dict(F=-1), "negative"), (dict(P=(1 << 32) - 1), "2^32 - 2"), (dict(F=1 << 31), "2^31"),
                          (dict(T=0), "texture_size"), (dict(T=46341), "texture_size"), (dict(pix=None), "null"), (dict(bary=None), "null"),
                          (dict(zbuf=None), "null"), (dict(uv=None), "null"), (dict(pix=p + 4), "misaligned"), (dict(bary=p + 2), "misaligned"),
                          (dict(uv=p + 1), "misaligned")):
            assert call(**bad) == -1 and word in _lib.last_error() and name in _lib.last_error(), (name, bad, _lib.last_error())
        assert call(P=0) == 0                                          # nothing to do: nothing launched
    assert views["gsr_texture_texels"](out=None) == -1 and "null" in _lib.last_error()
    assert views["gsr_texture_texels"](out=p + 2) == -1 and "misaligned" in _lib.last_error()
    bake = views["gsr_texture_bake_view"]
    for bad, word in ((dict(stride=2), "rgb_stride"), (dict(stride=1 << 31), "rgb_stride"), (dict(rgb=None), "null"), (dict(tex=None), "null"),
                      (dict(count=None), "null"), (dict(owner=None), "null"), (dict(owner=p + 2), "misaligned"), (dict(rgb=p + 3), "misaligned")):
        assert bake(**bad) == -1 and word in _lib.last_error(), (bad, _lib.last_error())
    assert bake(F=0, uv=None) == 0                                     # no face: every pixel is invalid, nothing launched

    def fill(**k):
        return L.gsr_texture_fill(k.get("V", 4), k.get("F", 2), k.get("G", 2), k.get("A", 2), k.get("S", 4), k.get("n", 6), k.get("verts", p),
                                  k.get("faces", p), k.get("centers", p), k.get("M", p), k.get("features", p), k.get("offs", p),
                                  k.get("bary", p), k.get("tex", p), None)

    for bad, word in ((dict(V=-1), "negative"), (dict(F=-1), "negative"), (dict(F=1 << 28), "2^28"), (dict(V=1 << 31), "2^31"), (dict(G=0), "G ="),
                      (dict(G=9), "G ="), (dict(S=3), "S ="), (dict(S=33), "S ="), (dict(A=0), "A ="), (dict(A=11586, F=2), "A ="),
                      (dict(F=9, A=2), "squares"), (dict(n=0), "n ="), (dict(n=17), "n ="), (dict(verts=None), "null"), (dict(faces=None), "null"),
                      (dict(centers=None), "null"), (dict(M=None), "null"), (dict(features=None), "null"), (dict(offs=None), "null"),
                      (dict(bary=None), "null"), (dict(tex=None), "null"), (dict(faces=p + 4), "misaligned"), (dict(tex=p + 2), "misaligned"),
                      (dict(offs=p + 1), "misaligned")):
        assert fill(**bad) == -1 and word in _lib.last_error() and "gsr_texture_fill" in _lib.last_error(), (bad, _lib.last_error())
