"""autovfx_amd.texture on the GPU: the three kernels bit for bit against the numpy contract, one view against a torch restatement of the
reference's loop body (sampler, soft blend, the six index operations) on the same device, and the drop-in through install() against the
restated function on stub ``rc``, camera and pytorch3d names."""
import sys
import types

import numpy as np
import pytest
import torch

import texture_cases as TC
from autovfx_amd import texture

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), device=DEV)


def atlas_on_gpu(F, S):
    verts_uv, faces_uv, T, A, offs, bary = texture.atlas(F, S, DEV)
    return verts_uv, faces_uv, T, verts_uv[faces_uv]


# ---- a pixel's texel ----
@pytest.mark.parametrize("H,W,F", ((1, 1, 1), (37, 53, 3), (65, 64, 257)))
def test_texels_of_pixels_bit_for_bit(H, W, F):
    face_uvs, T = TC.face_uvs_of(F, 10)
    if H == 1:                                     # one pixel, inside its face
        pix, bary, zbuf = np.zeros((1, 1), np.int64), np.asarray([[[0.2, 0.3, 0.5]]], F32), np.full((1, 1), F32(3.0))
    else:
        pix, bary, zbuf, _ = (a.copy() for a in TC.fragments(F, H, W, seed=H + F))
    if H > 1:                                      # every kind of invalid pixel among the valid ones
        seen = np.argwhere(pix >= 0)
        assert len(seen) > 40
        for k, (r, c) in enumerate(seen[:: len(seen) // 12][:12]):
            if k % 4 == 0:
                pix[r, c] = F + k
            elif k % 4 == 1:
                zbuf[r, c] = (0.0, -2.0, np.nan)[(k // 4) % 3]
            elif k % 4 == 2:
                bary[r, c, k % 3] = np.nan
            else:
                bary[r, c] = (40.0, -20.0, -19.0)                       # far outside the face: the border texels
    want = texture.texels_of_pixels_host(pix, bary, zbuf, face_uvs, T)
    got = texture.texels_of_pixels(dev(pix), dev(bary), dev(zbuf), dev(face_uvs), T)
    assert got.dtype == torch.int32 and tuple(got.shape) == (H, W)
    assert np.array_equal(got.cpu().numpy().reshape(-1), want)
    assert (want >= 0).any() and (H == 1 or (want < 0).any())


def test_atlas_on_the_gpu():
    """``atlas`` on the device holds what the reference's statements give there: torch divides a tensor by a host number with one
    multiplication by its reciprocal on the GPU, so a value may sit one ulp from ``atlas_host``'s correctly rounded quotient."""
    for F, S in ((1, 4), (8, 10), (5001, 10)):
        got, same, host = texture.atlas(F, S, DEV), TC.atlas_restated_torch(F, S, DEV), texture.atlas_host(F, S)
        assert got[2:4] == same[2:4] == host[2:4]
        for g, w, h in zip((got[0], got[1], got[4], got[5]), (same[0], same[1], same[4], same[5]), (host[0], host[1], host[4], host[5])):
            assert g.device.type == "cuda" and g.dtype == w.dtype and torch.equal(g, w)
            if h.dtype == np.float32:
                # a quotient is one ulp off at most; a barycentric is 1 - (c_0 + c_1) of two such quotients below 4 (ulp 2^-22) and two
                # more roundings, so it may miss an exact 0 by a few 2^-22: compared absolutely
                off = np.abs(g.cpu().numpy().astype(np.float64) - h)
                bound = np.spacing(np.abs(h)).astype(np.float64) if h.shape[-1] == 2 else np.full(h.shape, 4 * 2.0 ** -22)
                print(f"atlas F={F} S={S} {list(h.shape)}: {int((off > 0).sum())} of {off.size} values off atlas_host, at most {off.max():.3g}")
                assert (off <= bound).all()
            else:
                assert np.array_equal(g.cpu().numpy(), h)


# ---- the fill ----
@pytest.mark.parametrize("S", (4, 10))
@pytest.mark.parametrize("G", (1, 3, 6))
@pytest.mark.parametrize("F", (1, 2, 3, 257, 5001))
def test_fill_bit_for_bit(F, G, S):
    verts, faces, centers, M, features = (a.copy() for a in TC.fill_case(F, G, seed=F + G))
    if F >= 3:
        centers[1 * G + (G - 1), 1] = np.nan       # face 1: a NaN q, at the last Gaussian
        if G > 1:
            M[(F - 1) * G + 1, 0, 0] = np.inf      # the last face: inf - inf somewhere in w
        faces[2, 2] = verts.shape[0]               # face 2 is out of range
        if F > 100:
            faces[F // 2, 0] = -1
    _, _, T, A, offs, bary = texture.atlas_host(F, S)
    want = texture.fill_host(verts, faces, centers, M, features, offs, bary, A, S)
    got = texture.fill(dev(verts), dev(faces), dev(centers), dev(M), dev(features), dev(offs), dev(bary), A, S)
    assert tuple(got.shape) == (T, T, 3)
    assert np.array_equal(got.cpu().numpy(), want, equal_nan=True)
    owned = TC.owned_texels(F, S, A, offs)
    assert (want.reshape(-1, 3)[owned[0]] != 0.5).any()
    if F >= 3:
        assert (want.reshape(-1, 3)[owned[2]] == 0.5).all()
        assert np.array_equal(want.reshape(-1, 3)[owned[1]], np.tile(features[1 * G + G - 1] * F32(texture.SH_C0) + F32(0.5), (owned.shape[1], 1)))


# ---- one view ----
def bake_on_gpu(views, face_uvs, T, fill, strided=False):
    """``views``: (fragments, rgb [H, W, 3]).  Returns tex, count and whether the owner buffer was clean after every view."""
    tex, count, owner = dev(fill), torch.zeros((T, T), device=DEV), texture.new_owner(T, DEV)
    clean = []
    for (pix, bary, zbuf, _), rgb in views:
        image = dev(rgb)
        if strided:                                # the colours as the first three channels of an RGBA image
            rgba = torch.full(image.shape[:-1] + (4,), 7.0, device=DEV)
            rgba[..., :3] = image
            image = rgba[..., :3]
            assert not image.is_contiguous()
        texture.bake_view(tex, count, owner, image, dev(pix), dev(bary), dev(zbuf), face_uvs)
        clean.append(bool((owner == -1).all()))
    return tex.cpu().numpy(), count.cpu().numpy(), clean


def bake_on_host(views, face_uvs, T, fill):
    tex, count = fill, np.zeros((T, T), F32)
    for (pix, bary, zbuf, _), rgb in views:
        tex, count = texture.bake_view_host(tex, count, rgb, pix, bary, zbuf, face_uvs)
    return tex, count


def three_views(F, H, W, collide, zlo=2.0, zhi=40.0):
    face_uvs, T = TC.face_uvs_of(F, 10)
    views = []
    for v in range(3):
        fr = TC.fragments(F, H, W, seed=31 + v, radius=0.7, zlo=zlo, zhi=zhi)
        views.append((fr if collide else TC.thinned(fr, face_uvs, T), TC.colours(H, W, seed=v)))
    fill = np.random.default_rng(9).uniform(0, 1, (T, T, 3)).astype(F32)
    return views, face_uvs, T, fill


@pytest.mark.parametrize("collide,strided", ((True, False), (False, False), (True, True)))
def test_bake_view_bit_for_bit(collide, strided):
    F, H, W = (3, 65, 64) if collide else (257, 65, 64)
    views, face_uvs, T, fill = three_views(F, H, W, collide)
    texels = [texture.texels_of_pixels_host(fr[0], fr[1], fr[2], face_uvs, T) for fr, _ in views]
    seen = [t[t >= 0] for t in texels]
    if collide:                                    # heavy: ten pixels and more per texel
        assert all(len(s) > 10 * len(np.unique(s)) for s in seen)
    else:
        assert all(len(s) == len(np.unique(s)) and len(s) > 300 for s in seen)
    assert len(np.intersect1d(seen[0], seen[1])) > 0                    # texels that sum over views
    want_tex, want_count = bake_on_host(views, face_uvs, T, fill)
    got_tex, got_count, clean = bake_on_gpu(views, dev(face_uvs), T, fill, strided)
    assert clean == [True, True, True]
    assert np.array_equal(got_count, want_count) and want_count.max() >= 2
    assert np.array_equal(got_tex, want_tex)
    again_tex, again_count, _ = bake_on_gpu(views, dev(face_uvs), T, fill, strided)
    assert np.array_equal(again_tex, got_tex) and np.array_equal(again_count, got_count)


def test_bake_view_direct_calls_say_why_not(monkeypatch):
    face_uvs, T = TC.face_uvs_of(3, 10)
    pix, bary, zbuf, _ = TC.fragments(3, 37, 53, seed=1)
    tex, count, owner = torch.zeros(T, T, 3, device=DEV), torch.zeros(T, T, device=DEV), texture.new_owner(T, DEV)
    rgb, uv = dev(TC.colours(37, 53, 0)), dev(face_uvs)
    args = dict(tex=tex, count=count, owner=owner, rgb=rgb, pix_to_face=dev(pix), bary=dev(bary), zbuf=dev(zbuf), face_uvs=uv)
    for change, word in ((dict(rgb=rgb.cpu()), "must be on a GPU"), (dict(rgb=rgb.double()), "float32"), (dict(owner=owner.long()), "int32"),
                         (dict(count=count[:-1]), "count must be"), (dict(tex=tex.permute(1, 0, 2)[:, :, :]), "tex must be|contiguous"),
                         (dict(zbuf=dev(zbuf)[:-1]), "zbuf must hold"), (dict(rgb=rgb[:-1]), "rgb must hold"), (dict(face_uvs=uv[:, :, :1]), "face_uvs must be"),
                         (dict(pix_to_face=dev(pix).int()), "int64")):
        with pytest.raises(ValueError, match=word):
            texture.bake_view(**{**args, **change})
    assert bool((owner == -1).all()) and float(count.sum()) == 0.0
    from autovfx_amd import _lib
    monkeypatch.setattr(_lib, "capturing", lambda: True)
    with pytest.raises(ValueError, match="capturing"):
        texture.bake_view(**args)
    with pytest.raises(ValueError, match="capturing"):
        texture.texels_of_pixels(args["pix_to_face"], args["bary"], args["zbuf"], uv, T)


# ---- against the reference's loop body, restated in torch on the same device ----
def reference_on_gpu(views, verts_uv, faces_uv, T, fill):
    tex, counter = dev(fill), torch.zeros((T, T, 1), device=DEV)
    targets = []
    for fr, rgb in views:
        pix, bary, zbuf, dists = TC.as_fragments(fr, DEV)
        targets.append(TC.reference_view(tex, counter, dev(rgb), pix, bary, zbuf, dists, verts_uv, faces_uv).cpu().numpy())
    return tex.cpu().numpy(), counter[..., 0].cpu().numpy(), targets


def test_one_view_against_the_restated_loop_body_without_collisions():
    F, H, W = 257, 65, 64
    views, face_uvs, T, fill = three_views(F, H, W, collide=False)
    assert max(float(fr[2].max()) for fr, _ in views) < 50
    verts_uv, faces_uv, T_gpu, face_uvs_gpu = atlas_on_gpu(F, 10)
    assert T_gpu == T
    want_tex, want_count, _ = reference_on_gpu(views, verts_uv, faces_uv, T, fill)
    got_tex, got_count, _ = bake_on_gpu(views, face_uvs_gpu, T, fill)
    assert np.array_equal(got_count, want_count) and want_count.max() >= 2 and (want_count == 0).any()
    assert np.array_equal(got_tex, want_tex)


def test_one_view_against_the_restated_loop_body_with_collisions():
    """``count`` is the reference's everywhere; which of a texel's pixels gives the colour is open there and the lowest here: each
    texel holds the colour of one of the pixels the restated shader sends to it."""
    F, H, W = 3, 65, 64
    views, face_uvs, T, fill = three_views(F, H, W, collide=True)
    verts_uv, faces_uv, _, face_uvs_gpu = atlas_on_gpu(F, 10)
    for fr, rgb in views:
        want_tex, want_count, targets = reference_on_gpu([(fr, rgb)], verts_uv, faces_uv, T, fill)
        got_tex, got_count, _ = bake_on_gpu([(fr, rgb)], face_uvs_gpu, T, fill)
        assert np.array_equal(got_count, want_count)
        texel = targets[0][:, 0] * T + targets[0][:, 1]                 # per valid pixel, in pixel order: where the reference's shader sends it
        colour = rgb[fr[2] > 0]
        ours = got_tex.reshape(-1, 3)
        for t in np.unique(texel):
            assert (colour[texel == t] == ours[t]).all(axis=1).any(), t
        untouched = np.ones(T * T, bool)
        untouched[texel] = False
        assert np.array_equal(ours[untouched], fill.reshape(-1, 3)[untouched])
        assert np.array_equal(want_tex.reshape(-1, 3)[untouched], fill.reshape(-1, 3)[untouched])


def test_a_far_view_votes_for_its_own_texels():
    """Depths about ``zfar`` and beyond (difference 2): pinned to the numpy contract."""
    F, H, W = 3, 37, 53
    face_uvs, T = TC.face_uvs_of(F, 10)
    fr = TC.fragments(F, H, W, seed=4, radius=0.7, zlo=99.8, zhi=160.0)
    assert float(fr[2].max()) > 100 and (fr[0] >= 0).sum() > 100
    views = [(fr, TC.colours(H, W, seed=3))]
    fill = np.full((T, T, 3), F32(0.5))
    want_tex, want_count = bake_on_host(views, face_uvs, T, fill)
    got_tex, got_count, clean = bake_on_gpu(views, dev(face_uvs), T, fill)
    assert clean == [True] and np.array_equal(got_count, want_count) and np.array_equal(got_tex, want_tex) and want_count.sum() > 10


# ---- the drop-in through install(), on a module shaped like the reference's ----
@pytest.fixture
def installed():
    import autovfx_amd
    mod = types.ModuleType("stubtexturegpu.sugar_model")
    original = mod.extract_texture_image_and_uv_from_gaussians = TC.extract_texture_image_and_uv_from_gaussians
    mod.SuGaR = TC.StubModel
    sys.modules[mod.__name__] = mod
    try:
        autovfx_amd.install(path=False)
        assert mod.reference_extract_texture_image_and_uv_from_gaussians is original
        assert TC.extract_texture_image_and_uv_from_gaussians is mod.extract_texture_image_and_uv_from_gaussians is not original   # (an importer: rebound)
        yield mod
    finally:
        autovfx_amd.uninstall()
        sys.modules.pop(mod.__name__, None)
    assert mod.extract_texture_image_and_uv_from_gaussians is original and TC.extract_texture_image_and_uv_from_gaussians is original


@pytest.mark.parametrize("F,G,S", ((7, 3, 10), (257, 6, 4)))
def test_drop_in_through_install_against_the_restated_function(F, G, S, installed):
    rc = TC.StubModel(F=F, G=G, S=S, views=3, H=65, W=64, seed=F, device=DEV)
    # the scene: the nearest Gaussian of every texel is clear of the others in the reference's exp(-q / 2) too -- the next one has 4 q,
    # and exp(-q / 2) and exp(-2 q) are thousands of ulps apart from q = 1e-4 up to where the latter underflows
    verts, faces = (t.cpu().numpy() for t in (rc.surface_mesh.verts_list()[0], rc.surface_mesh.faces_list()[0]))
    _, _, T, A, offs, bary = texture.atlas_host(F, S)
    _, q = texture.fill_host(verts, faces, rc.points.cpu().numpy(), rc._M.cpu().numpy(), rc.sh_coordinates[:, 0].cpu().numpy(), offs, bary, A, S,
                             return_q=True)
    assert q[..., -1].min() > 1e-4 and q[..., -1].max() < 150
    with torch.no_grad():
        rasterized = TC.MeshRasterizer.calls
        got = installed.extract_texture_image_and_uv_from_gaussians(rc, square_size=S)
        assert TC.MeshRasterizer.calls == rasterized + 3
        assert rc.render_calls == [(0, 0, True), (1, 0, True), (2, 0, True)]
        want = installed.reference_extract_texture_image_and_uv_from_gaussians(rc, square_size=S)
    assert len(got) == len(want) == 3
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.device == w.device and tuple(g.shape) == tuple(w.shape)
        assert torch.equal(g, w)
    texture_img = got[2].cpu().numpy()
    assert tuple(texture_img.shape) == (T, T, 3) and len(np.unique(texture_img.reshape(-1, 3), axis=0)) > 100
    # with autograd on the call is the reference's: the same values here, no kernel of ours
    again = installed.extract_texture_image_and_uv_from_gaussians(rc, square_size=S)
    assert torch.equal(again[2], want[2])
