"""The GPU PNG deflate encoder against its host restatement, byte for byte, and the frame writer's batch path and preview kernel.

The cases and what each of them reaches are png_deflate_cases.py's and are asserted, without a GPU, in test_png_deflate.py.  Here the
kernels must return exactly the restatement's file: every token, every code length, every block's type and place, both checksums."""
import io

import numpy as np
import pytest
import torch

import png_deflate_cases as cases
from autovfx_amd import frame_io

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_behind():
    """The cases' files and traces (tens of MB) and the writers' pinned slots go when this module is done."""
    yield
    cases.case.cache_clear()
    cases.case_image.cache_clear()
    frame_io.release_cached_slots()


def _gpu_file(img: np.ndarray, planar: bool = False) -> bytes:
    src = torch.from_numpy(np.array(img)).cuda()           # (a copy: the cases are read-only)
    if planar:
        src = src.permute(2, 0, 1).contiguous()
    return frame_io.encode_png_gpu_deflate(src, planar=planar).cpu().numpy().tobytes()


def _assert_same_file(got: bytes, want: bytes, label: str, trace=None):
    at = cases.first_difference(got, want)
    if at is None:
        return
    where = ""
    if trace is not None:
        inside = [(i, b) for i, b in enumerate(trace["blocks"]) if b["offset"] <= at < b["offset"] + b["size"]]
        where = f", in block {inside[0][0]} ({inside[0][1]['type']}, from {inside[0][1]['offset']})" if inside else ", outside the deflate blocks"
    raise AssertionError(f"{label}: {len(got)} bytes against the restatement's {len(want)}, first difference at offset {at}{where}: "
                         f"{got[at:at + 8].hex()} != {want[at:at + 8].hex()}")


def _check_case(case_id: str, planar: bool = False):
    img, want, trace = cases.case(case_id)
    h, w, c = img.shape
    got = _gpu_file(img, planar)
    assert len(got) <= frame_io.png_deflate_max_size(w, h, c)
    _assert_same_file(got, want, f"{case_id} planar={planar}", trace)


@pytest.mark.parametrize("case_id", [i for i in cases.SINGLE_IDS if not i.startswith("rows:")])
def test_one_row_case_is_the_restatements_file(case_id):
    _check_case(case_id)


@pytest.mark.parametrize("planar", [False, True])
@pytest.mark.parametrize("case_id", [i for i in cases.SINGLE_IDS if i.startswith("rows:")])
def test_multi_row_case_is_the_restatements_file(case_id, planar):
    _check_case(case_id, planar)


def test_phase_family_is_the_restatements_file():
    """Block 0 ending in every bit phase, block 1 starting and ending in every byte phase of a word (asserted in test_png_deflate.py)."""
    for j in range(cases.PHASE_FAMILY):
        _check_case(f"phase{j}")


# ---- the batch path and the preview kernel: one built frame -------------------------------------------------------------------------

H, W = 80, 64          # the RGBA stream is two deflate blocks, each RGB stream one: the three jobs of one launch have different grids
N_FRAMES = 5


def _depth_index(d: np.ndarray) -> np.ndarray:
    """uint8(clip(d / 3, 0, 1) * 255) in fp32, operation by operation."""
    assert d.dtype == np.float32
    q = d / np.float32(3.0)
    q = np.minimum(np.maximum(q, np.float32(0.0)), np.float32(1.0)) * np.float32(255.0)
    assert q.dtype == np.float32
    return q.astype(np.uint8)


def _normal_byte(n: np.ndarray) -> np.ndarray:
    """uint8((n + 1) / 2 * 255) in fp32, operation by operation."""
    assert n.dtype == np.float32
    v = (n + np.float32(1.0)) / np.float32(2.0) * np.float32(255.0)
    assert v.dtype == np.float32
    return v.astype(np.uint8)


def _edge_values(quantise, centre_of, lo, hi):
    """For every k in 1 .. 255 the fp32 values on both sides of the edge where ``quantise`` steps to k, two on either side, found by
    stepping with nextafter from ``centre_of(k)``; those outside [lo, hi] are left out.  Also returns how many edges were found."""
    f32 = np.float32
    up, down = (lambda v: np.nextafter(v, f32(np.inf))), (lambda v: np.nextafter(v, f32(-np.inf)))
    q = lambda v: int(quantise(np.array([v], f32))[0])
    c0 = f32(centre_of(0))                                   # nothing steps to 0: the values around where 0 begins
    out, edges = [down(down(c0)), down(c0), c0, up(c0), up(up(c0))], 0
    for k in range(1, 256):
        x = f32(centre_of(k))
        while q(x) >= k:
            x = down(x)
        while q(x) < k:
            x = up(x)                                        # x: the smallest value that quantises to k
        assert q(down(x)) == k - 1 and q(x) == k
        edges += 1
        out += [down(down(x)), down(x), x, up(x)]
    out = np.array(out, f32)
    return out[(out >= lo) & (out <= hi)], edges


def _built_frame():
    g = np.random.default_rng(7)
    d_edges, n_d = _edge_values(_depth_index, lambda k: 3.0 * k / 255.0, np.float32(-np.inf), np.float32(np.inf))
    n_edges, n_n = _edge_values(_normal_byte, lambda k: 2.0 * k / 255.0 - 1.0, np.float32(-1.0), np.float32(1.0))
    assert n_d == 255 and n_n == 255 and len(d_edges) == 1025 and len(n_edges) >= 1020
    special_d = np.array([0.0, -0.0, -1.5, -1e30, 3.0, 3.5, 1e30, np.inf, -np.inf], np.float32)
    # the edge values fill the first rows; behind them a slow ramp and one normal, so that these two images compress (dynamic blocks)
    depth = (np.float32(0.4) + np.float32(2.2 / (H * W)) * np.arange(H * W, dtype=np.float32))
    depth[:len(d_edges)] = g.permutation(d_edges)
    depth[len(d_edges):len(d_edges) + len(special_d)] = special_d
    normal = np.tile(np.array([0.0, 0.6, 0.8], np.float32), H * W)
    normal[:len(n_edges)] = g.permutation(n_edges)
    normal[len(n_edges):len(n_edges) + 2] = (-1.0, 1.0)
    assert normal.min() >= -1.0 and normal.max() <= 1.0
    depth, normal = depth.reshape(H, W), normal.reshape(H, W, 3)
    base = g.integers(0, 256, (4, H, W)).astype(np.uint8)
    base[:, 50:, 10:40] = 9                                   # a flat area: matches, and a compressible second block
    renders = [(np.roll(base, 7 * i, axis=2).astype(np.float32) / np.float32(255.0)) for i in range(N_FRAMES)]
    return renders, depth, normal


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    """The frames through GpuFrameWriter in both modes (three slots, five frames in flight), and what the host makes of them."""
    from autovfx_amd.frame_parallel import pack_rgba8
    renders, depth, normal = _built_frame()
    root = tmp_path_factory.mktemp("frames")
    for deflate in (True, False):
        with frame_io.GpuFrameWriter(str(root / ("deflate" if deflate else "stored")), workers=2, slots=3, deflate=deflate) as w:
            for i, r in enumerate(renders):
                w.submit(f"{i:05d}", {"render": torch.from_numpy(r).cuda(), "depth": torch.from_numpy(depth).cuda(),
                                      "normal": torch.from_numpy(normal).cuda()})
    host = {"images": [pack_rgba8(torch.from_numpy(r[:3]), torch.from_numpy(r[3:4])).permute(1, 2, 0).contiguous().numpy() for r in renders],
            "depth": np.ascontiguousarray(frame_io.depth2img(depth, 3.0)), "normal": _normal_byte(normal)}
    return root, host, depth, normal


def test_batch_path_writes_the_restatements_files(written):
    """gsr_frame_files_deflate: three images of two sizes per launch, frames in flight through fewer slots than frames.  Each PNG on disk
    is the restatement's file of the host-quantised array (pack_rgba8, depth2img, the truncated normal map); the .npy is np.save's."""
    root, host, depth, _ = written
    assert len(cases.encode(host["images"][0])[1]["blocks"]) == 2 and len(cases.encode(host["depth"])[1]["blocks"]) == 1
    want_depth, want_normal = cases.encode(host["depth"]), cases.encode(host["normal"])
    npy = io.BytesIO()
    np.save(npy, depth)
    for i in range(N_FRAMES):
        want_rgba = cases.encode(host["images"][i])
        assert all(b["type"] == "dynamic" for _, t in (want_rgba, want_depth, want_normal) for b in t["blocks"])
        for sub, (want, trace) in (("images", want_rgba), ("depth", want_depth), ("normal", want_normal)):
            _assert_same_file((root / "deflate" / sub / f"{i:05d}.png").read_bytes(), want, f"frame {i} {sub}", trace)
        assert (root / "deflate" / "depth" / f"{i:05d}.npy").read_bytes() == npy.getvalue()


def test_stored_mode_decodes_to_the_same_pixels(written):
    root, host, depth, _ = written
    npy = io.BytesIO()
    np.save(npy, depth)
    for i in range(N_FRAMES):
        for sub, want in (("images", host["images"][i]), ("depth", host["depth"]), ("normal", host["normal"])):
            for mode in ("stored", "deflate"):
                np.testing.assert_array_equal(frame_io.decode_png((root / mode / sub / f"{i:05d}.png").read_bytes()), want, err_msg=f"{mode} {sub} {i}")
        assert (root / "stored" / "depth" / f"{i:05d}.npy").read_bytes() == npy.getvalue()


def test_preview_kernel_at_every_truncation_edge(written):
    """frame_previews_kernel's contract is the same fp32 operations in the same order, truncation.  The frame holds, for every k, the
    fp32 values either side of the edge where the depth index and the normal byte step to k (two ulps each way), depth 0, negative,
    above 3 and infinite, normals of exactly -1 and +1: a division turned into a multiplication by a reciprocal, or a contracted
    multiply-add, moves some of these pixels.  Equality with numpy's fp32 evaluation."""
    root, _, depth, normal = written
    got_d = frame_io.decode_png((root / "deflate" / "depth" / "00000.png").read_bytes())
    got_n = frame_io.decode_png((root / "deflate" / "normal" / "00000.png").read_bytes())
    idx = _depth_index(depth)
    assert set(idx.reshape(-1).tolist()) == set(range(256)) and set(_normal_byte(normal).reshape(-1).tolist()) == set(range(256))
    # every colour of the table differs from its neighbours, so the pixel tells the index
    lut = frame_io.TURBO_LUT.astype(int)
    assert (np.abs(np.diff(lut, axis=0)).sum(axis=1) > 0).all()
    wrong = np.flatnonzero((got_d != frame_io.TURBO_LUT[idx]).any(axis=-1).reshape(-1))
    assert len(wrong) == 0, f"{len(wrong)} depth pixels, first: depth {depth.reshape(-1)[wrong[0]]!r} -> index {idx.reshape(-1)[wrong[0]]}"
    wrong = np.flatnonzero((got_n != _normal_byte(normal)).reshape(-1))
    assert len(wrong) == 0, f"{len(wrong)} normal bytes, first: {normal.reshape(-1)[wrong[0]]!r} -> {got_n.reshape(-1)[wrong[0]]}"


def test_preview_of_a_nan_depth_is_table_entry_0(tmp_path):
    """numpy leaves uint8(NaN) undefined; the kernel's fmaxf(NaN, 0) is 0: a NaN depth takes the colour of depth 0 (frame_io's docstring)."""
    g = np.random.default_rng(8)
    depth = g.random((8, 16), dtype=np.float32) * np.float32(3.0)
    nan_at = np.zeros((8, 16), bool)
    nan_at[2, 3] = nan_at[7, 15] = nan_at[0, 0] = True
    with_nan = np.where(nan_at, np.float32(np.nan), depth)
    frame = {"render": torch.rand(4, 8, 16).cuda(), "depth": torch.from_numpy(with_nan).cuda(),
             "normal": torch.nn.functional.normalize(torch.randn(8, 16, 3), dim=-1).cuda()}
    with frame_io.GpuFrameWriter(str(tmp_path), workers=1, slots=2, deflate=True) as w:
        w.submit("nan", frame)
    got = frame_io.decode_png((tmp_path / "depth" / "nan.png").read_bytes())
    np.testing.assert_array_equal(got, frame_io.depth2img(np.where(nan_at, np.float32(0.0), depth), 3.0))
    assert (got[nan_at] == frame_io.TURBO_LUT[0]).all()
    assert np.array_equal(np.load(tmp_path / "depth" / "nan.npy"), with_nan, equal_nan=True)
