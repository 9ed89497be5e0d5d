"""gsr_resize_rgba8_bilinear / gsr_resize_f32_nearest on the GPU against their host restatements (resample_cases.py), bit for bit:
every size at which the kernels or their tables change path with every named input, cached and transposed tables, a sweep of axis pairs,
unwritten and overwritten memory, side streams, strided sources, two host threads, mixed layer sizes in composite_frame, refusals.

The restatements are held to Pillow on the CPU (test_resample.py); nothing here asks Pillow."""
from __future__ import annotations

import threading

import numpy as np
import pytest
import torch

import resample_cases as cases
from resample_cases import KINDS, SIZES, bits, case_seed, size_id

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZE_IDS = [size_id(*s) for s in SIZES]


def _wh(hw):
    return (hw[1], hw[0])


def _gpu_rgba8(img: np.ndarray, dst_hw) -> np.ndarray:
    from autovfx_amd import compositor
    got = compositor.resize_rgba8(torch.from_numpy(img).to(DEV), _wh(dst_hw))
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(dst_hw) + (4,) and got.is_contiguous()
    return got.cpu().numpy()


def _gpu_depth(d: np.ndarray, dst_hw) -> np.ndarray:
    from autovfx_amd import compositor
    got = compositor.resize_depth(torch.from_numpy(d).to(DEV), _wh(dst_hw))
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(dst_hw) and got.is_contiguous()
    return got.cpu().numpy()


def _first_difference(got: np.ndarray, want: np.ndarray):
    at = np.argwhere(got != want)
    return None if len(at) == 0 else (tuple(at[0]), got[tuple(at[0])], want[tuple(at[0])], len(at))


# ---- every size with every input, first use of a table and cached use --------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("src_hw,dst_hw", SIZES, ids=SIZE_IDS)
def test_rgba8_equals_the_restatement_on_every_size_and_kind(src_hw, dst_hw, kind):
    img = cases.image(kind, *src_hw, case_seed(src_hw, dst_hw, kind))
    want = cases.resize_rgba8_host(img, _wh(dst_hw))
    first, cached = _gpu_rgba8(img, dst_hw), _gpu_rgba8(img, dst_hw)
    assert _first_difference(first, want) is None, _first_difference(first, want)
    assert np.array_equal(first, cached)


@pytest.mark.parametrize("src_hw,dst_hw", SIZES, ids=SIZE_IDS)
def test_depth_equals_the_restatement_on_every_size(src_hw, dst_hw):
    d = cases.depth(*src_hw, case_seed(src_hw, dst_hw))
    want = bits(cases.resize_depth_host(d, _wh(dst_hw)))
    first, cached = bits(_gpu_depth(d, dst_hw)), bits(_gpu_depth(d, dst_hw))
    assert _first_difference(first, want) is None, _first_difference(first, want)
    assert np.array_equal(first, cached)


def test_a_cached_table_serves_the_other_axis_of_the_transposed_sizes():
    """(8, 12) -> (6, 18) builds the tables 12 -> 18 for its rows and 8 -> 6 for its columns; (12, 8) -> (18, 6) then finds both in the
    cache and uses each on the other axis."""
    src_hw, dst_hw = (8, 12), (6, 18)
    img, d = cases.image("noise", *src_hw, 77), cases.depth(*src_hw, 77)
    assert np.array_equal(_gpu_rgba8(img, dst_hw), cases.resize_rgba8_host(img, _wh(dst_hw)))
    assert np.array_equal(bits(_gpu_depth(d, dst_hw)), bits(cases.resize_depth_host(d, _wh(dst_hw))))
    img_t, d_t = np.ascontiguousarray(img.transpose(1, 0, 2)), np.ascontiguousarray(d.T)
    got = _gpu_rgba8(img_t, dst_hw[::-1])
    want = cases.resize_rgba8_host(img_t, dst_hw)          # (size_wh of the transposed target (18, 6) is (6, 18))
    assert want.shape == (18, 6, 4)
    assert _first_difference(got, want) is None, _first_difference(got, want)
    assert np.array_equal(bits(_gpu_depth(d_t, dst_hw[::-1])), bits(cases.resize_depth_host(d_t, dst_hw)))


def test_a_sweep_of_axis_pairs():
    """At most 150 axis pairs (each leaves two small tables on the device for the life of the process), 255 / 256 / 257 among the
    output widths; the input kinds in turn."""
    sweep = cases.gpu_sweep()
    assert len(sweep) <= cases.SWEEP_MAX_PAIRS and {255, 256, 257} <= {d[1] for _, d in sweep}
    for n, (src_hw, dst_hw) in enumerate(sweep):
        kind = KINDS[n % len(KINDS)]
        img, d = cases.image(kind, *src_hw, 1000 + n), cases.depth(*src_hw, 1000 + n)
        got, want = _gpu_rgba8(img, dst_hw), cases.resize_rgba8_host(img, _wh(dst_hw))
        assert _first_difference(got, want) is None, (src_hw, dst_hw, kind, _first_difference(got, want))
        got, want = bits(_gpu_depth(d, dst_hw)), bits(cases.resize_depth_host(d, _wh(dst_hw)))
        assert _first_difference(got, want) is None, (src_hw, dst_hw, _first_difference(got, want))


# ---- every output byte written and nothing beyond ----------------------------------------------------------------------------------

GUARD = 64        # bytes on either side of a carved-out plane


def _carved(nbytes: int, fill: int):
    """``nbytes`` between two guards, every byte ``fill``; returns ``(whole, inner)`` as uint8."""
    whole = torch.full((GUARD + nbytes + GUARD,), fill, dtype=torch.uint8, device=DEV)
    return whole, whole[GUARD:GUARD + nbytes]


def _guards_hold(whole: torch.Tensor, nbytes: int, fill: int) -> bool:
    return bool((whole[:GUARD] == fill).all()) and bool((whole[GUARD + nbytes:] == fill).all())


@pytest.mark.parametrize("src_hw,dst_hw", [((12, 9), (18, 11)), ((2, 513), (2, 257))], ids=["two-passes", "one-pass-257-wide"])
def test_rgba8_writes_every_byte_of_dst_and_nothing_outside_dst_and_tmp(src_hw, dst_hw):
    from autovfx_amd import _lib
    img = cases.image("alpha_steps", *src_hw, 5)
    want = cases.resize_rgba8_host(img, _wh(dst_hw))
    src = torch.from_numpy(img).to(DEV)
    two_passes = src_hw[0] != dst_hw[0] and src_hw[1] != dst_hw[1]
    n_dst, n_tmp = dst_hw[0] * dst_hw[1] * 4, src_hw[0] * dst_hw[1] * 4
    runs = []
    for fill in (0x55, 0xAA):
        (dst_w, dst), (tmp_w, tmp) = _carved(n_dst, fill), _carved(n_tmp, fill)
        assert dst.data_ptr() % 4 == 0 and tmp.data_ptr() % 4 == 0
        _lib.call("gsr_resize_rgba8_bilinear", src.data_ptr(), src_hw[1], src_hw[0], dst.data_ptr(), dst_hw[1], dst_hw[0], tmp.data_ptr(),
                  device=src.device)
        torch.cuda.synchronize()
        assert _guards_hold(dst_w, n_dst, fill), "written outside dst"
        assert _guards_hold(tmp_w, n_tmp, fill), "written outside tmp"
        if not two_passes:
            assert bool((tmp == fill).all()), "a single pass has no use for tmp"
        runs.append(dst.cpu().numpy().reshape(want.shape))
    assert np.array_equal(runs[0], runs[1]), "a byte of dst keeps what was there before the call"
    assert _first_difference(runs[0], want) is None, _first_difference(runs[0], want)


@pytest.mark.parametrize("src_hw,dst_hw", [((12, 9), (18, 11)), ((2, 513), (2, 257))], ids=["both-axes", "257-wide"])
def test_nearest_writes_every_element_of_dst_and_nothing_outside(src_hw, dst_hw):
    from autovfx_amd import _lib
    d = cases.depth(*src_hw, 6)
    want = bits(cases.resize_depth_host(d, _wh(dst_hw)))
    src = torch.from_numpy(d).to(DEV)
    n = dst_hw[0] * dst_hw[1]
    runs = []
    for fill in (0x55555555, 0xAAAAAAAA - (1 << 32)):           # 4-byte fills (the second as the int32 it is)
        whole = torch.full((GUARD // 4 + n + GUARD // 4,), fill, dtype=torch.int32, device=DEV)
        dst = whole[GUARD // 4:GUARD // 4 + n]
        _lib.call("gsr_resize_f32_nearest", src.data_ptr(), src_hw[1], src_hw[0], dst.data_ptr(), dst_hw[1], dst_hw[0], device=src.device)
        torch.cuda.synchronize()
        assert bool((whole[:GUARD // 4] == fill).all()) and bool((whole[GUARD // 4 + n:] == fill).all()), "written outside dst"
        runs.append(dst.cpu().numpy().view(np.uint32).reshape(want.shape))
    assert np.array_equal(runs[0], runs[1]), "an element of dst keeps what was there before the call"
    assert _first_difference(runs[0], want) is None, _first_difference(runs[0], want)


# ---- streams, strides, threads -----------------------------------------------------------------------------------------------------

MASK8, MASK32 = 0x5A, 0x5A5A5A5A
SIDE_STREAM_SIZE = ((10, 77), (7, 45))                        # used nowhere else: its tables are built while the side stream runs
THREAD_SIZES = [((7, 211), (5, 97)), ((11, 193), (13, 89))]   # used nowhere else: each thread's first call builds its tables


def _elsewhere():
    """Every ``(in, out)`` axis pair the other tests of this file (and the sizes of test_compositor.py's resize tests) touch."""
    used = set()
    for s, d in SIZES + cases.gpu_sweep() + [((8, 12), (6, 18)), ((72, 104), (36, 52)), ((54, 65), (36, 52))]:
        used |= {(s[0], d[0]), (s[1], d[1]), (s[1], d[0]), (s[0], d[1])}
    return used


def test_side_stream_fed_by_a_kernel_without_a_synchronisation():
    """The source is produced by a kernel on a side stream and resized on that stream at once; the tables of this size are built (and
    uploaded) during that call."""
    from autovfx_amd import compositor
    src_hw, dst_hw = SIDE_STREAM_SIZE
    assert not ({(src_hw[0], dst_hw[0]), (src_hw[1], dst_hw[1])} & _elsewhere())
    img, d = cases.image("noise", *src_hw, 31), cases.depth(*src_hw, 31)
    masked_c = torch.from_numpy(img ^ np.uint8(MASK8)).to(DEV)
    masked_d = torch.from_numpy((bits(d) ^ np.uint32(MASK32)).view(np.int32)).to(DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got_c = compositor.resize_rgba8(masked_c ^ MASK8, _wh(dst_hw))
        got_d = compositor.resize_depth((masked_d ^ MASK32).view(torch.float32), _wh(dst_hw))
    side.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(got_c.cpu().numpy(), cases.resize_rgba8_host(img, _wh(dst_hw)))
    assert np.array_equal(bits(got_d.cpu().numpy()), bits(cases.resize_depth_host(d, _wh(dst_hw))))


def test_non_contiguous_sources():
    from autovfx_amd import compositor
    src_hw, dst_hw = (12, 9), (18, 11)
    wide = cases.image("noise", src_hw[0], src_hw[1] * 2, 41)                   # every second column
    wide6 = np.random.default_rng(42).integers(0, 256, src_hw + (6,), dtype=np.uint8)   # a channel slice of a wider tensor
    wide_d = cases.depth(src_hw[0], src_hw[1] * 2, 43)
    for host, view in ((wide, lambda t: t[:, ::2]), (wide6, lambda t: t[..., 1:5]), (wide, lambda t: t[:, 1::2])):
        t = view(torch.from_numpy(host).to(DEV))
        assert not t.is_contiguous() and tuple(t.shape) == src_hw + (4,)
        got = compositor.resize_rgba8(t, _wh(dst_hw))
        torch.cuda.synchronize()
        want = cases.resize_rgba8_host(np.ascontiguousarray(view(torch.from_numpy(host)).numpy()), _wh(dst_hw))
        assert np.array_equal(got.cpu().numpy(), want)
    for view in (lambda t: t[:, ::2], lambda t: t[:, :src_hw[0]].T[:, :src_hw[1]]):
        t = view(torch.from_numpy(wide_d).to(DEV))
        assert not t.is_contiguous() and tuple(t.shape) == src_hw
        got = compositor.resize_depth(t, _wh(dst_hw))
        torch.cuda.synchronize()
        want = cases.resize_depth_host(np.ascontiguousarray(view(torch.from_numpy(wide_d)).numpy()), _wh(dst_hw))
        assert np.array_equal(bits(got.cpu().numpy()), bits(want))


def test_two_host_threads_on_two_streams_build_their_tables_at_once():
    """Two host threads on two HIP streams, each resizing a size pair nobody has used yet, so both go through the table cache's first
    use together; the results are the serial ones (and the restatement's)."""
    from autovfx_amd import compositor
    used = _elsewhere() | {(SIDE_STREAM_SIZE[0][i], SIDE_STREAM_SIZE[1][i]) for i in (0, 1)}
    mine = [{(s[0], d[0]), (s[1], d[1])} for s, d in THREAD_SIZES]
    assert not (mine[0] & used) and not (mine[1] & used) and not (mine[0] & mine[1])
    dev = torch.device("cuda", 0)
    inputs = [(cases.image("noise", *s, 50 + t), cases.depth(*s, 50 + t)) for t, (s, _) in enumerate(THREAD_SIZES)]
    on_gpu = [(torch.from_numpy(c).to(dev), torch.from_numpy(d).to(dev)) for c, d in inputs]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    got, errors, gate = [None, None], [], threading.Barrier(2)

    def worker(t):
        try:
            torch.cuda.set_device(dev)
            wh = _wh(THREAD_SIZES[t][1])
            gate.wait(timeout=30)
            with torch.cuda.stream(streams[t]):
                got[t] = (compositor.resize_rgba8(on_gpu[t][0], wh), compositor.resize_depth(on_gpu[t][1], wh))
            streams[t].synchronize()
        except BaseException as e:      # noqa: BLE001 -- handed to the main thread
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    [th.start() for th in threads]
    [th.join() for th in threads]
    assert not errors, errors
    torch.cuda.synchronize()
    for t, (_, dst_hw) in enumerate(THREAD_SIZES):
        serial_c, serial_d = _gpu_rgba8(inputs[t][0], dst_hw), _gpu_depth(inputs[t][1], dst_hw)
        assert np.array_equal(got[t][0].cpu().numpy(), serial_c) and np.array_equal(bits(got[t][1].cpu().numpy()), bits(serial_d))
        assert np.array_equal(serial_c, cases.resize_rgba8_host(inputs[t][0], _wh(dst_hw)))
        assert np.array_equal(bits(serial_d), bits(cases.resize_depth_host(inputs[t][1], _wh(dst_hw))))


# ---- composite_frame with layers at mixed sizes ------------------------------------------------------------------------------------

def oracle_from_mixed_layers(L, hw):
    """``oracle_from_blender_layers`` of test_compositor.py with every layer at a size of its own and the restatements in Pillow's
    place: the smoke depth fill on the layers as they arrive, every layer but the background brought to the frame's size (one that
    is there already comes back as a copy), the per-pixel composite."""
    from oracle import compositor_oracle as co
    args = dict(L)
    if "s_f_c" in args:
        args["s_f_d"], _ = co.smoke_depth_fill(args["s_f_c"], args["s_f_d"], None)
    for k in args:
        if k != "bg_c":
            args[k] = (cases.resize_rgba8_host if args[k].ndim == 3 else cases.resize_depth_host)(args[k], _wh(hw))
    return co.composite_frame(**args)


def test_composite_frame_takes_layers_at_mixed_sizes():
    from autovfx_amd import compositor
    from test_compositor import synthetic_layers
    hw = (36, 52)
    L = synthetic_layers(*hw, seed=61, with_3dgs=True, with_smoke=True, with_fire=True)
    L["o_c"] = synthetic_layers(hw[0] * 2, hw[1] * 2, seed=62)["o_c"]                           # 2 x
    L["s_d"] = synthetic_layers(int(hw[0] * 1.5), int(hw[1] * 1.25), seed=63)["s_d"]            # 1.5 x 1.25
    assert L["o_c"].shape == (72, 104, 4) and L["s_d"].shape == (54, 65)
    assert all(v.shape[:2] == hw for k, v in L.items() if k not in ("o_c", "s_d"))
    want = oracle_from_mixed_layers(L, hw)
    t = {k: torch.from_numpy(v).to(DEV) for k, v in L.items()}
    t["s_f_d"] = compositor.smoke_depth_fill(t["s_f_c"], t["s_f_d"])
    got = compositor.composite_frame(**t)
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and tuple(got.shape) == hw + (4,)
    assert _first_difference(got.cpu().numpy(), want) is None, _first_difference(got.cpu().numpy(), want)


# ---- refusals, before anything is launched -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size_wh", [(0, 5), (5, 0), (-1, 5), (4, -3), (0, 0)])
def test_a_target_size_that_is_not_positive_is_refused(size_wh):
    from autovfx_amd import compositor
    img, d = torch.from_numpy(cases.image("noise", 6, 7, 1)).to(DEV), torch.from_numpy(cases.depth(6, 7, 1)).to(DEV)
    with pytest.raises(RuntimeError):
        compositor.resize_rgba8(img, size_wh)
    with pytest.raises(RuntimeError):
        compositor.resize_depth(d, size_wh)
    out_c, out_d = torch.full((5, 5, 4), 7, dtype=torch.uint8, device=DEV), torch.full((5, 5), 7.0, device=DEV)
    with pytest.raises(RuntimeError):
        compositor.resize_rgba8(img, size_wh, out=out_c)
    with pytest.raises(RuntimeError):
        compositor.resize_depth(d, size_wh, out=out_d)
    torch.cuda.synchronize()
    assert bool((out_c == 7).all()) and bool((out_d == 7.0).all())


H_OUT, W_OUT = 4, 5
BAD_OUT_RGBA8 = {
    "shape-wider": lambda: torch.full((H_OUT, W_OUT + 1, 4), 7, dtype=torch.uint8, device=DEV),
    "shape-transposed": lambda: torch.full((W_OUT, H_OUT, 4), 7, dtype=torch.uint8, device=DEV),
    "shape-smaller": lambda: torch.full((H_OUT - 1, W_OUT, 4), 7, dtype=torch.uint8, device=DEV),
    "shape-three-channels": lambda: torch.full((H_OUT, W_OUT, 3), 7, dtype=torch.uint8, device=DEV),
    "shape-flat": lambda: torch.full((H_OUT * W_OUT * 4,), 7, dtype=torch.uint8, device=DEV),
    "dtype-int8": lambda: torch.full((H_OUT, W_OUT, 4), 7, dtype=torch.int8, device=DEV),
    "dtype-float32": lambda: torch.full((H_OUT, W_OUT, 4), 7, dtype=torch.float32, device=DEV),
    "device-cpu": lambda: torch.full((H_OUT, W_OUT, 4), 7, dtype=torch.uint8),
    "strided-columns": lambda: torch.full((H_OUT, W_OUT * 2, 4), 7, dtype=torch.uint8, device=DEV)[:, ::2],
    "strided-channels": lambda: torch.full((H_OUT, W_OUT, 6), 7, dtype=torch.uint8, device=DEV)[..., 1:5],
    "strided-transposed": lambda: torch.full((W_OUT, H_OUT, 4), 7, dtype=torch.uint8, device=DEV).transpose(0, 1),
}
BAD_OUT_DEPTH = {
    "shape-wider": lambda: torch.full((H_OUT, W_OUT + 1), 7.0, device=DEV),
    "shape-transposed": lambda: torch.full((W_OUT, H_OUT), 7.0, device=DEV),
    "shape-smaller": lambda: torch.full((H_OUT - 1, W_OUT), 7.0, device=DEV),
    "shape-extra-axis": lambda: torch.full((H_OUT, W_OUT, 1), 7.0, device=DEV),
    "dtype-int32": lambda: torch.full((H_OUT, W_OUT), 7, dtype=torch.int32, device=DEV),
    "dtype-float64": lambda: torch.full((H_OUT, W_OUT), 7.0, dtype=torch.float64, device=DEV),
    "dtype-float16": lambda: torch.full((H_OUT, W_OUT), 7.0, dtype=torch.float16, device=DEV),
    "device-cpu": lambda: torch.full((H_OUT, W_OUT), 7.0),
    "strided-columns": lambda: torch.full((H_OUT, W_OUT * 2), 7.0, device=DEV)[:, ::2],
    "strided-transposed": lambda: torch.full((W_OUT, H_OUT), 7.0, device=DEV).T,
}


def _unchanged(out: torch.Tensor) -> bool:
    base = out._base if out._base is not None else out            # the whole allocation a view was cut from
    return bool((base == 7).all())


@pytest.mark.parametrize("bad", list(BAD_OUT_RGBA8))
def test_resize_rgba8_refuses_an_out_it_cannot_write_through(bad):
    from autovfx_amd import compositor
    img = torch.from_numpy(cases.image("noise", 8, 10, 2)).to(DEV)
    out = BAD_OUT_RGBA8[bad]()
    with pytest.raises(RuntimeError, match=r"resize_rgba8: out must be a contiguous torch\.uint8 tensor \(4, 5, 4\) on cuda:0"):
        compositor.resize_rgba8(img, (W_OUT, H_OUT), out=out)
    torch.cuda.synchronize()
    assert _unchanged(out)


@pytest.mark.parametrize("bad", list(BAD_OUT_DEPTH))
def test_resize_depth_refuses_an_out_it_cannot_write_through(bad):
    from autovfx_amd import compositor
    d = torch.from_numpy(cases.depth(8, 10, 2)).to(DEV)
    out = BAD_OUT_DEPTH[bad]()
    with pytest.raises(RuntimeError, match=r"resize_depth: out must be a contiguous torch\.float32 tensor \(4, 5\) on cuda:0"):
        compositor.resize_depth(d, (W_OUT, H_OUT), out=out)
    torch.cuda.synchronize()
    assert _unchanged(out)


def test_a_valid_out_is_written_and_returned():
    from autovfx_amd import compositor
    src_hw, dst_hw = (12, 9), (18, 11)
    img, d = cases.image("noise", *src_hw, 3), cases.depth(*src_hw, 3)
    out_c = torch.full(dst_hw + (4,), 7, dtype=torch.uint8, device=DEV)
    out_d = torch.full(dst_hw, 7.0, device=DEV)
    assert compositor.resize_rgba8(torch.from_numpy(img).to(DEV), _wh(dst_hw), out=out_c) is out_c
    assert compositor.resize_depth(torch.from_numpy(d).to(DEV), _wh(dst_hw), out=out_d) is out_d
    torch.cuda.synchronize()
    assert np.array_equal(out_c.cpu().numpy(), cases.resize_rgba8_host(img, _wh(dst_hw)))
    assert np.array_equal(bits(out_d.cpu().numpy()), bits(cases.resize_depth_host(d, _wh(dst_hw))))
