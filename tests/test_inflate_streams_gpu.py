"""The wave's inflate ON the device (``gsr_inflate_zlib_blocks``: ``inflate_zlib<64>``, one wave per stream) on the hand-made streams of
``deflate_streams``: the 64-lane ``copy_match`` -- lane mod distance from a float reciprocal, five pieces, the ring's wrap -- runs
only there, and zlib's own encoder gives it few of its shapes (no distance above 32506, overlapping long matches at the distances the
data happen to have).  Every output byte is compared with the replay zlib vouched for; every byte AROUND an output -- ``out`` is filled
with 0xA5, the jobs lie at all 16 alignments with 64 bytes between them -- must still be 0xA5: that holds the 16-byte flush path and
the last, partial flush to their regions."""
import struct
import zlib

import numpy as np
import pytest
import torch

import deflate_streams as ds
from autovfx_amd import exr, layer_io
from test_inflate_sanitized import sanitized_corpus
from test_layer_io import _host_lane_inflate

pytestmark = pytest.mark.gpu

FILL, GAP = 0xA5, 64


def _launch(jobs, dev):
    """``jobs``: [(stream, dst_bytes)], one launch.  ``(out, status, regions)``: the whole output buffer (0xA5 before the launch), the
    statuses, and per job where its output lies -- job k at an offset that is k mod 16 behind a multiple of 16, 64 bytes or more
    between two jobs and at both ends."""
    table = np.zeros((len(jobs), 4), np.uint32)
    src_at, cursor, regions = 0, GAP, []
    for k, (stream, n) in enumerate(jobs):
        dst_at = cursor + (k - cursor) % 16
        table[k] = (src_at, len(stream), dst_at, n)
        regions.append((dst_at, n))
        src_at += (len(stream) + 3) & ~3
        cursor = dst_at + n + GAP
    packed = np.zeros(src_at + 4, np.uint8)
    for k, (stream, _n) in enumerate(jobs):
        packed[table[k, 0]:table[k, 0] + len(stream)] = np.frombuffer(stream, np.uint8)
    d_packed, d_table = torch.from_numpy(packed).to(dev), torch.from_numpy(table.view(np.int32)).to(dev)
    out = torch.full((cursor,), FILL, dtype=torch.uint8, device=dev)
    status = torch.full((len(jobs),), -1, dtype=torch.int32, device=dev)
    assert out.data_ptr() % 16 == 0 and d_packed.data_ptr() % 4 == 0
    with torch.cuda.device(dev):
        layer_io._lib.call("gsr_inflate_zlib_blocks", d_packed.data_ptr(), out.data_ptr(), d_table.data_ptr(), len(jobs), status.data_ptr(), None,
                           device=dev)
    torch.cuda.current_stream(dev).synchronize()
    return out.cpu().numpy(), status.cpu().numpy(), regions


def _gaps_untouched(out, regions):
    """Every byte outside the jobs' regions is still 0xA5; how many there are."""
    outside = np.ones(len(out), bool)
    for at, n in regions:
        outside[at:at + n] = False
    touched = np.flatnonzero(outside & (out != FILL))
    assert touched.size == 0, f"{touched.size} bytes written outside every job's output, the first at {int(touched[0])}"
    assert {at % 16 for at, _n in regions} == set(range(min(16, len(regions))))
    return int(outside.sum())


def _good_in_one_launch(corpus, dev):
    out, status, regions = _launch([(stream, len(data)) for _name, stream, data in corpus], dev)
    bad = []
    for k, (name, _stream, data) in enumerate(corpus):
        at, n = regions[k]
        if status[k] != 0 or out[at:at + n].tobytes() != data:
            bad.append((name, int(status[k])))
    assert not bad, f"{len(bad)} of {len(corpus)} streams refused or misread on the device (name, status): {bad[:10]}"
    checked = _gaps_untouched(out, regions)
    print(f"{len(corpus)} streams, {sum(n for _at, n in regions)} output bytes equal to the replay, {checked} gap bytes still 0x{FILL:02X}")


def test_every_match_shape_on_the_device():
    """A: every length 3 ... 258 at distances 1 ... 130, around 192, 256, 4096, zlib's limit 32506 and the ring's size 32768."""
    _good_in_one_launch(ds.corpus_a(), torch.device("cuda", 0))


def test_matches_at_segment_and_ring_boundaries_on_the_device():
    """B: matches across the ends of a 4 KB segment and of the ring, behind stored blocks, with a last flush of 1 ... 17 bytes."""
    _good_in_one_launch(ds.corpus_b(), torch.device("cuda", 0))


def test_dynamic_headers_on_the_device():
    """C: the slow path of ``decode_symbol`` (words of 11 ... 15 and 9 ... 15 bits), repeats across the two codes, one-word codes."""
    _good_in_one_launch(ds.corpus_c(), torch.device("cuda", 0))


def test_refused_streams_on_the_device_leave_their_neighbours_alone():
    """D between good streams of C, in one launch: each refused stream has the host lane's status -- the one named in the corpus --,
    each good neighbour its bytes, and nothing is written outside a job's own region.  The list is the sanitized program's
    (``sanitized_corpus``): only streams that ran clean under the sanitizers on the host reach the device here."""
    dev = torch.device("cuda", 0)
    clean = sanitized_corpus()
    refused = [(name, stream, n) for name, stream, n in clean if name.startswith("D ")]
    neighbours = [(name, stream, n) for name, stream, n in clean if name.startswith("C ")]
    named = {name: status for name, _s, _n, status in ds.corpus_d()}
    replays = {name: data for name, _s, data in ds.corpus_c()}
    assert len(refused) == len(named) and len(neighbours) == len(replays)
    jobs = []
    for k, bad in enumerate(refused):
        jobs += [bad, neighbours[k % len(neighbours)]]
    out, status, regions = _launch([(stream, n) for _name, stream, n in jobs], dev)
    wrong = []
    for k, (name, stream, n) in enumerate(jobs):
        at, _ = regions[k]
        if name in named:
            if not (status[k] == named[name] == _host_lane_inflate(stream, n)[0]):
                wrong.append((name, int(status[k]), named[name]))
        elif status[k] != 0 or out[at:at + n].tobytes() != replays[name]:
            wrong.append((name, int(status[k]), 0))
    assert not wrong, f"(name, the device's status, the host lane's): {wrong}"
    checked = _gaps_untouched(out, regions)
    print(f"{len(refused)} refused streams between {len(refused)} good ones, {checked} gap bytes still 0x{FILL:02X}")


def _depth_file_with_matches_at_the_ring_size(tmp_path):
    """The path of the rewritten file, and the depth first written to it."""
    g = np.random.default_rng(5)
    H, W = 64, 520
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    depth = (3.0 + np.sin(xx * 0.01) + np.cos(yy * 0.05) + 0.001 * g.random((H, W))).astype(np.float32)
    p = str(tmp_path / "Image0001.exr")
    exr.write_exr(p, {"Z": depth}, compression="ZIP")
    buf = open(p, "rb").read()
    table_at = exr.read_header(buf)["offsets_at"]
    n_blocks = (H + 15) // 16
    blocks, n_matches = [], 0
    for off in struct.unpack_from(f"<{n_blocks}Q", buf, table_at):
        y, size = struct.unpack_from("<ii", buf, off)
        raw = bytearray(zlib.decompress(buf[off + 8:off + 8 + size]))
        assert len(raw) == 16 * 4 * W == 33280
        raw[ds.WINDOW:] = raw[:len(raw) - ds.WINDOW]
        for at in g.integers(ds.WINDOW, len(raw), 5):                  # a few bytes off the period: literals between the matches
            raw[at] ^= 0x5A
        tokens, at = [], ds.WINDOW
        while at < len(raw):
            run = 0
            while run < 258 and at + run < len(raw) and raw[at + run] == raw[at + run - ds.WINDOW]:
                run += 1
            tokens.append((run, ds.WINDOW) if run >= 3 else raw[at])
            at += run if run >= 3 else 1
        n_matches += sum(isinstance(t, tuple) for t in tokens)
        z = ds.zlib_stream(ds.stored_blocks(bytes(raw[:ds.WINDOW])) + [ds.fixed_block(tokens)], bytes(raw))
        assert len(z) < len(raw) and zlib.decompress(z) == bytes(raw)           # (a block that did not shrink would be read as stored)
        blocks.append(struct.pack("<ii", y, len(z)) + z)
    assert n_matches >= 2 * n_blocks
    at, table = table_at + 8 * n_blocks, b""
    for b in blocks:
        table += struct.pack("<Q", at)
        at += len(b)
    open(p, "wb").write(buf[:table_at] + table + b"".join(blocks))
    return p, depth


def test_load_depth_with_matches_at_the_ring_size(tmp_path):
    """Through the caller: a 64 x 520 float ZIP depth pass -- a block is 16 lines of 2080 bytes = 33 280 bytes, more than the ring --
    whose blocks are rewritten as 32 768 stored bytes and then the rest as matches of distance 32768 (the payload repeats with that
    period but for a few bytes, which are literals).  The GPU inflates them without setting the error flag, and the plane is the
    host reader's of the same file."""
    p, depth = _depth_file_with_matches_at_the_ring_size(tmp_path)
    want = exr.load_depth_exr(p)
    assert not np.array_equal(want.view(np.uint32), depth.view(np.uint32))     # (the rewritten payload, not the one first written)
    dev = torch.device("cuda", 0)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    got = layer_io.load_depth(p, dev, None, flag)
    assert int(flag.cpu()) == 0
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
