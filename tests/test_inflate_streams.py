"""The wave's inflate (csrc/gsr_inflate_core.h) on one host lane, on streams zlib's encoder never writes: ``deflate_streams`` builds
them bit by bit, zlib's DEcoder vouches for each where it is built, and the host lane must give zlib's bytes -- or, for the streams
with a defect, the status named beside them.  Bytes are compared for equality; nothing here has a tolerance."""
import pytest

import deflate_streams as ds
from test_layer_io import _host_lane_inflate


def _held_to_the_replay(corpus):
    bad = []
    for name, stream, data in corpus:
        got = _host_lane_inflate(stream, len(data))
        if got != (0, data):
            bad.append((name, got[0]))
            continue
        over = _host_lane_inflate(stream, len(data) - 1)[0] if data else ds.OUTPUT_OVERFLOW
        short = _host_lane_inflate(stream, len(data) + 1)[0]
        if (over, short) != (ds.OUTPUT_OVERFLOW, ds.SHORT_OUTPUT):
            bad.append((name, "sizes -1 / +1", over, short))
    assert not bad, f"{len(bad)} of {len(corpus)} streams (name, status): {bad[:10]}"


def test_corpora_are_what_the_issue_lists():
    """The corpora reach what they were built for -- said from the builder's own records, not from the code under test."""
    a, b, c, d = ds.corpus_a(), ds.corpus_b(), ds.corpus_c(), ds.corpus_d()
    assert len(a) == 148 and all(len(data) > 32768 + 258 for _n, _s, data in a)       # the ring wraps, in the ninth segment
    assert {len(data) % 4096 for _n, _s, data in b} >= set(range(1, 18))                    # every size of the last, partial flush
    assert len({name for name, *_ in a + b + c}) == len(a + b + c)
    assert {status for *_x, status in d} == {ds.BAD_BLOCK_TYPE, ds.BAD_STORED, ds.BAD_LENGTHS, ds.BAD_CODE, ds.BAD_DISTANCE,
                                            ds.OUTPUT_OVERFLOW, ds.INPUT_OVERRUN, ds.BAD_CHECKSUM, ds.SHORT_OUTPUT}


def test_every_match_shape_on_the_host_lane():
    """A: every length 3 ... 258 at every distance of the grid, 32768 = the ring's size among them."""
    _held_to_the_replay(ds.corpus_a())


def test_matches_at_segment_and_ring_boundaries_on_the_host_lane():
    """B: a match that starts 0 ... 259 bytes in front of a 4 KB segment's end, the ring's wrap and its second wrap."""
    _held_to_the_replay(ds.corpus_b())


def test_dynamic_headers_on_the_host_lane():
    """C: code words of every length 1 ... 15, HLIT / HDIST / HCLEN at their ends, repeats that run from the literal lengths into the
    distance lengths or end at the last length, one-word and empty codes, tables rebuilt between blocks."""
    _held_to_the_replay(ds.corpus_c())


@pytest.mark.parametrize("k", range(len(ds.corpus_d())), ids=[name for name, *_ in ds.corpus_d()])
def test_defect_is_refused_with_its_status(k):
    """D: the status reasoned out for each defect (``deflate_streams.corpus_d``) is the one the host lane gives."""
    name, stream, n, status = ds.corpus_d()[k]
    assert _host_lane_inflate(stream, n)[0] == status, name
