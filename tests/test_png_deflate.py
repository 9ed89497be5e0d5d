"""The host restatement of the GPU PNG deflate encoder (png_deflate_cases.py), held on its own, and the coverage its cases claim.

Nothing here runs on the GPU.  The restatement's files must be files (zlib, Pillow and the chunk CRCs accept them and the inflated stream
is the Paeth stream), its code must be as good as Huffman's where nothing was clamped and complete where something was -- and every
case must reach, by the restatement's own trace, the path it was built for.  tests/test_png_deflate_gpu.py then asks the kernels for
the same bytes."""
import heapq

import numpy as np
import pytest

import png_deflate_cases as cases
from png_deflate_cases import BLOCK, EOB, PIECE, RUN_VALUE
from test_frame_io import _check_png_file


def _optimal_cost(counts):
    """Huffman's cost (sum of count x depth) from a heap, independent of how ties are broken."""
    heap = [int(c) for c in counts]
    if len(heap) == 1:
        return heap[0]
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        w = heapq.heappop(heap) + heapq.heappop(heap)
        cost += w
        heapq.heappush(heap, w)
    return cost


@pytest.mark.parametrize("case_id", cases.CASE_IDS)
def test_the_restatement_writes_a_valid_file_with_a_sound_code(case_id):
    img, data, tr = cases.case(case_id)
    _check_png_file(data, img, paeth=True)
    hist, lengths = tr["hist"], tr["lengths"]
    used = hist > 0
    assert (lengths[used] >= 1).all() and not lengths[~used].any() and lengths.max() <= 15
    kraft = int(sum(1 << (15 - int(d)) for d in lengths[used]))
    if max(tr["depths"]) <= 15:
        assert not tr["limit_picks"]
        assert int((hist * lengths).sum()) == _optimal_cost(hist[used]), "not an optimal code"
        assert kraft == 1 << 15
    else:
        assert tr["limit_picks"] and kraft == 1 << 15 and lengths.max() == 15, "a clamped code must be complete"
    # a rarer symbol never has the shorter code
    by_count = sorted((int(hist[s]), s) for s in np.flatnonzero(used))
    dealt = [int(lengths[s]) for _, s in by_count]
    assert dealt == sorted(dealt, reverse=True)
    # the blocks lie one behind the other from file offset 43 and the tokens tile the stream
    at = 43
    for b in tr["blocks"]:
        assert b["offset"] == at
        at += b["size"]
    assert at + 4 + 4 + 12 == len(data)
    assert tr["token_pos"][0] == 0 and np.array_equal(tr["token_pos"][1:], (tr["token_pos"] + tr["token_len"])[:-1])
    assert int((tr["token_pos"] + tr["token_len"])[-1]) == len(tr["stream"])
    assert int(hist[EOB]) == len(tr["blocks"])


def _matches(tr, dynamic_only=True):
    """(pos, len) of the match tokens (of dynamic blocks)."""
    m = tr["token_len"] > 1
    if dynamic_only:
        dyn = np.array([b["type"] == "dynamic" for b in tr["blocks"]])
        m &= dyn[tr["token_block"]]
    return tr["token_pos"][m], tr["token_len"][m]


def _token_at(tr, pos):
    i = int(np.searchsorted(tr["token_pos"], pos))
    assert tr["token_pos"][i] == pos, f"no token starts at {pos}"
    return int(tr["token_len"][i])


def test_run_sweep_reaches_every_length_every_offset_and_every_clipping():
    """Every start offset 0 .. 63 x every run 1 .. 66: all 62 match lengths come out of dynamic blocks, runs of 1 and 2 as literals, a
    piece that is one match of 64, runs clipped by the piece's end with 1 and with 2 literals left over, runs going on behind it."""
    seen_lengths, whole_piece, rest, continued, offsets = set(), 0, set(), 0, set()
    for chunk in range(cases.SWEEP_CHUNKS):
        _, _, tr = cases.case(f"sweep{chunk}")
        stream, slots = cases.sweep_layout(chunk)
        assert np.array_equal(stream, tr["stream"])
        assert all(b["type"] == "dynamic" for b in tr["blocks"]), "filler keeps the blocks dynamic"
        assert len(stream) <= 5 * BLOCK
        pos, lens = _matches(tr)
        seen_lengths |= set(int(v) for v in lens)
        whole_piece += int(((pos % PIECE == 0) & (lens == PIECE)).sum())
        for o, r, p in slots:
            offsets.add(p % PIECE)
            assert p % PIECE == o and (stream[p - 1:p + r] == RUN_VALUE).all() and stream[p - 2] != RUN_VALUE and stream[p + r] != RUN_VALUE
            # the run as the rule cuts it: piece by piece, a clipped part of 3 or more is a match, less is literals
            at, left, before = p, r, 0
            while left:
                part = min(left, PIECE - at % PIECE)
                if part >= 3:
                    assert _token_at(tr, at) == part, (o, r, at)
                    continued += at % PIECE == 0 and at > p      # a match at a piece's start that goes on where the piece before ended
                else:
                    assert all(_token_at(tr, at + k) == 1 for k in range(part)), (o, r, at)
                    if before >= 3:                               # literals left over behind a match that the piece's end clipped
                        rest.add(part)
                at, left, before = at + part, left - part, part
            assert _token_at(tr, p - 1) == 1, "the head of a run is a literal"
    assert offsets == set(range(PIECE))
    assert seen_lengths == set(range(3, PIECE + 1)), sorted(set(range(3, PIECE + 1)) - seen_lengths)
    assert whole_piece >= 1 and rest == {1, 2} and continued >= 1


def _block_types(case_id):
    return [b["type"] for b in cases.case(case_id)[2]["blocks"]]


def test_seam_cases_reach_their_seams():
    tr = cases.case("seam:match_behind_dynamic")[2]
    assert _block_types("seam:match_behind_dynamic") == ["dynamic", "dynamic"] and _token_at(tr, BLOCK) == 10
    tr = cases.case("seam:match_behind_stored")[2]
    assert _block_types("seam:match_behind_stored") == ["stored", "dynamic"] and _token_at(tr, BLOCK) == 10
    assert tr["stream"][BLOCK - 1] == tr["stream"][BLOCK] and (tr["token_len"][tr["token_block"] == 0] == 1).all()
    # stored behind dynamic and dynamic behind stored, each kind also as the file's last block
    assert _block_types("seam:dynamic_stored") == ["dynamic", "stored"]
    assert _block_types("seam:dynamic_stored_dynamic") == ["dynamic", "stored", "dynamic"]
    assert _block_types("seam:stored_stored_dynamic") == ["stored", "stored", "dynamic"]
    for name, run in (("seam:short_last_piece_in_a_run", 10), ("seam:short_last_piece_run_over_the_piece_seam", 5)):
        tr = cases.case(name)[2]
        n = len(tr["stream"])
        assert 0 < n % PIECE < PIECE and _block_types(name)[-1] == "dynamic"
        assert int(tr["token_len"][-1]) == run and int(tr["token_pos"][-1]) + run == n, "the last token is a match that ends with the stream"
    assert int(cases.case("seam:short_last_piece_run_over_the_piece_seam")[2]["token_pos"][-1]) % PIECE == 0
    img, _, tr = cases.case("seam:four_blocks_exactly")
    assert img.shape == (1, 21845, 3) and len(tr["stream"]) == 4 * BLOCK and _block_types("seam:four_blocks_exactly") == ["dynamic"] * 4
    for b in (1, 2, 3):
        assert _token_at(tr, b * BLOCK) == 3 * b
    assert int(tr["token_len"][-1]) == PIECE and [_token_at(tr, BLOCK + k) for k in (640, 641, 704, 768, 769)] == [1, 63, 64, 1, 1]


def test_alphabet_cases_have_the_alphabets_they_claim():
    img, _, tr = cases.case("alphabet:constant")
    assert img.shape == (1, 1365, 3) and sorted(np.flatnonzero(tr["hist"]).tolist()) == [0, 4, EOB, 276]
    symbols = list(range(257)) + cases.LENGTH_SYMBOLS
    _, _, tr = cases.case("alphabet:equal")
    assert sorted(np.flatnonzero(tr["hist"]).tolist()) == symbols and len(symbols) == 277
    assert set(tr["hist"][symbols].tolist()) == {1} and _block_types("alphabet:equal") == ["dynamic"]
    assert sorted(set(tr["lengths"][symbols].tolist())) == [8, 9]
    _, _, tr = cases.case("alphabet:distinct")
    assert sorted(np.flatnonzero(tr["hist"]).tolist()) == symbols
    assert len(set(tr["hist"][symbols].tolist())) == 277, "every count distinct"
    assert "dynamic" in _block_types("alphabet:distinct") and len(tr["stream"]) <= 4 * BLOCK
    _, _, tr = cases.case("alphabet:ties")
    assert sorted(tr["lengths"][tr["hist"] > 0].tolist()) == [1, 3, 3, 4, 4, 4, 5, 6, 7, 8, 9, 10, 11, 11] and _block_types("alphabet:ties") == ["dynamic"]


@pytest.mark.parametrize("case_id", ["limit:literals", "limit:matches"])
def test_length_limit_cases_clamp_and_pick_below_14(case_id):
    _, _, tr = cases.case(case_id)
    assert int((tr["hist"] > 0).sum()) >= 22
    assert max(tr["depths"]) >= 20 and len(tr["limit_picks"]) >= 4 and min(tr["limit_picks"]) < 14
    assert _block_types(case_id) == ["dynamic"] * 3
    assert int(tr["hist"].max()) < len(tr["stream"]) / 2
    in_chain = [s for s in cases.LENGTH_SYMBOLS if tr["hist"][s]]
    if case_id == "limit:matches":
        assert in_chain == [257, 265, 273] and [int(tr["hist"][s]) for s in in_chain] == [5, 13, 34]
        assert any(tr["lengths"][s] == 15 for s in in_chain), "a match symbol among the clamped ones"
    else:
        assert not in_chain and (tr["token_len"] == 1).all()


def test_phase_family_reaches_every_bit_and_byte_phase():
    """The end of block 0 in every bit phase (where the sync marker's padding starts), block 1's first and last byte in every phase of a
    32-bit word (how the block's image in LDS is shifted, and which of its edge bytes go out one by one)."""
    end_bits, starts, ends = set(), set(), set()
    for j in range(cases.PHASE_FAMILY):
        _, _, tr = cases.case(f"phase{j}")
        b0, b1 = tr["blocks"]
        assert b0["type"] == b1["type"] == "dynamic"
        end_bits.add(b0["end_bit"] % 8)
        starts.add(b1["offset"] % 4)
        ends.add((b1["offset"] + b1["size"]) % 4)
    assert end_bits == set(range(8)) and starts == set(range(4)) and ends == set(range(4))


def test_multi_row_cases_are_the_decode_tests_images():
    from test_frame_io import _test_images
    for shape in cases.MULTI_ROW_SHAPES:
        h, w, c = shape
        for kind, img in _test_images(shape, h * 131 + w + c).items():
            assert np.array_equal(cases.case_image(f"rows:{kind}:{h}x{w}x{c}"), img)
    assert "dynamic" in _block_types("rows:mixed:300x100x4") and set(_block_types("rows:noise:300x100x4")) == {"stored"}


def test_the_cases_tell_each_rule_from_its_neighbour():
    """A kernel that took 4 for the match threshold, the node on a tie, or the smallest populated length in the limiter would write a
    valid file too.  On these cases it would write ANOTHER file: the byte comparison sees it."""
    def differs(case_id, **rule):
        img, want, _ = cases.case(case_id)
        got, _ = cases.encode(img, **rule)
        _check_png_file(got, img, paeth=True)
        return got != want
    assert differs("sweep0", min_match=4)
    assert differs("alphabet:ties", tie_leaf=False) and differs("sweep0", tie_leaf=False)
    assert differs("limit:literals", limit_from_largest=False) and differs("limit:matches", limit_from_largest=False)


def test_length_symbols_against_the_rfc_table():
    """RFC 1951 3.2.5, typed in: (symbol, extra bits, lengths)."""
    rfc = [(257, 0, 3, 3), (264, 0, 10, 10), (265, 1, 11, 12), (268, 1, 17, 18), (269, 2, 19, 22), (272, 2, 31, 34), (273, 3, 35, 42),
           (276, 3, 59, 66)]
    for sym, eb, lo, hi in rfc:
        for n in range(lo, min(hi, 64) + 1):
            assert cases.length_code(n) == (sym, eb, n - lo)
    assert [cases.length_code(n)[0] for n in (10, 11, 18, 19, 34, 35, 58, 59, 64)] == [264, 265, 268, 269, 272, 273, 275, 276, 276]
