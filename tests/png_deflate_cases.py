"""The GPU PNG deflate encoder restated on the host, and the cases it is compared on byte for byte.

``encode(img)`` is a plain numpy / Python encoder written from the rules the kernels of ``gsr_frameio.hip`` document (the block
"Compressed PNGs" and the comments of the kernels behind it; DESIGN.md states the ties those comments leave open).  Every decision in
it is an integer one, so the file it returns is THE file: the GPU tests ask ``encode_png_gpu_deflate`` for the same bytes.  Beside the
file it returns a trace -- tokens, histogram, depths, what the length limiter did, where each block lies -- from which the CPU tests
assert that a case reaches the path it was built for, instead of hoping that the code under test did.

The cases are mostly ONE-ROW images: with H = 1 the Paeth predictor is the left pixel, the image is the per-channel running sum of
the residuals, and the filtered stream is a free design variable (``row_image``).

``rules`` (``encode(..., **rules)``) switches single rules to a neighbouring one (another match threshold, the other tie rule, the
length limiter starting from the other end).  The CPU tests use it to show that the cases tell the rule from its neighbour: a
neighbour's file differs on some case, so a kernel that followed it would be seen.
"""
from __future__ import annotations

import functools
import struct
import zlib

import numpy as np

BLOCK = 16384          # filtered-stream bytes per deflate block
PIECE = 64             # ... per independently tokenised piece
HEADER_BITS = 1222     # 3 + 14 + 19 * 3 + 287 * 4
EOB = 256
N_SYMS = 286

# RFC 1951 3.2.5: length symbol -> (extra bits, first length), as far as 64 reaches
_LENGTH_TABLE = [(257, 0, 3), (258, 0, 4), (259, 0, 5), (260, 0, 6), (261, 0, 7), (262, 0, 8), (263, 0, 9), (264, 0, 10),
                 (265, 1, 11), (266, 1, 13), (267, 1, 15), (268, 1, 17), (269, 2, 19), (270, 2, 23), (271, 2, 27), (272, 2, 31),
                 (273, 3, 35), (274, 3, 43), (275, 3, 51), (276, 3, 59)]
LENGTH_SYMBOLS = [s for s, _, _ in _LENGTH_TABLE]


def length_code(n: int):
    """Match length 3 .. 64 -> (symbol, extra bits, extra value)."""
    assert 3 <= n <= 64
    for sym, ebits, base in reversed(_LENGTH_TABLE):
        if n >= base:
            assert n - base < (1 << ebits)
            return sym, ebits, n - base
    raise AssertionError(n)


def paeth_stream(img: np.ndarray) -> np.ndarray:
    """The scanline stream of ``img`` with every row Paeth-filtered (PNG filter type 4), [H, 1 + W*C] uint8."""
    H, W, C = img.shape
    raw = img.reshape(H, W * C).astype(np.int16)
    left, up, ul = np.zeros_like(raw), np.zeros_like(raw), np.zeros_like(raw)
    left[:, C:] = raw[:, :-C]
    up[1:] = raw[:-1]
    ul[1:, C:] = raw[:-1, :-C]
    p = left + up - ul
    pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - ul)
    pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
    return np.concatenate((np.full((H, 1), 4, np.uint8), ((raw - pred) & 255).astype(np.uint8)), axis=1)


# ---- tokens -----------------------------------------------------------------------------------------------------------------

def tokenize(stream: np.ndarray, min_match: int = 3):
    """(positions, lengths) of the tokens: length 1 is the literal ``stream[pos]``, length >= 3 a match of distance 1.

    Per 64-byte piece: a byte equal to its predecessor (which may lie in the piece or block before; the stream's first byte has none)
    starts a run, clipped to the piece and to the stream's end; a clipped length of ``min_match`` or more is one match, otherwise
    the byte is a literal and the walk moves one byte on."""
    n = len(stream)
    pieces = (n + PIECE - 1) // PIECE
    same = np.zeros(pieces * PIECE, bool)
    same[1:n] = stream[1:] == stream[:-1]
    same = same.reshape(pieces, PIECE)
    run = np.zeros((pieces, PIECE + 1), np.int32)          # bytes from here on, inside the piece and the stream, that equal their predecessor
    for j in range(PIECE - 1, -1, -1):
        run[:, j] = np.where(same[:, j], run[:, j + 1] + 1, 0)
    pos, lens = [], []
    for p in range(pieces):
        first, count = p * PIECE, min(PIECE, n - p * PIECE)
        if not same[p].any():
            pos.extend(range(first, first + count))
            lens.extend([1] * count)
            continue
        r, i = run[p], 0
        while i < count:
            k = int(r[i])
            if k >= min_match:
                pos.append(first + i)
                lens.append(k)
                i += k
            else:
                pos.append(first + i)
                lens.append(1)
                i += 1
    return np.asarray(pos, np.int64), np.asarray(lens, np.int64)


def token_symbols(stream: np.ndarray, pos: np.ndarray, lens: np.ndarray) -> np.ndarray:
    sym_of_len = np.zeros(PIECE + 1, np.int64)
    for k in range(3, PIECE + 1):
        sym_of_len[k] = length_code(k)[0]
    return np.where(lens == 1, stream[pos].astype(np.int64), sym_of_len[lens])


# ---- the code ---------------------------------------------------------------------------------------------------------------

def merge_depths(weights, tie_leaf: bool = True):
    """Huffman's algorithm on leaves sorted ascending, with two queues (leaves; internal nodes in creation order): the depth of every
    leaf, unclamped.  Equal heads: the leaf goes first (``tie_leaf``)."""
    n = len(weights)
    if n == 1:
        return [1]
    inf = float("inf")
    node_w, parent_of_leaf, parent_of_node = [], [0] * n, [0] * (n - 1)
    li = ni = 0
    for k in range(n - 1):
        w = 0
        for _ in range(2):
            lw = weights[li] if li < n else inf
            nw = node_w[ni] if ni < len(node_w) else inf
            if (lw <= nw) if tie_leaf else (lw < nw):
                parent_of_leaf[li] = k
                li += 1
                w += lw
            else:
                parent_of_node[ni] = k
                ni += 1
                w += nw
        node_w.append(w)
    depth_of_node = [0] * (n - 1)                           # the root is the last node made
    for k in range(n - 3, -1, -1):
        depth_of_node[k] = depth_of_node[parent_of_node[k]] + 1
    return [depth_of_node[parent_of_leaf[j]] + 1 for j in range(n)]


def limit_lengths(depths, limit_from_largest: bool = True):
    """Depths clamped to 15 -> (count per length [16], the ``bits`` each run of the length-limit loop picked).

    While the Kraft sum exceeds 2^15: take one code from the largest ``bits <= 14`` that has one, give ``bits + 1`` two, take one
    from 15 (each run lowers the sum by exactly one)."""
    count_of = [0] * 16
    for d in depths:
        count_of[min(d, 15)] += 1
    picks = []
    while len(depths) >= 2 and sum(count_of[d] << (15 - d) for d in range(1, 16)) > (1 << 15):
        order = range(14, 0, -1) if limit_from_largest else range(1, 15)
        bits = next(b for b in order if count_of[b])
        count_of[bits] -= 1
        count_of[bits + 1] += 2
        count_of[15] -= 1
        picks.append(bits)
    return count_of, picks


def canonical_codes(lengths: np.ndarray) -> np.ndarray:
    """RFC 1951 3.2.2: codes by length, then by symbol."""
    count_of = np.bincount(lengths, minlength=16)
    count_of[0] = 0
    next_code, code = [0] * 16, 0
    for d in range(1, 16):
        code = (code + int(count_of[d - 1])) << 1
        next_code[d] = code
    codes = np.zeros(len(lengths), np.int64)
    for s, d in enumerate(lengths):
        if d:
            codes[s] = next_code[d]
            next_code[d] += 1
    return codes


def _reverse_bits(v: np.ndarray, n: np.ndarray) -> np.ndarray:
    out = np.zeros_like(v)
    for b in range(16):
        out |= np.where(b < n, ((v >> b) & 1) << np.maximum(n - 1 - b, 0), 0)
    return out


def _pack_fields(values: np.ndarray, nbits: np.ndarray, total_bits: int) -> np.ndarray:
    """Bit fields, each least significant bit first, one behind the other -> bytes (deflate's bit order), zero padded to ``total_bits``."""
    start = np.concatenate(([0], np.cumsum(nbits)[:-1]))
    assert int(nbits.sum()) <= total_bits and total_bits % 8 == 0
    bits = np.zeros(total_bits, np.uint8)
    for b in range(int(nbits.max())):
        m = nbits > b
        bits[start[m] + b] = (values[m] >> b) & 1
    return np.packbits(bits, bitorder="little")


def _chunk(tag: bytes, body: bytes) -> bytes:
    return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xFFFFFFFF)


# ---- the file ---------------------------------------------------------------------------------------------------------------

def encode(img: np.ndarray, planar_irrelevant=None, *, min_match: int = 3, tie_leaf: bool = True, limit_from_largest: bool = True):
    """uint8 ``[H,W,3|4]`` -> ``(file_bytes, trace)``.  How the source is laid out in memory (interleaved or planar) does not enter.

    ``trace``: ``stream`` (the filtered bytes); ``blocks``: per block its ``type`` ("dynamic" / "stored"), byte ``offset`` in the file,
    ``size`` and, for a dynamic block, ``end_bit`` (bits from the block's first byte to behind its end-of-block code: where the sync
    marker starts); ``token_pos`` / ``token_len`` / ``token_sym`` / ``token_block``: the tokens (length 1: a literal); ``hist`` and
    ``hist_blocks``; ``sorted``: the used symbols as (count, symbol); ``depths``: their unclamped depths in that order;
    ``limit_picks``: the ``bits`` every run of the length-limit loop picked; ``lengths`` and ``codes`` (bit-reversed) by symbol."""
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] in (3, 4)
    H, W, C = img.shape
    stream = paeth_stream(img).reshape(-1)
    n = len(stream)
    blocks = (n + BLOCK - 1) // BLOCK
    pos, lens = tokenize(stream, min_match)
    syms = token_symbols(stream, pos, lens)
    block_of = pos // BLOCK
    hist_blocks = np.zeros((blocks, N_SYMS), np.int64)
    np.add.at(hist_blocks, (block_of, syms), 1)
    hist_blocks[:, EOB] += 1                                 # one end-of-block per block, whatever the block's type turns out to be
    hist = hist_blocks.sum(axis=0)

    used = sorted((int(hist[s]), s) for s in range(N_SYMS) if hist[s])     # by (count, symbol)
    depths = merge_depths([c for c, _ in used], tie_leaf)
    count_of, picks = limit_lengths(depths, limit_from_largest)
    dealt = [d for d in range(15, 0, -1) for _ in range(count_of[d])]      # by sorted position: the rarest gets the longest
    lengths = np.zeros(N_SYMS, np.int64)
    for (_, s), d in zip(used, dealt):
        lengths[s] = d
    codes = _reverse_bits(canonical_codes(lengths), lengths)               # as they go into the stream: first bit of the code in bit 0

    # a dynamic block's header: BFINAL, BTYPE 10, HLIT 29, HDIST 0, HCLEN 15, the code-length code (0 bits for 16 .. 18, 4 bits for the
    # lengths 0 .. 15, whose canonical codes are then the lengths themselves), 286 + 1 lengths, the single distance length being 1
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    head_v = [0, 2, 29, 0, 15] + [0 if o >= 16 else 4 for o in order]
    head_n = [1, 2, 5, 5, 4] + [3] * 19
    all_lengths = np.concatenate((lengths, [1]))
    head_v = np.concatenate((np.asarray(head_v, np.int64), _reverse_bits(all_lengths, np.full(287, 4, np.int64))))
    head_n = np.concatenate((np.asarray(head_n, np.int64), np.full(287, 4, np.int64)))
    assert int(head_n.sum()) == HEADER_BITS

    extra_bits = np.zeros(N_SYMS, np.int64)                  # of a match symbol: its extra bits and the 1-bit distance code
    for sym, eb, _ in _LENGTH_TABLE:
        extra_bits[sym] = eb + 1
    body, trace_blocks, at = b"", [], 8 + 25 + 8 + 2         # signature, IHDR chunk, IDAT length and type, 78 01
    for b in range(blocks):
        lo, blen, last = b * BLOCK, min(BLOCK, n - b * BLOCK), b + 1 == blocks
        bits = int((hist_blocks[b] * (lengths + extra_bits)).sum())
        size = (HEADER_BITS + bits + 7) // 8 if last else (HEADER_BITS + bits + 3 + 7) // 8 + 4
        if size <= 5 + blen:
            m = block_of == b
            tsym, tlen = syms[m], lens[m]
            v, nb = [head_v], [head_n]
            # per token: the symbol's code; for a match its extra bits and the distance code (one 0 bit) behind it
            ev = np.array([length_code(int(k))[2] if k > 1 else 0 for k in tlen], np.int64)
            tv = np.stack((codes[tsym], ev), axis=1).reshape(-1)
            tn = np.stack((lengths[tsym], extra_bits[tsym]), axis=1).reshape(-1)
            keep = tn > 0
            v += [tv[keep], [codes[EOB]]]
            nb += [tn[keep], [lengths[EOB]]]
            v, nb = np.concatenate(v).astype(np.int64), np.concatenate(nb).astype(np.int64)
            v[0] = 1 if last else 0
            end_bit = int(nb.sum())
            assert end_bit == HEADER_BITS + bits
            data = _pack_fields(v, nb, 8 * size).tobytes()
            if not last:                                     # three zero bits, padding to a byte, 00 00 FF FF
                assert not any(data[-4:]) and (end_bit + 3 + 7) // 8 == size - 4
                data = data[:-2] + b"\xff\xff"
            kind = "dynamic"
        else:
            data = struct.pack("<BHH", 1 if last else 0, blen, blen ^ 0xFFFF) + stream[lo:lo + blen].tobytes()
            size, end_bit, kind = 5 + blen, None, "stored"
        assert len(data) == size
        trace_blocks.append({"type": kind, "offset": at, "size": size, "end_bit": end_bit})
        body += data
        at += size
    idat = b"\x78\x01" + body + struct.pack(">I", zlib.adler32(stream.tobytes()) & 0xFFFFFFFF)
    file = (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 6 if C == 4 else 2, 0, 0, 0)) + _chunk(b"IDAT", idat)
            + _chunk(b"IEND", b""))
    trace = {"stream": stream, "blocks": trace_blocks, "token_pos": pos, "token_len": lens, "token_sym": syms, "token_block": block_of,
             "hist": hist, "hist_blocks": hist_blocks, "sorted": used, "depths": depths, "limit_picks": picks, "lengths": lengths,
             "codes": codes}
    return file, trace


# ---- building blocks of the cases -------------------------------------------------------------------------------------------------

def row_image(stream) -> np.ndarray:
    """The one-row image whose filtered stream is ``stream`` (which starts with the filter type, 4): per channel, the running sum of the
    residuals mod 256.  The stream's length decides the channel count: 1 + 3 W, else 1 + 4 W."""
    stream = np.asarray(stream, np.uint8)
    assert stream[0] == 4
    resid = stream[1:]
    C = 3 if len(resid) % 3 == 0 else 4
    assert len(resid) % C == 0 and len(resid) > 0, f"a stream of {len(stream)} bytes is neither 1 + 3 W nor 1 + 4 W"
    img = (np.cumsum(resid.reshape(-1, C).astype(np.int64), axis=0) & 255).astype(np.uint8)[None]
    assert np.array_equal(paeth_stream(img).reshape(-1), stream)
    return img


def filler(n: int, start: int = 0) -> np.ndarray:
    """Bytes cycling through 1, 2, 3 by stream position: no two neighbours equal, none equal to the filter type."""
    return (1 + (start + np.arange(n)) % 3).astype(np.uint8)


def filler_stream(n: int) -> np.ndarray:
    s = filler(n)
    s[0] = 4
    return s


def spread(counts: dict) -> list:
    """The multiset ``{value: count}`` in an order in which no two neighbours are equal (the largest count at most half, rounded up):
    values by falling count into the even places, then the odd ones."""
    items = [v for v, c in sorted(counts.items(), key=lambda kv: (-kv[1], kv[0])) for _ in range(c)]
    out = [None] * len(items)
    out[0::2] = items[:(len(items) + 1) // 2]
    out[1::2] = items[(len(items) + 1) // 2:]
    assert all(a != b for a, b in zip(out, out[1:]))
    return out


def stream_of_counts(lit_counts: dict, units=()) -> np.ndarray:
    """A stream whose token histogram is ``lit_counts`` (literal value -> count; the filter byte is one of the 4s) plus one match of
    length n behind a head literal of value v for every ``(v, n)`` of ``units`` (the heads are taken from v's count).  Every unit lies
    inside one piece, between two bytes that differ from v; no other two neighbours are equal."""
    counts = dict(lit_counts)
    counts[4] = counts.get(4, 0) - 1
    for v, _ in units:
        counts[v] -= 1
    assert all(c >= 0 for c in counts.values())
    lits = spread({v: c for v, c in counts.items() if c})
    out, todo, i = [4], list(units), 0
    while i < len(lits) or todo:
        if todo:
            v, n = todo[0]
            nxt = lits[i] if i < len(lits) else None
            if out[-1] != v and nxt != v and len(out) % PIECE + n + 1 <= PIECE:
                out += [v] * (n + 1)
                todo.pop(0)
                continue
        assert i < len(lits), "literals ran out before every match was placed"
        out.append(lits[i])
        i += 1
    return np.asarray(out, np.uint8)


def fit_row(make, tries: int = 12):
    """``make(extra)`` for the first ``extra`` in 0, 1, ... whose stream is as long as a one-row image's (1 + 3 W or 1 + 4 W)."""
    for extra in range(tries):
        s = make(extra)
        if (len(s) - 1) % 3 == 0 or (len(s) - 1) % 4 == 0:
            return s
    raise AssertionError("no fitting length")


# ---- the cases ------------------------------------------------------------------------------------------------------------------

RUN_VALUE = 200
SWEEP_CHUNKS = 8


def sweep_layout(chunk: int):
    """Run sweep, offsets 8 chunk .. 8 chunk + 7: ``(stream, [(offset, run, position)])``.  One run per slot of two or three pieces
    between fillers: a head byte of RUN_VALUE at position - 1 and ``run`` more behind it, each equal to its predecessor, the first of
    them at ``offset`` within its piece."""
    slots, at = [], 2 * PIECE
    for o in range(8 * chunk, 8 * chunk + 8):
        for r in range(1, 67):
            slots.append((o, r, at + o))
            at += PIECE * ((o + r + 2 + PIECE - 1) // PIECE)    # (a filler byte behind the run, and one more in front of the next head)
    n = row_len(at + PIECE)
    s = filler_stream(n)
    for o, r, p in slots:
        s[p - 1:p + r] = RUN_VALUE
    return s, slots


def _with_run(s, at, n, value=RUN_VALUE):
    s[at:at + n] = value
    return s


def _noise_after(prev: int, n: int, seed: int, then=(1, 2, 3, 4)) -> np.ndarray:
    """n noise bytes behind the byte ``prev`` in which no byte equals its predecessor (steps of 1 .. 255 mod 256): nothing for the
    tokeniser, nothing for the code -- a block of it goes out stored.  The last byte is none of ``then`` (what may follow it)."""
    g = np.random.default_rng(seed)
    v = ((int(prev) + np.cumsum(g.integers(1, 256, n))) % 256).astype(np.uint8)
    while int(v[-1]) in then or (n > 1 and v[-1] == v[-2]) or (n == 1 and v[-1] == prev):
        v[-1] = (int(v[-1]) + 1) % 256
    return v


def row_len(n: int) -> int:
    """The smallest stream length >= n that a one-row image has (1 + 3 W or 1 + 4 W)."""
    while (n - 1) % 3 and (n - 1) % 4:
        n += 1
    return n


def _seam_stream(name: str) -> np.ndarray:
    if name == "match_behind_dynamic":                       # a run over the seam: block 1 starts with a match whose source is block 0's last byte
        return _with_run(filler_stream(row_len(BLOCK + 900)), BLOCK - 1, 11)
    if name == "match_behind_stored":                        # 16 383 noise bytes behind the filter byte, then a run that continues the last of them
        s = filler_stream(row_len(BLOCK + 900))
        s[1:BLOCK] = _noise_after(4, BLOCK - 1, 11)
        return _with_run(s, BLOCK, 10, int(s[BLOCK - 1]))
    if name == "dynamic_stored":                             # the last block stored, behind a sync marker
        s = filler_stream(row_len(BLOCK + 1000))
        s[BLOCK:] = _noise_after(s[BLOCK - 1], len(s) - BLOCK, 12)
        return s
    if name == "dynamic_stored_dynamic":                     # a stored block between two sync markers
        s = filler_stream(row_len(2 * BLOCK + 1000))
        s[BLOCK:2 * BLOCK] = _noise_after(s[BLOCK - 1], BLOCK, 13)
        return _with_run(s, 2 * BLOCK + 70, 40)
    if name == "stored_stored_dynamic":
        s = filler_stream(row_len(2 * BLOCK + 3000))
        s[1:2 * BLOCK] = _noise_after(4, 2 * BLOCK - 1, 14)
        return s
    if name == "short_last_piece_in_a_run":                  # the stream ends 37 bytes into a piece, inside a run that began 10 bytes earlier
        n = 5 * PIECE + 37
        return _with_run(filler_stream(n), n - 11, 11)
    if name == "short_last_piece_run_over_the_piece_seam":   # ... 5 bytes into a piece, inside a run that came in from the piece before
        n = 7 * PIECE + 5
        return _with_run(filler_stream(n), n - 9, 9)
    if name == "four_blocks_exactly":                        # 1 x 21845 x 3; runs over every block seam, the last one up to the stream's end
        s = filler_stream(4 * BLOCK)
        for b in (1, 2, 3):
            _with_run(s, b * BLOCK - 5, 5 + 3 * b)
        _with_run(s, BLOCK + 640, 130)
        return _with_run(s, 4 * BLOCK - 70, 70)
    raise KeyError(name)


SEAMS = ["match_behind_dynamic", "match_behind_stored", "dynamic_stored", "dynamic_stored_dynamic", "stored_stored_dynamic",
         "short_last_piece_in_a_run", "short_last_piece_run_over_the_piece_seam", "four_blocks_exactly"]

# one length per length symbol, the shortest
_UNIT_LENGTHS = [base for _, _, base in _LENGTH_TABLE]


def _alphabet_equal() -> np.ndarray:
    """All 256 literals, all 20 length symbols and end-of-block, once each: one block.  The head of every match is one of the literals."""
    units = sorted(((100 + k, n) for k, n in enumerate(_UNIT_LENGTHS)), key=lambda u: -u[1])
    return stream_of_counts({v: 1 for v in range(256)}, units)


def _alphabet_distinct() -> np.ndarray:
    """The same 277 symbols with 277 different counts: end-of-block 3 (three blocks), the length symbols 1, 2, 4, 5 .. 21, the literals
    22 .. 277 (a little more for the most frequent one, to make the stream as long as a row).  All matches repeat literal 0."""
    match_counts = [c for c in range(1, 22) if c != 3]
    assert len(match_counts) == 20

    def make(extra):
        lit = {v: 22 + v for v in range(256)}
        lit[0], lit[255] = 277, 22                           # the heads are literal 0s: the 228 matches take theirs from a large count
        lit[0] += extra
        units = [(0, n) for n, c in zip(_UNIT_LENGTHS, match_counts) for _ in range(c)]
        units = [units[i] for i in np.random.default_rng(3).permutation(len(units))]
        return stream_of_counts(lit, units)
    return fit_row(make)


def _alphabet_ties() -> np.ndarray:
    """Counts 1, 1, 2, 4 .. 64 (a chain that weighs 128; one of the 1s is the end-of-block), then 128, 128, 128, 256, 512, 1026: at
    several merges a leaf and a node weigh the same.  The leaf first: lengths 11, 11, 10 .. 5, 4, 4, 4, 3, 3, 1; the node first: 12, 12,
    11 .. 6, 5, 5, 5, 3, 2, 1 -- the same cost, another file."""
    return stream_of_counts({4: 1, 9: 2, 10: 4, 11: 8, 12: 16, 13: 32, 14: 64, 20: 128, 30: 128, 40: 128, 50: 256, 60: 512, 70: 1026})


def _fibonacci(n: int):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f


def _chain_literals() -> np.ndarray:
    """Counts 1, 1, 2, 3, 5 ... 17711 over 22 symbols, the 3 being the three end-of-blocks: Huffman's tree is a chain 21 deep."""
    f = _fibonacci(22)
    values = [4, 9] + [20 + 7 * k for k in range(19)]        # the symbol of every count but the 3
    assert len(set(values)) == 21

    def make(extra):
        lit = dict(zip(values, f[:3] + f[4:]))
        lit[values[-1]] += extra
        return stream_of_counts(lit)
    return fit_row(make)


def _chain_with_matches() -> np.ndarray:
    """The same chain with three of its counts held by match symbols (5: length 3, 13: lengths 11 / 12, 34: lengths 35 .. 42); the
    matches repeat the most frequent literal."""
    f = _fibonacci(22)
    values = [4, 9] + [20 + 7 * k for k in range(19)]
    top = values[-1]

    def make(extra):
        counts = f[:3] + f[4:]
        lit = {v: c for v, c in zip(values, counts) if c not in (5, 13, 34)}
        units = [(top, 3)] * 5 + [(top, 11 + k % 2) for k in range(13)] + [(top, 35 + k % 8) for k in range(34)]
        lit[top] += extra
        return stream_of_counts(lit, units)
    return fit_row(make)


PHASE_FAMILY = 34


def _phase_stream(j: int) -> np.ndarray:
    """Two blocks of filler with j bytes of block 0 turned into literal 77: a longer code than the filler's two bits, whose length also
    shrinks as j grows, so the end of block 0 wanders through the bit and byte phases."""
    s = filler_stream(row_len(BLOCK + 640))
    s[100 + 7 * np.arange(j)] = 77
    return _with_run(s, BLOCK + 70, 20)


MULTI_ROW_SHAPES = [(7, 5, 4), (64, 33, 3), (4, 4095, 4), (300, 100, 4)]
MULTI_ROW_KINDS = ["noise", "ramp", "flat", "mixed"]


def multi_row_images(shape, seed):
    """What a frame can look like to the encoder (the images of the decode tests in test_frame_io.py): noise, a smooth ramp with a little
    noise, large flat areas, all of it in one image."""
    h, w, c = shape
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    noise = g.integers(0, 256, shape).astype(np.uint8)
    ramp = ((xx[..., None] * (3 + np.arange(c)) + yy[..., None] * 2 + g.integers(0, 3, shape)) % 256).astype(np.uint8)
    flat = np.zeros(shape, np.uint8)
    flat[h // 3:, w // 4:] = ramp[h // 3:, w // 4:]
    mixed = ramp.copy()
    mixed[: h // 2, : w // 2] = noise[: h // 2, : w // 2]
    mixed[h // 2:, w // 2:] = 17
    return {"noise": noise, "ramp": ramp, "flat": flat, "mixed": mixed}


CASE_IDS = ([f"sweep{c}" for c in range(SWEEP_CHUNKS)] + [f"seam:{s}" for s in SEAMS]
            + ["alphabet:constant", "alphabet:equal", "alphabet:distinct", "alphabet:ties", "limit:literals", "limit:matches"]
            + [f"phase{j}" for j in range(PHASE_FAMILY)]
            + [f"rows:{kind}:{h}x{w}x{c}" for (h, w, c) in MULTI_ROW_SHAPES for kind in MULTI_ROW_KINDS])
# the ids the GPU tests parametrize over one by one (the phase family goes through one test)
SINGLE_IDS = [i for i in CASE_IDS if not i.startswith("phase")]


@functools.lru_cache(maxsize=None)
def case_image(case_id: str) -> np.ndarray:
    if case_id.startswith("sweep"):
        img = row_image(sweep_layout(int(case_id[5:]))[0])
    elif case_id.startswith("seam:"):
        img = row_image(_seam_stream(case_id[5:]))
    elif case_id == "alphabet:constant":
        img = np.zeros((1, 1365, 3), np.uint8)
    elif case_id == "alphabet:equal":
        img = row_image(_alphabet_equal())
    elif case_id == "alphabet:distinct":
        img = row_image(_alphabet_distinct())
    elif case_id == "alphabet:ties":
        img = row_image(_alphabet_ties())
    elif case_id == "limit:literals":
        img = row_image(_chain_literals())
    elif case_id == "limit:matches":
        img = row_image(_chain_with_matches())
    elif case_id.startswith("phase"):
        img = row_image(_phase_stream(int(case_id[5:])))
    elif case_id.startswith("rows:"):
        _, kind, dims = case_id.split(":")
        h, w, c = (int(v) for v in dims.split("x"))
        img = multi_row_images((h, w, c), h * 131 + w + c)[kind]
    else:
        raise KeyError(case_id)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def case(case_id: str):
    """``(img, file_bytes, trace)`` of a case, computed once per process and left unchanged."""
    img = case_image(case_id)
    file, trace = encode(img)
    return img, file, trace


def first_difference(got: bytes, want: bytes):
    """None if equal, else the first offset at which the two differ (the shorter one's length if one is a prefix of the other)."""
    if got == want:
        return None
    a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    n = min(len(a), len(b))
    d = np.flatnonzero(a[:n] != b[:n])
    return int(d[0]) if len(d) else n
