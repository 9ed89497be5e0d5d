"""zlib streams written by hand, for the wave's inflate (csrc/gsr_inflate_core.h): the streams zlib's own encoder never writes.

A WRITER only -- a bit writer, the three block types of RFC 1951, the zlib wrapper of RFC 1950 -- and nothing of a decoder: what a
stream must inflate to is the replay of the tokens it was written from (``replay``), and every stream meant to be good is held to
``zlib.decompress(stream) == replay`` where the corpus is built (``good``), every stream meant to be bad to zlib refusing it
(``corpus_d``).
zlib is the reference; the writer is not trusted on its own.

Tokens: an ``int`` is a literal byte, a pair ``(length, distance)`` a match, a ``Raw`` names its symbols and extra bits itself (the
symbols that do not exist).  The corpora (``corpus_a`` ... ``corpus_d``) are seeded and cached: the CPU, sanitizer and GPU tests read the
same lists.
"""
from __future__ import annotations

import functools
import struct
import zlib
from collections import namedtuple

import numpy as np

from png_deflate_cases import canonical_codes

WINDOW = 32768
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)

# inflate::Status (csrc/gsr_inflate_core.h)
OK, BAD_HEADER, BAD_BLOCK_TYPE, BAD_STORED, BAD_LENGTHS, BAD_CODE, BAD_DISTANCE, OUTPUT_OVERFLOW, INPUT_OVERRUN, BAD_CHECKSUM, SHORT_OUTPUT = range(11)

# RFC 1951 3.2.5, as the table it is printed as
LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LENGTH_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)

# a token that spells out its symbols: literal / length symbol, its extra bits (value, count), and for a length symbol the distance
# symbol and its extra bits (dsym None: nothing follows)
Raw = namedtuple("Raw", "lsym lextra dsym dextra", defaults=((0, 0), None, (0, 0)))


def length_symbol(n: int):
    """Match length 3 ... 258 -> (symbol, extra value, extra bits); 258 has its own symbol."""
    assert 3 <= n <= 258
    k = 28 if n == 258 else max(i for i in range(28) if LENGTH_BASE[i] <= n)
    assert n - LENGTH_BASE[k] < (1 << LENGTH_EXTRA[k])
    return 257 + k, n - LENGTH_BASE[k], LENGTH_EXTRA[k]


def distance_symbol(d: int):
    assert 1 <= d <= WINDOW
    k = max(i for i in range(30) if DIST_BASE[i] <= d)
    assert d - DIST_BASE[k] < (1 << DIST_EXTRA[k])
    return k, d - DIST_BASE[k], DIST_EXTRA[k]


_LENGTH_SYMBOL = [None] * 3 + [length_symbol(n) for n in range(3, 259)]


class BitWriter:
    """Bits in deflate's order: the first bit written is the least significant bit of the first byte."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.cnt = 0

    def put(self, value: int, n: int):
        """A field of n bits, least significant bit first (header fields, extra bits)."""
        assert 0 <= value < (1 << n) or n == 0 and value == 0
        self.acc |= value << self.cnt
        self.cnt += n
        while self.cnt >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.cnt -= 8

    def code(self, word: int, n: int):
        """A Huffman code word of n bits, most significant bit first."""
        assert n > 0, "a symbol without a code word"
        self.put(int(f"{word:0{n}b}"[::-1], 2), n)

    def align(self):
        if self.cnt:
            self.put(0, 8 - self.cnt)

    def raw(self, data: bytes):
        assert self.cnt == 0
        self.out += data

    def bit_length(self) -> int:
        return 8 * len(self.out) + self.cnt

    def done(self) -> bytes:
        self.align()
        return bytes(self.out)


def _write_tokens(w: BitWriter, tokens, lit_code, lit_len, dist_code, dist_len):
    for t in tokens:
        if isinstance(t, Raw):
            w.code(int(lit_code[t.lsym]), int(lit_len[t.lsym]))
            w.put(*t.lextra)
            if t.dsym is not None:
                w.code(int(dist_code[t.dsym]), int(dist_len[t.dsym]))
                w.put(*t.dextra)
        elif isinstance(t, tuple):
            ls, lv, ln = _LENGTH_SYMBOL[t[0]]
            ds, dv, dn = distance_symbol(t[1])
            w.code(int(lit_code[ls]), int(lit_len[ls]))
            w.put(lv, ln)
            w.code(int(dist_code[ds]), int(dist_len[ds]))
            w.put(dv, dn)
        else:
            w.code(int(lit_code[t]), int(lit_len[t]))


_FIXED_LIT = np.array([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
_FIXED_DIST = np.array([5] * 32)


def fixed_block(tokens, end=True):
    """A fixed-code block (RFC 1951 3.2.6).  ``end=False`` leaves the end-of-block symbol out (for streams that are cut there)."""
    def emit(w: BitWriter, final: bool):
        w.put(int(final), 1)
        w.put(1, 2)
        _write_tokens(w, list(tokens) + ([256] if end else []), canonical_codes(_FIXED_LIT), _FIXED_LIT, canonical_codes(_FIXED_DIST), _FIXED_DIST)
    return emit


def stored_block(data: bytes, length=None, nlen=None):
    """A stored block.  ``length`` / ``nlen``: what the LEN / NLEN fields say, if not the truth."""
    assert len(data) <= 65535
    def emit(w: BitWriter, final: bool):
        w.put(int(final), 1)
        w.put(0, 2)
        w.align()
        n = len(data) if length is None else length
        w.raw(struct.pack("<HH", n, (n ^ 0xFFFF) if nlen is None else nlen))
        w.raw(data)
    return emit


def stored_blocks(data: bytes):
    """``data`` as stored blocks of at most 65535 bytes."""
    return [stored_block(data[k:k + 65535]) for k in range(0, len(data), 65535)]


def typed_block(block_type: int):
    """Only a block header (for the block type that does not exist)."""
    def emit(w: BitWriter, final: bool):
        w.put(int(final), 1)
        w.put(block_type, 2)
    return emit


def expand_ops(ops):
    """The code lengths a sequence of code-length symbols spells: 0 ... 15 themselves, (16, n) the previous length n times, (17, n) /
    (18, n) n zeros."""
    out = []
    for op in ops:
        if isinstance(op, tuple):
            sym, n = op
            assert (sym, 3 <= n <= 6) == (16, True) or (sym, 3 <= n <= 10) == (17, True) or (sym, 11 <= n <= 138) == (18, True), op
            out += [out[-1] if sym == 16 else 0] * n
        else:
            out.append(op)
    return out


def ops_with_runs(lens, runs):
    """One code-length symbol per length, except the runs the caller places: ``runs`` maps a start index to ``(16 | 17 | 18, count)``."""
    ops, k = [], 0
    while k < len(lens):
        if k in runs:
            ops.append(runs[k])
            k += runs[k][1]
        else:
            ops.append(int(lens[k]))
            k += 1
    assert k == len(lens) and expand_ops(ops) == [int(v) for v in lens], "a run that is not in the lengths"
    return ops


def code_length_code(ops):
    """Lengths (at most 7 bits, Kraft-complete) of the code-length code for the symbols the ops use: the more frequent, the shorter."""
    hist = np.zeros(19, np.int64)
    for op in ops:
        hist[op[0] if isinstance(op, tuple) else op] += 1
    used = [int(s) for s in np.argsort(-hist, kind="stable") if hist[s]]
    if len(used) < 2:                                              # (a one-word code is incomplete: no inflate accepts it here)
        used.append(next(s for s in (0, 8, 16) if s not in used))
    m, k = len(used), len(used).bit_length() - 1
    n_short = (2 << k) - m                                        # n_short words of k bits and 2 (m - 2^k) of k + 1: complete
    lens = np.zeros(19, np.int64)
    for rank, s in enumerate(used):
        lens[s] = k if rank < n_short else k + 1
    return lens


def dynamic_block(lit_lens, dist_lens, header_ops, tokens, hclen=None, hlit=None, hdist=None, cl_lens=None, check=True, end=True):
    """A dynamic block: HLIT / HDIST / HCLEN, the code-length code, ``header_ops`` written with it, the tokens written with the codes
    ``lit_lens`` / ``dist_lens``.  With ``check`` the ops must spell exactly those lengths; a stream with a defect in its header says
    ``check=False`` and, where the 5-bit count fields shall lie, ``hlit`` / ``hdist``."""
    lit_lens, dist_lens = np.asarray(lit_lens, np.int64), np.asarray(dist_lens, np.int64)
    if check:
        assert 257 <= len(lit_lens) <= 286 and 1 <= len(dist_lens) <= 30
        assert expand_ops(header_ops) == [int(v) for v in lit_lens] + [int(v) for v in dist_lens]
    cl = code_length_code(header_ops) if cl_lens is None else np.asarray(cl_lens, np.int64)
    need = max(k for k in range(19) if cl[CL_ORDER[k]]) + 1
    n_cl = max(need, 4) if hclen is None else hclen
    assert need <= n_cl <= 19, f"HCLEN {n_cl} does not reach the code-length code's last length"
    cl_code = canonical_codes(cl)
    def emit(w: BitWriter, final: bool):
        w.put(int(final), 1)
        w.put(2, 2)
        w.put((len(lit_lens) if hlit is None else hlit) - 257, 5)
        w.put((len(dist_lens) if hdist is None else hdist) - 1, 5)
        w.put(n_cl - 4, 4)
        for k in range(n_cl):
            w.put(int(cl[CL_ORDER[k]]), 3)
        for op in header_ops:
            sym, n = op if isinstance(op, tuple) else (op, 0)
            w.code(int(cl_code[sym]), int(cl[sym]))
            if sym >= 16:
                w.put(n - (3, 3, 11)[sym - 16], (2, 3, 7)[sym - 16])
        _write_tokens(w, list(tokens) + ([256] if end else []), canonical_codes(lit_lens), lit_lens, canonical_codes(dist_lens), dist_lens)
    return emit


def replay(tokens, prefix: bytes = b"") -> bytes:
    """What the tokens say, behind ``prefix``: the expected output."""
    out = bytearray(prefix)
    for t in tokens:
        if isinstance(t, tuple):
            n, d = t
            assert 3 <= n <= 258 and 1 <= d <= len(out)
            if d >= n:
                out += out[len(out) - d:len(out) - d + n]
            else:
                out += (bytes(out[-d:]) * (n // d + 1))[:n]
        else:
            out.append(t)
    return bytes(out)


def zlib_stream(blocks, data: bytes, adler=None, finals=None) -> bytes:
    """CMF / FLG (32 KB window, no dictionary), the blocks -- the last one final, or as ``finals`` says -- and the Adler-32 of ``data``."""
    w = BitWriter()
    w.raw(b"\x78\x01")
    for k, block in enumerate(blocks):
        block(w, k == len(blocks) - 1 if finals is None else finals[k])
    w.align()
    w.raw(struct.pack(">I", zlib.adler32(data) if adler is None else adler))
    return w.done()


def zlib_says(stream: bytes, n: int):
    """zlib's inflation of the stream, or None where zlib refuses it, stops before its end or gives another size than ``n``."""
    d = zlib.decompressobj()
    try:
        out = d.decompress(stream)
    except zlib.error:
        return None
    return out if d.eof and len(out) == n else None


def good(stream: bytes, data: bytes):
    assert zlib.decompress(stream) == data, "the builder and zlib disagree on a stream meant to be good"
    return stream, data


# ---- A: every match shape ------------------------------------------------------------------------------------------------------------
A_DISTANCES = (list(range(1, 131)) + [191, 192, 193] + list(range(255, 260)) + [4095, 4096, 4097, 16384] + [32505, 32506, 32507]
               + [32766, 32767, 32768])


@functools.lru_cache(maxsize=None)
def corpus_a():
    """Per distance one fixed-code stream: ``dist + r`` random literals (r in 0 ... 69: the phase against lanes and segments), then for
    every length 3 ... 258 that match and one random literal.  ``[(name, stream, data)]``."""
    g = np.random.default_rng(1951)
    out = []
    for dist in A_DISTANCES:
        r = int(g.integers(0, 70))
        tokens = [int(v) for v in g.integers(0, 256, dist + r)]
        for n, lit in zip(range(3, 259), g.integers(0, 256, 256)):
            tokens += [(n, dist), int(lit)]
        data = replay(tokens)
        out.append((f"A dist={dist} r={r}",) + good(zlib_stream([fixed_block(tokens)], data), data))
    return out


# ---- B: phases against the segment and ring boundaries -------------------------------------------------------------------------------
B_DISTANCES, B_LENGTHS, B_BOUNDARIES = (1, 2, 3, 5, 63, 64, 65, 100, 32768), (3, 64, 65, 129, 258), (4096, 32768, 65536)


@functools.lru_cache(maxsize=None)
def corpus_b():
    """A match that starts ``k`` bytes in front of a boundary B, behind a prefix of stored blocks (a ``bits_seek`` in front of the
    match), followed by 0 ... 17 literals -- the last, partial flush has every size 1 ... 17 somewhere."""
    g = np.random.default_rng(1950)
    prefix = bytes(g.integers(0, 256, max(B_BOUNDARIES), dtype=np.uint8))
    out, tail = [], 0
    for dist in B_DISTANCES:
        for n in B_LENGTHS:
            for boundary in B_BOUNDARIES:
                for k in sorted({0, 1, 2, n - 1, n, n + 1, 259}):
                    at = boundary - k
                    if dist > at:
                        continue
                    tokens = [(n, dist)] + [int(v) for v in g.integers(0, 256, tail)]
                    data = replay(tokens, prefix[:at])
                    stream = zlib_stream(stored_blocks(prefix[:at]) + [fixed_block(tokens)], data)
                    out.append((f"B dist={dist} len={n} at={boundary}-{k} tail={tail}",) + good(stream, data))
                    tail = (tail + 1) % 18
    return out


# ---- C: dynamic headers ------------------------------------------------------------------------------------------------------------
def chain_lengths(n_symbols: int, symbols):
    """A Kraft-complete code with a word of every length 1 ... 15: lengths 1, 2, ..., 14, 15, 15 on the sixteen ``symbols``."""
    assert len(symbols) == 16 and len(set(symbols)) == 16
    lens = np.zeros(n_symbols, np.int64)
    for s, l in zip(symbols, list(range(1, 16)) + [15]):
        lens[s] = l
    return lens


def split_lengths(n_symbols: int, symbols, g, start=(1, 1)):
    """A Kraft-complete code on ``symbols``: from the lengths ``start``, a random word of fewer than 15 bits is split into two until
    every symbol has one."""
    lens = list(start)
    while len(lens) < len(symbols):
        k = int(g.choice([i for i, l in enumerate(lens) if l < 15]))
        lens[k] += 1
        lens.append(lens[k])
    out = np.zeros(n_symbols, np.int64)
    for s, l in zip(symbols, g.permutation(lens)):
        out[s] = l
    return out


def cover_tokens(lit_lens, dist_lens, g):
    """Tokens that use every code word of the two codes at least once: each literal, each length symbol with its extra bits at zero
    and at all ones (so 284 with extra 30), each distance symbol likewise (28 and 29 with all-ones extra bits).  With the largest
    distance they reach: the caller puts that many bytes in front."""
    lit_syms = [s for s in range(min(len(lit_lens), 256)) if lit_lens[s]]
    len_syms = [s for s in range(257, len(lit_lens)) if lit_lens[s]]
    dist_syms = [s for s in range(len(dist_lens)) if dist_lens[s]]
    tokens = list(lit_syms)
    if dist_syms and len_syms:                                     # (without a length symbol the distance code stays unused)
        lengths = []
        for s in len_syms:
            k = s - 257
            lengths += [LENGTH_BASE[k], LENGTH_BASE[k] + (1 << LENGTH_EXTRA[k]) - 1 - (k == 27)]       # (symbol 284's extra 31 would be 258)
        distances = []
        for s in dist_syms:
            distances += [DIST_BASE[s], DIST_BASE[s] + (1 << DIST_EXTRA[s]) - 1]
        for k in range(max(len(lengths), len(distances))):
            tokens.append((lengths[k % len(lengths)], distances[k % len(distances)]))
            if lit_syms:
                tokens.append(lit_syms[int(g.integers(0, len(lit_syms)))])
    else:
        assert not len_syms or not dist_syms
    need = max([t[1] for t in tokens if isinstance(t, tuple)], default=0)
    return tokens, need


def _dynamic_stream(name, g, blocks_spec):
    """``blocks_spec``: per dynamic block ``(lit_lens, dist_lens, runs, keywords of dynamic_block, tokens or None)``.  A stored prefix as
    long as the largest distance, all tokens replayed behind it."""
    made, need = [], 0
    for lit_lens, dist_lens, runs, kw, tokens in blocks_spec:
        if tokens is None:
            tokens, d = cover_tokens(lit_lens, dist_lens, g)
            need = max(need, d)
        made.append((lit_lens, dist_lens, runs, kw, tokens))
    prefix = bytes(g.integers(0, 256, need, dtype=np.uint8))
    blocks, all_tokens = stored_blocks(prefix), []
    for lit_lens, dist_lens, runs, kw, tokens in made:
        ops = ops_with_runs(list(lit_lens) + list(dist_lens), runs)
        blocks.append(dynamic_block(lit_lens, dist_lens, ops, tokens, **kw))
        all_tokens += tokens
    data = replay(all_tokens, prefix)
    return (name,) + good(zlib_stream(blocks, data), data)


@functools.lru_cache(maxsize=None)
def corpus_c():
    """Dynamic headers, a few hundred bytes of output each behind a stored prefix as long as the largest distance used (32 768 where
    distance symbol 29 has a word).  Where ``tokens`` is None every code word of the block is used.  ``[(name, stream, data)]``."""
    g = np.random.default_rng(1952)
    out = []
    add = lambda name, spec: out.append(_dynamic_stream("C " + name, g, spec))
    lit_chain = chain_lengths(286, [65, 66, 0, 255, 256, 257, 264, 265, 97, 284, 285, 10, 32, 268, 277, 128])     # 284: 10 bits, 285: 11
    dist_chain = chain_lengths(30, [0, 1, 2, 3, 5, 8, 12, 28, 29, 16, 17, 20, 23, 25, 26, 27])                    # 28: 8 bits, 29: 9
    lit_wide = split_lengths(286, list(range(286)), g)
    dist_wide = split_lengths(30, list(range(30)), g)
    lit_small = split_lengths(257, [65, 66, 67, 68, 256], g)
    # every word length in both codes, HLIT 286, HDIST 30; HCLEN as small as the lengths allow, and 19
    add("chain codes", [(lit_chain, dist_chain, {}, {}, None)])
    add("chain codes HCLEN=19", [(lit_chain, dist_chain, {}, {"hclen": 19}, None)])
    add("wide codes HLIT=286 HDIST=30", [(lit_wide, dist_wide, {}, {}, None)])
    # zeros by 18: runs of exactly 138 and 11 in the literals, and one of 28 + 10 from the length symbols into the distances
    lit_gap = chain_lengths(286, [0, 150, 151, 152, 153, 154, 155, 156, 157, 158, 159, 160, 161, 256, 257, 162])
    dist_gap = chain_lengths(30, list(range(10, 26)))
    add("18: 138, 11, and literals into distances", [(lit_gap, dist_gap, {1: (18, 138), 139: (18, 11), 258: (18, 38)}, {}, None)])
    # zeros by 17: runs of exactly 3 and 10, and one from the length symbols into the distances (HLIT 260: 257 is coded, 258, 259 not)
    lit_17 = np.zeros(260, np.int64)
    lit_17[[20, 34, 256, 257]] = 2
    dist_17 = np.array([0, 0, 0, 1, 1, 0, 0, 0])
    add("17: 3, 10, and literals into distances; a run ending at n_lit + n_dist",
        [(lit_17, dist_17, {0: (17, 10), 10: (17, 10), 21: (17, 3), 24: (17, 10), 258: (17, 5), 265: (17, 3)}, {}, None)])
    # 16: runs of exactly 3 and 6, the second from the literal lengths into the distance lengths (HLIT 257)
    lit_16 = np.zeros(257, np.int64)
    lit_16[[0, 1, 2, 3]] = 3                                   # 16 x 3 behind lens[0]
    lit_16[[254, 255, 256]] = 3                                # 16 x 6 behind lens[254]: 255, 256 and four distance lengths
    lit_16[100] = 3
    dist_16 = np.array([3, 3, 3, 3, 1])
    add("16: 3, and 6 from literals into distances", [(lit_16, dist_16, {1: (16, 3), 255: (16, 6)}, {}, None)])
    # ... and a 16 and an 18 that end exactly at n_lit + n_dist
    add("16 ending at n_lit + n_dist", [(lit_16, np.array([1, 3, 3, 3, 3]), {259: (16, 3)}, {}, None)])
    lit_18 = np.zeros(257, np.int64)
    lit_18[[7, 256]] = 1
    add("18 ending at n_lit + n_dist; no distance code, literals only; HDIST=30", [(lit_18, np.zeros(30, np.int64), {257: (18, 30)}, {}, [7] * 40)])
    # HDIST 1, the distance code of one word: used (HLIT 258: one length symbol), unused and absent (HLIT 257: no length symbol)
    add("HLIT=258 HDIST=1: one distance word, used", [(split_lengths(258, [65, 66, 67, 256, 257], g), np.array([1]), {}, {}, None)])
    add("HLIT=257 HDIST=1: one distance word, unused", [(lit_small, np.array([1]), {}, {}, [65, 66, 67, 68] * 20)])
    add("HLIT=257 HDIST=1: no distance code", [(lit_small, np.array([0]), {}, {}, [68, 67, 66, 65] * 20)])
    # HCLEN at its smallest for a code that has code words at all: 5 (16, 17, 18, 0, 8) -- with 4 every length is zero, which no
    # inflate accepts (corpus D holds that one)
    lit_8 = np.full(257, 8, np.int64)
    lit_8[255] = 0
    add("HCLEN=5", [(lit_8, np.array([0]), {}, {"hclen": 5}, [int(v) for v in g.integers(0, 255, 300)])])
    # only the end-of-block symbol has a code word: alone (an empty output) and between other blocks
    lit_eob = np.zeros(257, np.int64)
    lit_eob[256] = 1
    add("only an end-of-block word", [(lit_eob, np.array([0]), {}, {}, [])])
    add("only an end-of-block word, between blocks", [(lit_small, np.array([1]), {}, {}, [65, 66] * 9), (lit_eob, np.array([0]), {}, {}, []),
                                                      (lit_chain, dist_chain, {}, {}, None)])
    # the tables rebuilt: two and three dynamic blocks with different codes back to back, long words after short and the reverse
    add("chain after wide", [(lit_wide, dist_wide, {}, {}, None), (lit_chain, dist_chain, {}, {}, None)])
    add("wide after chain after small", [(lit_small, np.array([1]), {}, {}, [65, 66, 67, 68]), (lit_chain, dist_chain, {}, {}, None),
                                         (lit_wide, dist_wide, {}, {}, None)])
    return out


# ---- D: streams that must be refused --------------------------------------------------------------------------------------------------
def _fixed_bits(tokens) -> int:
    """Where the next token of a fixed-code block would start: the bit offset in the zlib stream."""
    w = BitWriter()
    fixed_block(tokens, end=False)(w, True)
    return 16 + w.bit_length()


@functools.lru_cache(maxsize=None)
def corpus_d():
    """``[(name, stream, dst_len, status)]``: the smallest good stream with one defect each, and the status the host lane must give.
    zlib refuses every one (``zlib_says`` is None), asserted here."""
    g = np.random.default_rng(1953)
    out = []

    def add(name, stream, n, status):
        assert zlib_says(stream, n) is None, f"zlib accepts a stream meant to be bad: {name}"
        out.append(("D " + name, stream, n, status))

    fixed = lambda tokens, data, **kw: zlib_stream([fixed_block(tokens)], data, **kw)
    # a distance of pos + 1.  (The largest distance deflate can write is 32768, so the third position is 32767, not 32768.)
    add("distance 1 at 0", fixed([(3, 1)], b"abc"), 3, BAD_DISTANCE)
    add("distance 2 at 1", fixed([97, (3, 2)], b"aaaa"), 4, BAD_DISTANCE)
    far = bytes(g.integers(0, 256, 32767, dtype=np.uint8))
    add("distance 32768 at 32767", zlib_stream(stored_blocks(far) + [fixed_block([(3, 32768)])], far + b"abc"), 32770, BAD_DISTANCE)
    # one byte more than the caller expects: by a literal, by a match (its last byte), by a stored block
    data = replay([1, 2, 3, 4])
    add("a literal past dst_len", fixed([1, 2, 3, 4], data), 3, OUTPUT_OVERFLOW)
    data = replay([1, 2, 3, (100, 2)])
    add("a match past dst_len", fixed([1, 2, 3, (100, 2)], data), len(data) - 1, OUTPUT_OVERFLOW)
    add("a stored block past dst_len", zlib_stream([stored_block(b"stored")], b"stored"), 5, OUTPUT_OVERFLOW)
    add("one byte short of dst_len", fixed([1, 2, 3, 4], replay([1, 2, 3, 4])), 5, SHORT_OUTPUT)
    # dynamic headers.  The good stream: literals 65 ... 68 and the end-of-block symbol, one distance word
    lit = np.zeros(257, np.int64)
    lit[[65, 66, 67]] = 2
    lit[[68, 256]] = 3
    dist = np.array([1])
    tokens = [65, 66, 67, 68, 65]
    data = replay(tokens)
    lens = [int(v) for v in lit] + [1]
    header = lambda ops, lit_lens=lit, dist_lens=dist, toks=tokens, **kw: zlib_stream(
        [dynamic_block(lit_lens, dist_lens, ops, toks, check=False, **kw)], data)
    assert zlib_says(header(ops_with_runs(lens, {})), len(data)) == data                      # (the good stream the defects are put into)
    cl_all = [0] * 19
    for s in (0, 1, 2, 3):
        cl_all[s] = 3
    for s in (16, 17, 18):
        cl_all[s] = 3
    cl_all[4] = 3                                                 # eight words of three bits: complete, and 16 / 17 / 18 have one each
    add("16 as the first length symbol", header([(16, 3)] + lens[3:], cl_lens=cl_all), len(data), BAD_LENGTHS)
    add("a 17 run one past n_lit + n_dist", header(lens[:256] + [(17, 3)], cl_lens=cl_all), len(data), BAD_LENGTHS)
    add("a 16 run one past n_lit + n_dist", header(lens[:256] + [(16, 3)], cl_lens=cl_all), len(data), BAD_LENGTHS)
    add("an 18 run one past n_lit + n_dist", header([(18, 65)] + lens[65:248] + [(18, 11)], cl_lens=cl_all), len(data), BAD_LENGTHS)
    over = lit.copy()
    over[69] = 2
    add("an over-subscribed literal code", header([int(v) for v in over] + [1], cl_lens=cl_all), len(data), BAD_LENGTHS)
    under = lit.copy()
    under[68] = 0
    add("an incomplete literal code", header([int(v) for v in under] + [1], lit_lens=lit, toks=[65, 66, 67, 65], cl_lens=cl_all), len(data), BAD_LENGTHS)
    no_end = lit.copy()
    no_end[256], no_end[69] = 0, 3
    add("no end-of-block word", header([int(v) for v in no_end] + [1], lit_lens=no_end, toks=[65, 66, 67, 68, 65], end=False, cl_lens=cl_all),
        len(data), BAD_LENGTHS)
    add("HCLEN=4: every length zero", header([(18, 138), (18, 120)], cl_lens=[0] * 16 + [0, 1, 1], hclen=4, toks=[], end=False), 0, BAD_LENGTHS)
    for hlit in (287, 288):
        add(f"HLIT={hlit}", header(lens[:257] + [0] * (hlit - 257) + [1], hlit=hlit, cl_lens=cl_all), len(data), BAD_LENGTHS)
    for hdist in (31, 32):
        add(f"HDIST={hdist}", header(lens[:257] + [1] + [0] * (hdist - 1), hdist=hdist, cl_lens=cl_all), len(data), BAD_LENGTHS)
    # symbols the fixed code has words for and deflate has not
    for sym in (286, 287):
        add(f"fixed-code length symbol {sym}", fixed([1, 2, 3, Raw(sym, (0, 0), 0, (0, 0))], bytes(6)), 6, BAD_CODE)
    for sym in (30, 31):
        add(f"fixed-code distance symbol {sym}", fixed([1, 2, 3, Raw(257, (0, 0), sym, (0, 0))], bytes(6)), 6, BAD_CODE)
    add("block type 3", zlib_stream([typed_block(3)], b""), 0, BAD_BLOCK_TYPE)
    add("stored LEN != ~NLEN", zlib_stream([stored_block(b"stored", nlen=6 ^ 0xFFFE)], b"stored"), 6, BAD_STORED)
    add("a stored block longer than the input", zlib_stream([stored_block(b"stored", length=40)], b"stored"), 40, INPUT_OVERRUN)
    # the stream cut at a byte that lies inside a field.  Behind its end the reader delivers zero bits: the cut field reads as a smaller
    # value, and in the fixed code seven zero bits are the end-of-block word -- so each of these decodes on to the end of its block
    # without writing more than the whole stream would, and is refused there for having read past the end.
    def cut_inside(tokens, first_bit, n_bits):
        whole = zlib_stream([fixed_block(tokens)], replay(tokens))
        cut = (first_bit + n_bits - 1) // 8                      # the last byte boundary in front of the field's last bit
        assert first_bit < 8 * cut < first_bit + n_bits and cut >= 6
        return whole[:cut], len(replay(tokens))
    lits = [int(v) for v in g.integers(0, 144, 60)]
    add("cut in a code word", *cut_inside(lits, _fixed_bits(lits[:7]), 8), INPUT_OVERRUN)
    tokens = lits[:7] + [200, (257, 2)]                           # length symbol 284: five extra bits, 30
    add("cut in the extra bits of a length", *cut_inside(tokens, _fixed_bits(tokens[:-1]) + 8, 5), INPUT_OVERRUN)
    tokens = lits + [(3, 48)]                                     # distance symbol 10: four extra bits, 15
    add("cut in the extra bits of a distance", *cut_inside(tokens, _fixed_bits(tokens[:-1]) + 7 + 5, 4), INPUT_OVERRUN)
    whole = zlib_stream([fixed_block([1, 2, 3])], bytes([1, 2, 3]))
    for keep in (0, 1, 3):
        add(f"cut in the Adler-32, {keep} of its bytes left", whole[:len(whole) - 4 + keep], 3, INPUT_OVERRUN)
    add("a wrong Adler-32", zlib_stream([fixed_block([1, 2, 3])], bytes([1, 2, 3]), adler=zlib.adler32(bytes([1, 2, 3])) ^ 1), 3, BAD_CHECKSUM)
    return out


def good_corpora():
    """``[(name, stream, data)]`` of A, B and C."""
    return corpus_a() + corpus_b() + corpus_c()
