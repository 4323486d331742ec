"""A small DEFLATE assembler (RFC 1950 / 1951) and a catalogue of hand-built zlib streams.

Plain Python: nothing of the library is imported and no GPU is needed.  A compressor never writes most of what an inflater
has branches for -- over-subscribed and incomplete code sets, counts beyond their limits, repeat codes in illegal places,
the symbols that must not occur, a distance one past the start, 15-bit codes, the largest legal header -- so the streams
here are assembled field by field, every field settable to an illegal value, and an independent LZ77 replay of what was
emitted (`Deflate.model`) says what a valid stream must inflate to.

`cases()` is the catalogue: named streams with the expected output, the zlib message they are built to provoke, or -- for
the streams that end inside a field -- the bytes zlib hands out before it waits for more input.  tests/test_deflate_craft.py
holds the catalogue to the host's zlib (so that every rule is known to be reached before anything runs on a GPU);
tests/test_gpu_inflate_crafted.py holds k_inflate to the same verdicts."""
from collections import namedtuple

CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEXT = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DBASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
         8193, 12289, 16385, 24577)
DEXT = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)

# the fifteen messages of zlib's inflate.c that a data error can carry
MESSAGES = ("incorrect header check", "unknown compression method", "invalid window size", "invalid block type",
            "invalid stored block lengths", "too many length or distance symbols", "invalid code lengths set",
            "invalid bit length repeat", "invalid code -- missing end-of-block", "invalid literal/lengths set",
            "invalid distances set", "invalid literal/length code", "invalid distance code", "invalid distance too far back",
            "incorrect data check")

# kind: "valid" (expect = the output, the stream ends), "reject" (expect = substring of zlib's message), "ended" (the stream
# stops inside a field: expect = what zlib gives before it waits, no error), "needdict" (preset-dictionary header: Z_NEED_DICT)
Case = namedtuple("Case", "name stream expect kind")


class BitWriter:
    """Plain fields go in LSB first, Huffman codes MSB first (RFC 1951 3.1.1)."""

    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.nacc = 0

    @property
    def bitpos(self):
        return len(self.buf) * 8 + self.nacc

    def bits(self, value, n):
        assert 0 <= value < (1 << n) or (n == 0 and value == 0), (value, n)
        self.acc |= value << self.nacc
        self.nacc += n
        while self.nacc >= 8:
            self.buf.append(self.acc & 255)
            self.acc >>= 8
            self.nacc -= 8

    def code(self, code, n):
        rev = 0
        for i in range(n):
            rev |= ((code >> i) & 1) << (n - 1 - i)
        self.bits(rev, n)

    def align(self):
        if self.nacc:
            self.bits(0, 8 - self.nacc)

    def raw(self, data):
        assert self.nacc == 0
        self.buf += data

    def getvalue(self):
        out = bytes(self.buf)
        return out + bytes([self.acc]) if self.nacc else out


def canonical(lengths):
    """RFC 1951 3.2.2: symbol -> (code, length); symbols of length 0 have no code.  An over-subscribed set still gets its
    numbers (they overflow their widths): such a set is only ever written into a header, never used."""
    count = [0] * 17
    for n in lengths:
        count[n] += 1
    count[0] = 0
    nxt = [0] * 17
    code = 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for n in lengths:
        if n:
            out.append((nxt[n] & ((1 << n) - 1), n))
            nxt[n] += 1
        else:
            out.append(None)
    return out


def complete_lengths(k):
    """k >= 2 code lengths of a complete set, all floor(log2 k) or one more"""
    assert k >= 2
    b = k.bit_length() - 1
    deep = 2 * (k - (1 << b))
    return [b] * (k - deep) + [b + 1] * deep


def _table(spec, least):
    if isinstance(spec, dict):
        n = max(max(spec) + 1 if spec else 0, least)
        return [spec.get(i, 0) for i in range(n)]
    return list(spec)


def adler32(data):
    s1, s2 = 1, 0
    for i in range(0, len(data), 3800):
        for b in data[i:i + 3800]:
            s1 += b
            s2 += s1
        s1 %= 65521
        s2 %= 65521
    return (s2 << 16) | s1


FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


class Deflate:
    """One raw deflate stream under construction, and the record of what its symbols mean."""

    def __init__(self):
        self.w = BitWriter()
        self.ops = []            # ("lit", byte, end bit) | ("match", length, distance, end bit) | ("stored", bytes, first bit)
        self.ll = self.dd = None
        self._len = None
        self.marks = {}          # bit positions of the fields of the last block header written

    # ---- blocks ----
    def stored(self, data, final=False, len_=None, nlen=None):
        self.marks = {"hdr": self.w.bitpos}
        self.w.bits(int(final), 1)
        self.w.bits(0, 2)
        self.w.align()
        self.marks["len"] = self.w.bitpos
        n = len(data) if len_ is None else len_
        self.w.bits(n, 16)
        self.w.bits((n ^ 0xFFFF) if nlen is None else nlen, 16)
        self.marks["data"] = self.w.bitpos
        self.ops.append(("stored", bytes(data), self.w.bitpos))
        self.w.raw(data)

    def block_type(self, btype, final=False):
        self.marks = {"hdr": self.w.bitpos}
        self.w.bits(int(final), 1)
        self.w.bits(btype, 2)

    def fixed(self, final=False):
        self.block_type(1, final)
        self.ll, self.dd = canonical(FIXED_LL), canonical(FIXED_D)

    def dynamic(self, ll_lens, d_lens, final=False, hlit=None, hdist=None, hclen=None, cl_lens=None, tokens=None):
        """ll_lens / d_lens: list, or {symbol: length}.  tokens: the run-length coded lengths as (symbol 0..18, extra bits value)
        in any order and place; default one plain token per length.  cl_lens: {symbol: length} of the code-length code; default
        a complete set over the symbols the tokens use."""
        ll_lens, d_lens = _table(ll_lens, 257), _table(d_lens, 1)
        hlit = len(ll_lens) - 257 if hlit is None else hlit
        hdist = len(d_lens) - 1 if hdist is None else hdist
        if tokens is None:
            tokens = [(n, 0) for n in ll_lens + d_lens]
        if cl_lens is None:
            used = sorted({t[0] for t in tokens})
            while len(used) < 2:
                used.append(next(s for s in (0, 1) if s not in used))
            cl_lens = dict(zip(used, complete_lengths(len(used))))
        cl = _table(cl_lens, 19)
        if hclen is None:
            hclen = max(max([i for i, s in enumerate(CL_ORDER) if cl[s]], default=0) + 1, 4) - 4
        self.block_type(2, final)
        m = self.marks
        m["counts"] = self.w.bitpos
        self.w.bits(hlit, 5)
        self.w.bits(hdist, 5)
        self.w.bits(hclen, 4)
        m["cl"] = []
        for i in range(hclen + 4):
            m["cl"].append(self.w.bitpos)
            self.w.bits(cl[CL_ORDER[i]], 3)
        clc = canonical(cl)
        m["tok"], m["tokx"] = [], []
        for sym, extra in tokens:
            m["tok"].append(self.w.bitpos)
            self.w.code(*clc[sym])
            m["tokx"].append(self.w.bitpos)
            if sym >= 16:
                self.w.bits(extra, (2, 3, 7)[sym - 16])
        m["end"] = self.w.bitpos
        self.ll, self.dd = canonical(ll_lens), canonical(d_lens)

    # ---- symbols: the code and its extra bits are given separately ----
    def sym(self, s):
        self.w.code(*self.ll[s])

    def lit(self, b):
        self.sym(b)
        self.ops.append(("lit", b, self.w.bitpos))

    def length(self, s, extra=0):
        self.sym(s)
        if 257 <= s <= 285:
            self.w.bits(extra, LEXT[s - 257])
            self._len = min(LBASE[s - 257] + extra, 258)

    def dist(self, s, extra=0):
        self.w.code(*self.dd[s])
        if s < 30:
            self.w.bits(extra, DEXT[s])
            self.ops.append(("match", self._len, DBASE[s] + extra, self.w.bitpos))

    def match(self, length, distance):
        ls = 28 if length == 258 else max(i for i in range(28) if LBASE[i] <= length)
        ds = max(i for i in range(30) if DBASE[i] <= distance)
        self.length(257 + ls, length - LBASE[ls])
        self.dist(ds, distance - DBASE[ds])

    def eob(self):
        self.sym(256)

    # ---- the model: an LZ77 replay of the recorded symbols ----
    def model(self, upto_bit=None, starts=None):
        """The output of everything that is complete at bit `upto_bit` (a stored block's bytes as far as they are there).
        starts: a list that receives the output position of every match."""
        out = bytearray()
        for op in self.ops:
            if op[0] == "stored":
                n = len(op[1]) if upto_bit is None else max(0, min(len(op[1]), (upto_bit - op[2]) // 8))
                out += op[1][:n]
                if n < len(op[1]):
                    break
                continue
            if upto_bit is not None and op[-1] > upto_bit:
                break
            if op[0] == "lit":
                out.append(op[1])
            else:
                _, n, d, _ = op
                assert 0 < d <= len(out), "the model replays valid streams only"
                if starts is not None:
                    starts.append(len(out))
                for _ in range(n):
                    out.append(out[-d])
        return bytes(out)

    def raw(self):
        return self.w.getvalue()


def zlib_wrap(raw, data=b"", cmf=0x78, flg=None, adler="ok", dictid=None):
    """RFC 1950 around a raw deflate stream.  flg None: the check bits are made right (level bits 2, FDICT when dictid is
    given); adler: "ok", "bad", "none", or the four bytes themselves."""
    if flg is None:
        flg = 0x80 | (0x20 if dictid is not None else 0)
        flg += 31 - ((cmf << 8) | flg) % 31
        assert ((cmf << 8) | flg) % 31 == 0 and flg < 256
    a = adler32(data)
    tail = {"ok": a.to_bytes(4, "big"), "bad": (a ^ 0x00010000).to_bytes(4, "big"), "none": b""}.get(adler, adler)
    return bytes([cmf, flg]) + (dictid.to_bytes(4, "big") if dictid is not None else b"") + raw + tail


def _wrap(d, **kw):
    return zlib_wrap(d.raw(), d.model() if kw.get("adler", "ok") in ("ok", "bad") else b"", **kw)


def noise(n, seed=1):
    """n bytes without long repeats (a multiplicative generator: no library, same bytes everywhere)"""
    x = seed * 2654435761 % (1 << 32) or 1
    out = bytearray(n)
    for i in range(n):
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        out[i] = (x >> 16) & 255
    return bytes(out)


# ================================================================================================================
# plain compressors built on the assembler: arbitrary bytes as stored / fixed / dynamic blocks (container tests)
# ================================================================================================================
def _tokens_lz(data, start, end, hist=32768, with_matches=True):
    """greedy LZ77 over data[start:end] (matches may reach back before `start`): ("lit", b) | ("match", len, dist)"""
    last = {}
    for i in range(max(0, start - hist), start):
        last[data[i:i + 3]] = i
    i = start
    out = []
    while i < end:
        key = data[i:i + 3]
        j = last.get(key) if with_matches and i + 3 <= end else None
        if j is not None and i - j <= hist:
            n = 3
            while n < 258 and i + n < end and data[j + n] == data[i + n]:
                n += 1
            out.append(("match", n, i - j))
            for k in range(i, i + n):
                last[data[k:k + 3]] = k
            i += n
        else:
            out.append(("lit", data[i]))
            last[key] = i
            i += 1
    return out


def _emit(d, toks):
    for t in toks:
        if t[0] == "lit":
            d.lit(t[1])
        else:
            d.match(t[1], t[2])
    d.eob()


def spine_lengths(freq_order, n):
    """A complete set of n code lengths whose longest codes have 15 bits: a spine of lengths 1, 2, .. s for the s symbols that
    come first in freq_order, the rest in a subtree below it."""
    for s in range(14, 0, -1):
        rest = complete_lengths(n - s) if n - s >= 2 else None
        if rest and s + max(rest) == 15:
            lens = [0] * n
            order = list(freq_order) + [i for i in range(n) if i not in set(freq_order)]
            for k, symb in enumerate(order[:s]):
                lens[symb] = k + 1
            for symb, r in zip(order[s:], rest):
                lens[symb] = s + r
            return lens
    raise ValueError(n)


def add_block(d, data, start, end, how, final=False):
    """data[start:end] as one block of the given kind appended to d (the history before `start` is what d holds already)"""
    piece = data[start:end]
    if how == "stored":
        d.stored(piece, final)
        return
    if how == "fixed":
        d.fixed(final)
        _emit(d, _tokens_lz(data, start, end))
    elif how == "dyn_literals":                    # an empty distance set: HDIST = 0, the one length 0
        used = sorted(set(piece) | {256})
        while len(used) < 2:
            used.append(255 if 255 not in used else 254)
        ll = dict(zip(used, complete_lengths(len(used))))
        d.dynamic(ll, [0], final)
        _emit(d, [("lit", b) for b in piece])
    elif how == "dyn15":                           # every one of 286 + 30 symbols has a code; the longest have 15 bits
        toks = _tokens_lz(data, start, end)
        freq = {}
        for b in piece:
            freq[b] = freq.get(b, 0) + 1
        order = sorted(freq, key=lambda b: (-freq[b], b))
        d.dynamic(spine_lengths(order + [256], 286), spine_lengths([0, 1, 2, 3], 30), final)
        _emit(d, toks)
    else:
        raise ValueError(how)


def compress(data, how, phase_blocks=0):
    """A whole zlib stream of `data`.  how: "stored", "fixed", "dyn_literals", "dyn15", "mixed", or a list of block kinds
    (the data is cut into as many pieces).  phase_blocks: that many empty dynamic blocks (an odd number of bits each) in front of the last
    block, which move the bit position at which it ends.  Returns (stream, bit phase at which the last block ends)."""
    d = Deflate()
    kinds = ["stored", "fixed", "dyn_literals", "dyn15", "fixed"] if how == "mixed" else [how] if isinstance(how, str) else list(how)
    n = len(data)
    for k, kind in enumerate(kinds):
        if how == "mixed" and k == 2:
            d.stored(b"")                          # an empty stored block in between
        if k == len(kinds) - 1:
            for _ in range(phase_blocks):
                a = d.w.bitpos
                d.dynamic({256: 1}, [0], tokens=[(18, 127), (18, 107), (1, 0), (0, 0)])
                d.eob()
                assert (d.w.bitpos - a) & 1        # an odd size: 0..7 of them reach every bit phase
        add_block(d, data, n * k // len(kinds), n * (k + 1) // len(kinds), kind, final=k == len(kinds) - 1)
    assert d.model() == bytes(data)
    return zlib_wrap(d.raw(), data), d.w.bitpos % 8


# ================================================================================================================
# the catalogue
# ================================================================================================================
MATCH_STARTS = {}          # name of a valid entry -> output position of each of its matches (filled by cases())


def _valid(name, d, **kw):
    MATCH_STARTS["valid/" + name] = starts = []
    return Case("valid/" + name, _wrap(d, **kw), d.model(starts=starts), "valid")


def _reject(name, d, msg, **kw):
    assert msg in MESSAGES
    if not isinstance(d, (bytes, bytearray)):
        kw.setdefault("adler", "none")
        d = zlib_wrap(d.raw() + bytes(8), **kw)        # real bits behind: the stream does not merely end
    return Case("reject/" + name, bytes(d), msg, "reject")


ALL_LENGTHS = list(range(1, 16)) + [15]            # a complete set with every length 1..15 in it


def _all_lengths_block(d, n_lits, final=True):
    """lit/len codes of every length 1..15 (a 10-bit code -- the last one the LL_BITS = 10 first-level table holds -- next to
    an 11-bit one that takes the canonical walk) and distance codes of every length 1..15 (D_BITS = 9: a 9-bit code in the
    table, the 10-bit one behind it); every code is used"""
    ll_syms = list(range(65, 75)) + [256, 257, 258, 264, 265, 285]             # lengths 1..10 | 11 | 12, 13, 14, 15, 15
    ll = dict(zip(ll_syms, ALL_LENGTHS))
    d.dynamic(ll, ALL_LENGTHS, final)
    for i in range(n_lits):
        d.lit(65 + (i * 7 + i // 10) % 10)
    lsyms = [257, 258, 264, 265, 285]
    for ds in range(16):                                                        # distance symbols 0..15: up to 193 + 63 back
        s = lsyms[ds % 5]
        d.length(s, (1 << LEXT[s - 257]) - 1 if ds & 1 else 0)
        d.dist(ds, ((1 << DEXT[ds]) - 1) if ds % 3 == 0 else 0)
        d.lit(65 + ds % 10)
    d.eob()


def _valid_cases():
    out = []
    d = Deflate()
    _all_lengths_block(d, 300)
    out.append(_valid("every_code_length_1_to_15", d))

    # the largest legal header: 286 lit/len symbols (226 of 8 bits, 60 of 9), 30 distance symbols (2 of 4 bits, 28 of 5); every
    # symbol once (the one match more that 30 distance symbols need takes 257 again).  32,768 stored bytes make all distances legal.
    d = Deflate()
    d.stored(noise(32768, 2))
    d.dynamic([8] * 226 + [9] * 60, [4] * 2 + [5] * 28, final=True)
    for b in range(256):
        d.lit(b)
    for i in range(30):
        d.length(257 + i % 29, 0)
        d.dist(i, 0)
    d.eob()
    out.append(_valid("largest_header_286_30", d))

    # every length symbol 257..285, extra bits all zero and all one (284 + 31 = 258 is legal)
    d = Deflate()
    d.fixed(final=True)
    d.lit(120)
    d.lit(121)
    for s in range(257, 286):
        for e in {0, (1 << LEXT[s - 257]) - 1}:
            d.length(s, e)
            d.dist(1 if s & 1 else 0, 0)
    d.eob()
    out.append(_valid("every_length_symbol", d))

    # every distance symbol 0..29, extra bits all zero and all one, behind 32,768 stored bytes (24577 + 8191 = 32768)
    d = Deflate()
    d.stored(noise(32768, 3))
    d.fixed(final=True)
    for s in range(30):
        for e in sorted({0, (1 << DEXT[s]) - 1}):
            d.length(257 + s % 8, 0)
            d.dist(s, e)
    d.eob()
    out.append(_valid("every_distance_symbol", d))

    # overlapping matches around the 64 lanes that copy a piece: distance 1, 2, 3, 31, 32, 33, 63, 64, 65
    d = Deflate()
    d.fixed(final=True)
    for b in noise(70, 4):
        d.lit(b)
    for dist in (1, 2, 3, 31, 32, 33, 63, 64, 65):
        for n in (3, 63, 64, 65, 258):
            d.match(n, dist)
            d.lit((dist * 5 + n) & 255)
    d.eob()
    out.append(_valid("overlapping_matches", d))

    # both sides of the read-back from HBM (window 2,048: `dist + 64 > 2048` reads the output instead of LDS)
    d = Deflate()
    d.stored(noise(32768, 5))
    d.fixed(final=True)
    for dist in (1984, 1985, 2047, 2048, 2049, 32768):
        for n in (3, 70, 258):
            d.match(n, dist)
            d.lit(dist & 255)
    d.eob()
    out.append(_valid("hbm_readback_distances", d))

    # matches around the FLUSH = 1024 boundary of the window: beginning 1, 2 and 258 bytes in front of it, and across it
    for k in (1, 2, 258, 100):
        d = Deflate()
        d.fixed(final=True)
        for b in noise(1024 - k, 6 + k):
            d.lit(b)
        d.match(258, 37)
        for b in noise(40, 7):
            d.lit(b)
        d.match(200, 1000)
        d.match(258, 1)
        d.eob()
        out.append(_valid("match_%d_before_flush_1024" % k, d))

    # ---- the accepted oddities ----
    d = Deflate()
    d.dynamic({97: 1, 256: 2, 257: 2}, {0: 1}, final=True)          # one distance code of one bit (incomplete, allowed), used
    d.lit(97)
    d.length(257)
    d.dist(0)
    d.eob()
    out.append(_valid("one_code_distance_set_used", d))
    d = Deflate()
    d.dynamic({97: 1, 98: 2, 256: 2}, [0], final=True)              # empty distance set, literals only
    for b in b"abba":
        d.lit(b)
    d.eob()
    out.append(_valid("empty_distance_set_literals_only", d))
    d = Deflate()
    d.dynamic({256: 1}, [0], final=True)                            # the lit/len set is the single one-bit code 256
    d.eob()
    out.append(_valid("litlen_set_is_only_256", d))
    d = Deflate()
    # a repeat that runs from the lit/len lengths into the distance lengths: 2, then 16 x 5 = 256 | 257 | four distance codes
    ll, dd = {97: 1, 256: 2, 257: 2}, [2, 2, 2, 2]
    toks = [(18, 86), (1, 0), (18, 127), (18, 9), (2, 0), (16, 2)]
    _check_tokens(ll, dd, toks)
    d.dynamic(ll, dd, final=True, tokens=toks)
    for _ in range(4):
        d.lit(97)
    d.length(257)
    d.dist(3)
    d.length(257)
    d.dist(0)
    d.eob()
    out.append(_valid("repeat_runs_from_litlen_into_distance_lengths", d))
    d = Deflate()
    # a 16 that repeats the zero a 17 / an 18 set: 17, 16, 18, 16 spell 3 + 3 + 88 + 3 zeros; 18, 18, 16, 17 spell 138 + 11 + 6 + 3
    ll, dd = {97: 1, 256: 2, 257: 2}, {0: 1}
    toks = [(17, 0), (16, 0), (18, 77), (16, 0), (1, 0), (18, 127), (18, 0), (16, 3), (17, 0), (2, 0), (2, 0), (1, 0)]
    _check_tokens(ll, dd, toks)
    d.dynamic(ll, dd, final=True, tokens=toks)
    d.lit(97)
    d.length(257)
    d.dist(0)
    d.eob()
    out.append(_valid("repeat_16_of_a_zero_from_17_18", d))
    d = Deflate()
    for i in range(40):                                             # many empty stored and empty fixed blocks in a row
        d.stored(b"")
        d.fixed()
        d.eob()
    d.fixed(final=True)
    d.lit(33)
    d.eob()
    out.append(_valid("many_empty_stored_and_fixed_blocks", d))
    d = Deflate()
    d.stored(b"")                                                   # stored lengths 0 and 65535
    d.stored(noise(65535, 9), final=True)
    out.append(_valid("stored_0_and_65535", d))
    d = Deflate()
    d.fixed(final=True)                                             # a header that declares a 256-byte window (CINFO = 0) and a
    for b in noise(300, 12):                                        # match from further back: zlib does not hold the data to it
        d.lit(b)
    d.match(20, 300)
    d.eob()
    out.append(_valid("declared_window_256_distance_300", d, cmf=0x08))

    # input of more than 1,100 bytes whose codes straddle the refills of the 512-byte LDS copy (IN_WORDS = 128 dwords): 9-bit
    # literals and codes with extra bits at every bit phase; then the every-length codes (15-bit codes across the refills)
    d = Deflate()
    d.fixed()
    for i, b in enumerate(noise(900, 10)):
        d.lit(144 + b % 112)
        if i % 9 == 8 and i > 320:                                  # (distances up to 193 + 7 back)
            d.length(281 + i % 4, i % 32)
            d.dist(8 + i % 8, i % 8)
    d.eob()
    _all_lengths_block(d, 1500)
    assert len(d.raw()) >= 1100 + 512
    out.append(_valid("input_across_512_byte_refills", d))
    return out


def _check_tokens(ll, dd, toks):
    """what the run-length tokens spell equals the tables they go with (the hand-written token lists above)"""
    got = []
    for s, e in toks:
        if s < 16:
            got.append(s)
        elif s == 16:
            got += [got[-1]] * (3 + e)
        elif s == 17:
            got += [0] * (3 + e)
        else:
            got += [0] * (11 + e)
    assert got == _table(ll, 257) + _table(dd, 1), (len(got), got[-12:])


def _dyn_reject(name, msg, ll=None, dd=None, **kw):
    """a dynamic block header (lit/len 97: 1 bit, 256 and 257: 2 bits; two one-bit distance codes -- 258 + 2 lengths -- unless
    given) with one thing wrong"""
    d = Deflate()
    d.dynamic({97: 1, 256: 2, 257: 2} if ll is None else ll, {0: 1, 1: 1} if dd is None else dd, final=True, **kw)
    return _reject(name, d, msg)


def _reject_cases():
    out = []
    good = Deflate()
    good.fixed(final=True)
    for b in b"hello, hello":
        good.lit(b)
    good.eob()
    body = good.raw()
    text = good.model()
    out.append(_reject("header_check", zlib_wrap(body, text, flg=0x9D), "incorrect header check"))
    out.append(_reject("method_9", zlib_wrap(body, text, cmf=0x79), "unknown compression method"))
    out.append(_reject("window_bits_16", zlib_wrap(body, text, cmf=0x88), "invalid window size"))
    out.append(_reject("adler_wrong", zlib_wrap(body, text, adler="bad"), "incorrect data check"))
    d = Deflate()
    d.block_type(3, final=True)
    out.append(_reject("block_type_3", d, "invalid block type"))
    d = Deflate()
    d.fixed()
    d.lit(1)
    d.eob()
    d.block_type(3)
    out.append(_reject("block_type_3_behind_a_block", d, "invalid block type"))
    for name, n, nl in (("nlen_off_by_one", 5, 5 ^ 0xFFFE), ("len_equals_nlen", 0, 0), ("len_65535_nlen_65535", 65535, 65535)):
        d = Deflate()
        d.stored(b"hello", final=True, len_=n, nlen=nl)
        out.append(_reject("stored_" + name, d, "invalid stored block lengths"))
    # HLIT 30, 31 (287, 288 lit/len codes), HDIST 30, 31 (31, 32 distance codes)
    for name, kw in (("hlit_30", {"hlit": 30}), ("hlit_31", {"hlit": 31}), ("hdist_30", {"hdist": 30}), ("hdist_31", {"hdist": 31})):
        out.append(_dyn_reject(name, "too many length or distance symbols", **kw))
    out.append(_dyn_reject("cl_oversubscribed", "invalid code lengths set", cl_lens={0: 1, 1: 1, 2: 1}))
    out.append(_dyn_reject("cl_incomplete_two_codes", "invalid code lengths set", cl_lens={0: 2, 1: 2}, tokens=[(0, 0)] * 260))
    out.append(_dyn_reject("cl_incomplete_one_code", "invalid code lengths set", cl_lens={0: 1}, tokens=[(0, 0)] * 260))
    # repeat codes: a 16 with nothing before it; a 16, a 17, an 18 that each run one past nlen + ndist = 258 + 2
    out.append(_dyn_reject("repeat_16_first", "invalid bit length repeat", tokens=[(16, 0)] + [(1, 0)] * 257))
    head = [(0, 0)] * 97 + [(1, 0), (18, 127), (18, 9), (2, 0), (2, 0)]             # the 258 lit/len lengths
    _check_tokens({97: 1, 256: 2, 257: 2}, {0: 1, 1: 1}, head + [(1, 0), (1, 0)])
    out.append(_dyn_reject("repeat_16_one_past_the_end", "invalid bit length repeat", tokens=head + [(16, 0)]))           # 258 + 3
    out.append(_dyn_reject("repeat_17_one_past_the_end", "invalid bit length repeat", tokens=head + [(17, 0)]))           # 258 + 3
    out.append(_dyn_reject("repeat_18_one_past_the_end", "invalid bit length repeat",
                           tokens=[(0, 0)] * 97 + [(1, 0), (18, 127), (18, 14)]))                                         # 98 + 138 + 25
    out.append(_dyn_reject("no_end_of_block_code", "invalid code -- missing end-of-block", ll={97: 1, 98: 1}))
    for what, msg in (("ll", "invalid literal/lengths set"), ("dd", "invalid distances set")):
        for name, lens in (("oversubscribed", (1, 1, 1)), ("incomplete_two_codes", (2, 2)), ("single_code_of_length_2", (2,))):
            if what == "ll":
                ll = dict(zip((256, 97, 98), lens))
                out.append(_dyn_reject("litlen_" + name, msg, ll=ll, dd={0: 1}))
            else:
                d = Deflate()
                d.dynamic({97: 1, 256: 2, 257: 2}, dict(zip((0, 1, 2), lens)), final=True)
                out.append(_reject("distances_" + name, d, msg))
    for s in (286, 287):
        d = Deflate()
        d.fixed(final=True)
        d.lit(7)
        d.sym(s)
        out.append(_reject("fixed_litlen_%d" % s, d, "invalid literal/length code"))
    for s in (30, 31):
        d = Deflate()
        d.fixed(final=True)
        d.lit(7)
        d.length(257)
        d.dist(s)
        out.append(_reject("fixed_distance_%d" % s, d, "invalid distance code"))
    d = Deflate()
    d.dynamic({97: 1, 256: 2, 257: 2}, {0: 1}, final=True)
    d.lit(97)
    d.length(257)
    d.w.bits(1, 1)                                                  # the one code is `0`: this is the bit pattern without a code
    out.append(_reject("one_code_distance_set_unused_bit", d, "invalid distance code"))
    for bit in (0, 1):
        d = Deflate()
        d.dynamic({97: 1, 256: 2, 257: 2}, [0], final=True)
        d.lit(97)
        d.length(257)
        d.w.bits(bit, 1)                                            # an empty set and a real bit behind the length
        d.w.bits(0x7F, 7)
        out.append(_reject("empty_distance_set_real_bit_%d" % bit, d, "invalid distance code"))
    d = Deflate()
    d.fixed(final=True)
    d.length(257)
    d.dist(0)
    out.append(_reject("too_far_back_at_position_0", d, "invalid distance too far back"))
    d = Deflate()
    d.fixed(final=True)
    d.lit(97)
    d.length(257)
    d.dist(1)
    out.append(_reject("too_far_back_at_position_1", d, "invalid distance too far back"))
    d = Deflate()
    d.stored(b"0123456789")
    d.fixed(final=True)
    d.length(258)
    d.dist(6, 2)                                                    # 9 + 2 = 11 back, ten bytes there
    out.append(_reject("too_far_back_behind_a_stored_block", d, "invalid distance too far back"))
    return out


# where the "too far back" match stands in the output (tests: the match arriving exactly when the room is used up is no error)
TOO_FAR_BACK_AT = {"reject/too_far_back_at_position_0": 0, "reject/too_far_back_at_position_1": 1,
                   "reject/too_far_back_behind_a_stored_block": 10}


def _shift(d, k):
    """k one-bit literals in a block of their own: everything behind stands k bits further on"""
    d.dynamic({97: 1, 256: 2, 257: 2}, [0])
    for _ in range(k):
        d.lit(97)
    d.eob()


def _field_bodies():
    """field kind -> function(d) that writes a block containing the field and returns (first bit, bit behind the last)"""
    plain = dict(ll_lens={97: 1, 256: 2, 257: 2}, d_lens={0: 1, 1: 1})

    def block_header(d):
        d.fixed(final=True)
        d.eob()
        return d.marks["hdr"], d.marks["hdr"] + 3

    def header_14_bits(d):
        d.dynamic(final=True, **plain)
        return d.marks["counts"], d.marks["counts"] + 14

    def cl_length(d):
        d.dynamic(final=True, **plain)
        return d.marks["cl"][5], d.marks["cl"][5] + 3

    def length_token(d):
        d.dynamic(final=True, **plain)
        return d.marks["tok"][97], d.marks["tokx"][97]

    def repeat_extra(sym):
        def body(d):
            toks = {16: [(0, 0)] * 97 + [(1, 0)] + [(0, 0), (16, 3)] + [(18, 127), (18, 2)] + [(2, 0), (2, 0), (1, 0), (1, 0)],
                    17: [(0, 0)] * 97 + [(1, 0)] + [(17, 4)] + [(18, 127), (18, 2)] + [(2, 0), (2, 0), (1, 0), (1, 0)],
                    18: [(0, 0)] * 97 + [(1, 0)] + [(18, 127), (18, 9)] + [(2, 0), (2, 0), (1, 0), (1, 0)]}[sym]
            _check_tokens(plain["ll_lens"], plain["d_lens"], toks)
            d.dynamic(final=True, tokens=toks, **plain)
            i = [t[0] for t in toks].index(sym)
            return d.marks["tokx"][i], d.marks["tok"][i + 1]
        return body

    def litlen_code(d):
        d.fixed(final=True)
        d.lit(66)
        a = d.w.bitpos
        d.lit(200)                                                  # nine bits
        return a, d.w.bitpos

    def length_extra(d):
        d.fixed(final=True)
        d.lit(66)
        d.sym(284)
        a = d.w.bitpos
        d.w.bits(17, 5)
        return a, d.w.bitpos

    def distance_code(full):
        def body(d):
            if full == "full":
                d.fixed(final=True)
            else:
                d.dynamic({97: 1, 256: 2, 257: 2}, {0: 1} if full == "one" else [0], final=True)
            d.lit(97)
            d.length(257)                                           # no extra bits: its last bit is the last bit in front of the field
            a = d.w.bitpos
            if full == "full":
                d.dist(0)
                return a, d.w.bitpos
            return a, a + 1                                         # zlib asks for one bit before it looks at either table
        return body

    def distance_extra(d):
        d.fixed(final=True)
        d.lit(66)
        d.length(257)
        d.w.code(*d.dd[29])
        a = d.w.bitpos
        d.w.bits(5000, 13)
        return a, d.w.bitpos

    def stored_lengths(d):
        d.stored(b"stored", final=True)
        return d.marks["len"], d.marks["data"]

    def stored_bytes(d):
        d.stored(b"stored bytes", final=True)
        return d.marks["data"], d.w.bitpos

    def adler(d):
        d.fixed(final=True)
        d.lit(66)
        d.eob()
        a = (d.w.bitpos + 7) // 8 * 8
        return a, a + 32

    return [("block_header", block_header), ("header_14_bits", header_14_bits), ("code_length_code_length", cl_length),
            ("length_token", length_token), ("extra_bits_of_16", repeat_extra(16)), ("extra_bits_of_17", repeat_extra(17)),
            ("extra_bits_of_18", repeat_extra(18)), ("litlen_code", litlen_code), ("length_extra_bits", length_extra),
            ("distance_code_full_set", distance_code("full")), ("distance_code_one_code_set", distance_code("one")),
            ("distance_code_empty_set", distance_code("empty")), ("distance_extra_bits", distance_extra),
            ("stored_len_nlen", stored_lengths), ("stored_bytes", stored_bytes), ("adler_bytes", adler)]


FIELD_KINDS = tuple(k for k, _ in _field_bodies())


ENDS_EXACTLY_IN_FRONT = set()      # the ended-inside entries whose last bit is the last bit of the field in front (filled by cases())


def _ended_cases():
    """For every field kind and every bit phase (0..7 one-bit literals in front): the stream cut at every byte boundary from
    the end of the field in front (where that is a byte boundary) to the last one before the field is complete.  zlib waits
    for input there: it hands out what is complete and reports nothing."""
    out = []
    for kind, body in _field_bodies():
        exact = 0
        for k in range(8):
            d = Deflate()
            _shift(d, k)
            a, b = body(d)
            raw = d.raw() + (adler32(d.model()).to_bytes(4, "big") if kind == "adler_bytes" else b"")
            last = (b - 1) // 8
            for cut in range(min((a + 7) // 8, last), last + 1):
                if cut * 8 == a:
                    exact += 1
                    ENDS_EXACTLY_IN_FRONT.add("ended/%s/phase%d/cut%d" % (kind, k, cut))
                out.append(Case("ended/%s/phase%d/cut%d" % (kind, k, cut), zlib_wrap(raw[:cut], adler="none"), d.model(cut * 8), "ended"))
        assert exact >= 1, kind                                      # at least one phase ends exactly behind the field in front
    return out


def cases():
    """The catalogue: a list of Case(name, stream, expect, kind)."""
    out = _valid_cases() + _reject_cases() + _ended_cases()
    # a header that asks for a preset dictionary: accepted as far as it goes (zlib: Z_NEED_DICT; Inflater: 0 bytes, needsDictionary())
    d = Deflate()
    d.fixed(final=True)
    d.lit(66)
    d.eob()
    out.append(Case("valid/preset_dictionary_header", _wrap(d, dictid=0x12345678), b"", "needdict"))
    assert len({c.name for c in out}) == len(out)
    return out
