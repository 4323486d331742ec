"""Seeded damage of CodecHuffman, CodecCanonHuffman and CodecDeflate packings (CPU only).

Every generator is deterministic in its arguments and returns (label, packing) pairs; the label names the damage so that a failing
tile says what was done to it.  The kinds:

- header:  predictor byte, seed bytes, the nM32 field (CodecHuffman: bytes 6..9; canonical packings get the same byte positions,
           which there hold the start of the code-length table)
- tree:    every bit from bit 80 to 8 bits past the end of the serialised Huffman tree; for canonical packings every bit of the
           code-length tables (bit 48 to their end)
- text:    bits at a fixed odd stride over the text, every bit of the last 8 bytes, bursts of 8 random bytes
- length:  truncations (len-16 .. len-1, len/2, the end of the tree +-2 bytes) and extensions by 1 and 64 random bytes
- crafted: the oracle's own M32 stream of a good tile, altered, and re-encoded into a valid packing (Huffman text with a
           corrected nM32 field, or zlib for CodecDeflate): well-formed text that reaches the value stage

deviation() is the exact predicate for the inputs DESIGN.md 2 lists as documented deviations (no encoder writes them; the device
reports an error whatever the oracle does): nM32 > 6 * cells and Huffman trees deeper than 63."""
import zlib

import numpy as np

import oracle

HUFFMAN, CANON, DEFLATE = "huffman", "canon", "deflate"
MAX_DEPTH = 63                                   # gvrs_decode.hip: code length limit of the tree parser


def _bit(pk, i):
    return (pk[i >> 3] >> (i & 7)) & 1 if i < len(pk) * 8 else 0


def huffman_tree_walk(pk, bit0=80):
    """(end bit, deepest leaf) of the serialised tree at bit0, walked as HuffmanDecoder.decodeTree :87-120 walks it: the tree
    ends when its leaf count is reached (or the bits run out, or a leaf closes the root before the count)"""
    nbits = len(pk) * 8
    n_leaves = sum(_bit(pk, bit0 + k) << k for k in range(8)) + 1
    p = bit0 + 8
    if _bit(pk, p):
        return p + 9, 0                          # single-symbol form
    p += 1
    stack = [[0, 0]]                             # [depth, children placed] of the open branch nodes
    leaves = deepest = 0
    while leaves < n_leaves and stack and p < nbits:
        top = stack[-1]
        top[1] += 1
        d = top[0] + 1
        if _bit(pk, p):
            p += 9
            leaves += 1
            deepest = max(deepest, d)
            while stack and stack[-1][1] == 2:
                stack.pop()
        else:
            p += 1
            stack.append([d, 0])
    return min(p, nbits), deepest


def canon_table_end(pk):
    """bit position behind CodecCanonHuffman's code-length tables (CanonicalHuffman.decode :441-463), or None where they
    cannot be read"""
    from oracle import canon_ref as cr
    try:
        inp = cr.BitInputStore(pk, 6, len(pk) - 6)
        inp.getBit()
        meta = [0] * (cr.SYMBOL_SET_SIZE + 1)
        cr.LengthEncoder.readEncodedLengths(inp, cr.SYMBOL_SET_SIZE + 1, meta)
        lengths = [0] * (cr.N_SYMBOLS_TOTAL + 1 + 140)
        cr.CanonHuffTreeDecoder(meta).decodeTree(inp, cr.N_SYMBOLS_TOTAL, lengths)
        return 48 + inp.getPosition()
    except (IndexError, ValueError):
        return None


def text_start(pk, kind):
    return canon_table_end(pk) if kind == CANON else huffman_tree_walk(pk)[0]


def n_m32(pk):
    return int.from_bytes(pk[6:10], "little") if len(pk) >= 10 else None


def deviation(pk, kind, cells):
    """the documented deviation this packing falls under (a label), or None"""
    if kind == CANON or len(pk) < 10:
        return None
    if n_m32(pk) > 6 * cells:
        return "nM32 > 6*cells"
    if kind == HUFFMAN and 1 <= pk[1] <= 4 and huffman_tree_walk(pk)[1] > MAX_DEPTH:
        return "tree deeper than 63"
    return None


def oracle_decode(kind, r, c, pk):
    """the oracle's cells, or None where the reference throws"""
    f = {HUFFMAN: oracle.codec_huffman_decode, CANON: oracle.codec_canon_decode, DEFLATE: oracle.codec_deflate_decode}[kind]
    try:
        return f(r, c, pk)
    except (IOError, ValueError):
        return None


def _flip(pk, i):
    x = bytearray(pk)
    x[i >> 3] ^= 1 << (i & 7)
    return bytes(x)


def _put(pk, at, data):
    x = bytearray(pk)
    x[at:at + len(data)] = data
    return bytes(x)


def header_damage(pk, kind, cells):
    out = []
    for v in (0, 1, 2, 3, 4, 5, 255) + ((0x7f, 0x80) if kind == CANON else ()):
        if v != pk[1]:
            out.append(("predictor=%d" % v, _put(pk, 1, bytes([v]))))
    for v in (0x7fffffff, 0x80000000, 0xffffffff, 0):
        out.append(("seed=%#x" % v, _put(pk, 2, v.to_bytes(4, "little"))))
    n_stream = cells - 1
    orig = n_m32(pk)
    for v in sorted({n_stream - 1, n_stream, orig - 1, orig + 1, 6 * cells, 6 * cells + 1, 2 ** 31 - 1, 2 ** 31}):
        if v != orig and v >= 0:
            out.append(("nM32=%d" % v, _put(pk, 6, v.to_bytes(4, "little"))))
    return out


def tree_damage(pk, kind):
    if kind == CANON:
        end = canon_table_end(pk)
        return [("table bit %d" % i, _flip(pk, i)) for i in range(48, end)]
    end = min(huffman_tree_walk(pk)[0] + 8, len(pk) * 8)
    return [("tree bit %d" % i, _flip(pk, i)) for i in range(80, end)]


def text_damage(pk, kind, rng, n_stride=600, n_bursts=10):
    out = []
    t0, nb = text_start(pk, kind), len(pk) * 8
    stride = max(1, (nb - t0) // n_stride) | 1
    out += [("text bit %d" % i, _flip(pk, i)) for i in range(t0 + stride // 2, nb - 64, stride)]
    out += [("tail bit %d" % i, _flip(pk, i)) for i in range(max(t0, nb - 64), nb)]
    for _ in range(n_bursts):
        a = int(rng.integers((t0 + 7) // 8, max((t0 + 7) // 8 + 1, len(pk) - 8)))
        out.append(("burst at %d" % a, _put(pk, a, bytes(rng.integers(0, 256, 8, dtype=np.uint8)))))
    return out


def length_damage(pk, kind, rng):
    n = len(pk)
    te = (text_start(pk, kind) + 7) // 8
    cuts = sorted({k for k in list(range(n - 16, n)) + [n // 2, te - 2, te - 1, te, te + 1, te + 2] if 0 < k < n})
    out = [("truncated to %d" % k, pk[:k]) for k in cuts]
    out.append(("extended by 1", pk + bytes(rng.integers(0, 256, 1, dtype=np.uint8))))
    out.append(("extended by 64", pk + bytes(rng.integers(0, 256, 64, dtype=np.uint8))))
    return out


def damage_set(pk, kind, r, c, seed, parts=("header", "tree", "text", "length")):
    """the damage of one good packing, in a fixed order"""
    rng = np.random.default_rng(seed)
    out = []
    for part in parts:
        if part == "header":
            out += header_damage(pk, kind, r * c)
        elif part == "tree":
            out += tree_damage(pk, kind)
        elif part == "text":
            out += text_damage(pk, kind, rng)
        elif part == "length":
            out += length_damage(pk, kind, rng)
    return out


# ---------------------------------------------------------------- crafted M32 streams


def _values(m32):
    """the M32 stream cut into its values (byte ranges), as CodecM32.decode reads them"""
    out, p, n = [], 0, len(m32)
    while p < n:
        q = p + 1
        if m32[p] in (0x7f, 0x81):
            while q < n and q - p < 6 and m32[q] & 0x80:
                q += 1
            q += 1
        out.append((p, min(q, n)))
        p = q
    return out


def m32_alterations(m32, model, n_cols, rng):
    """(label, altered M32 stream) pairs of one good stream"""
    m = bytes(m32)
    vals = _values(m)
    out = [("last byte dropped", m[:-1])]
    a, _ = vals[-1]
    out.append(("trailing 0x7f", m[:a] + b"\x7f"))
    out.append(("trailing 0x81", m[:a] + b"\x81"))
    out.append(("0x7f appended", m + b"\x7f"))
    if model in (1, 2, 3):
        k = len(vals) // 2
        out.append(("null code 0x80", m[:vals[k][0]] + b"\x80" + m[vals[k][1]:]))
    # six-byte values whose sum with the prior wraps an int32 (CodecM32: 0x7f/0x81 and five continuation bytes)
    big = oracle.m32_encode(2 ** 31 - 1)
    out.append(("6-byte value inserted", m[:vals[3][0]] + big + m[vals[3][0]:]))
    out.append(("6-byte pair wraps", m[:vals[5][0]] + big + big + m[vals[6][1]:]))
    out.append(("extra bytes behind", m + bytes(rng.integers(0, 127, 5, dtype=np.uint8))))
    # a run of 3-byte values (0x7f + 2 continuation-form bytes) long enough to leave a 64-byte window with no value start
    run = oracle.m32_encode(300) * 40
    out.append(("3-byte run", m[:vals[10][0]] + run + m[vals[10 + 40][0]:] if len(vals) > 60 else m + run))
    if model == 4:
        out.append(("null at row start", m[:vals[n_cols][0]] + b"\x80" + m[vals[n_cols][1]:]))
        out.append(("null after a sum", m[:vals[n_cols + 1][0]] + b"\x80" + m[vals[n_cols + 1][1]:]))
    return out


def crafted_m32(kind, r, c, values, seed):
    """packings whose M32 stream is the oracle's stream of `values` (the model the oracle's encoder chooses), altered; CodecHuffman
    packings are Huffman-coded behind a header with the stream's length, CodecDeflate ones zlib-compressed"""
    rng = np.random.default_rng(seed)
    if kind == HUFFMAN:
        good, model = oracle.codec_huffman_encode(0, r, c, values)
    else:
        good, model = oracle.codec_deflate_encode(0, r, c, values)
    m32, s = oracle.predictor_encode(model, r, c, values)
    assert s == int.from_bytes(good[2:6], "little", signed=True)
    out = []
    for label, m in [("unaltered", m32)] + m32_alterations(m32, model, c, rng):
        hdr = good[:6] + len(m).to_bytes(4, "little")
        if kind == HUFFMAN:
            pk = oracle.huffman_encode(np.frombuffer(m, np.uint8), 80, hdr)[0]
        else:
            pk = hdr + zlib.compress(m, 6)
        out.append(("crafted: " + label, pk))
    return good, out


def outcome(kind, r, c, pk, good_cells):
    """'throws', 'same' (decodes to the original cells) or 'changed <n>' (decodes, n cells differ)"""
    got = oracle_decode(kind, r, c, pk)
    if got is None:
        return "throws"
    d = int(np.count_nonzero(got != good_cells))
    return "same" if d == 0 else "changed %d" % d
