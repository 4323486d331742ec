"""CodecCanonHuffman.analyze restated for the tests (compress/canonicalHuffman/CodecCanonHuffman.java:217-271,
CanonHuffmanStats.java, CanonicalHuffman.countSymbols :352-418, getEntropy :709-751, getEscapeBitCountTotal :656-662).

The text comes from the C oracle's canonical decoder, the bits in the code tables from the pure-Python restatement
(oracle.canon_ref: the tables alone, not the text), the counts from numpy -- index expressions as in countSymbols, quirks
included: the single 2-bit escape counts count2bit[(s >> 2) & 3], values in [-8388608, -8333609] count as 16-bit escapes,
the 6-bit class is left out of the escape-bit total, the predictor byte is used as an index only after the escape table
was added to, a byte of 5 lands on "All Predictors" twice."""
import math

import numpy as np

import oracle
from oracle import canon_ref as R

NULL = -2 ** 31
FIELDS = ("n_tiles", "n_bytes", "n_symbols", "n_bits_overhead", "n_text_counted", "sum_length", "sum_observed", "sum_escape_bits")


def bits_in_code_table(packing):
    """CanonicalHuffman.getBitsInCodeTableCount after decode: the reader's position behind the code tables, from byte 6."""
    inp = R.BitInputStore(packing, 6, len(packing) - 6)
    inp.getBit()                                                    # the reserved bit
    code_lengths = [0] * (R.SYMBOL_SET_SIZE + 1)
    R.LengthEncoder.readEncodedLengths(inp, R.SYMBOL_SET_SIZE + 1, code_lengths)
    text_lengths = [0] * (R.N_SYMBOLS_TOTAL + 1)
    R.CanonHuffTreeDecoder(code_lengths).decodeTree(inp, R.N_SYMBOLS_TOTAL, text_lengths)
    return inp.getPosition()


def count_symbols(text):
    """countSymbols over all entries: (node counts[260], count2bit[4], count8bit[256], class counts[6])."""
    r = np.asarray(text, np.int64)
    nodes = np.zeros(260, np.int64)
    c2 = np.zeros(4, np.int64)
    c8 = np.zeros(256, np.int64)
    left = np.ones(r.size, bool)

    def take(lo, hi):
        nonlocal left
        m = left & (r >= lo) & (r <= hi)
        left = left & ~m
        return r[m]

    plain = take(-128, 127)
    e2, e4, e6, e8 = take(-512, 511), take(-2048, 2047), take(-8192, 8191), take(-32768, 32767)
    nul = take(NULL, NULL)
    e16 = take(-8388608, 8388607)
    e24 = r[left]
    np.add.at(nodes, plain + 128, 1)
    for vals, shift, esc, per in ((e2, 2, 258, 1), (e4, 4, 258, 2), (e6, 6, 258, 3), (e8, 8, 257, 1), (e16, 16, 257, 2),
                                  (e24, 24, 257, 3)):
        np.add.at(nodes, (vals >> shift) + 128, 1)
        nodes[esc] += per * vals.size
    nodes[256] += nul.size
    nodes[259] = 1
    np.add.at(c2, (e2 >> 2) & 3, 1)
    for s in (2, 0):
        np.add.at(c2, (e4 >> s) & 3, 1)
    for s in (4, 2, 0):
        np.add.at(c2, (e6 >> s) & 3, 1)
    np.add.at(c8, (e8 >> 8) & 0xFF, 1)
    for s in (8, 16):
        np.add.at(c8, (e16 >> s) & 0xFF, 1)
    for s in (8, 16, 24):
        np.add.at(c8, (e24 >> s) & 0xFF, 1)
    classes = [e2.size, e4.size, e6.size, e8.size, e16.size, e24.size]
    return nodes, c2, c8, classes


def entropy(nodes, c2, c8):
    e = e2 = e8 = 0.0
    d = float(nodes.sum())
    for n in nodes:
        if n > 0:
            p = n / d
            e += p * math.log(p)
    for esc, counts, acc in ((258, c2, "e2"), (257, c8, "e8")):
        if nodes[esc] > 0:
            ne = float(nodes[esc])
            p = ne / d
            s = 0.0
            for c in counts:
                if c > 0:
                    q = c / ne
                    s += p * q * math.log(q)
            if acc == "e2":
                e2 += s
            else:
                e8 += s
    return -(e + e2 + e8) / math.log(2.0)


class Twin:
    """The six CanonHuffmanStats records (0..4 by predictor byte, 5 = all) and the escape table of one codec."""

    def __init__(self):
        self.stats = [dict.fromkeys(FIELDS, 0) for _ in range(6)]
        self.entropy = [0.0] * 6
        self.escapes = [0] * 6

    def _add(self, k, n_bytes, n, bits, observed, ent):
        s = self.stats[k]
        s["n_tiles"] += 1
        s["n_bytes"] += n_bytes
        s["n_symbols"] += n
        s["n_bits_overhead"] += bits
        s["n_text_counted"] += 1
        s["sum_length"] += n
        s["sum_observed"] += observed
        self.entropy[k] += ent

    def analyze(self, n_rows, n_cols, packing):
        """True where the reference's analyze returns, False where it throws."""
        n = n_rows * n_cols
        if len(packing) < 2:
            return False
        pred = packing[1]
        if pred == 0 and len(packing) == 6:
            self._add(0, 0, n, 0, 1, 0.0)
            self._add(5, 0, n, 0, 1, 0.0)
            return True
        if len(packing) <= 6:
            return False
        try:
            text, _ = oracle.canon_decode(packing, n, 48)
            bits = bits_in_code_table(packing)
        except (ValueError, IndexError):
            return False
        res = np.zeros(n, np.int64)
        res[:text.size] = text
        nodes, c2, c8, classes = count_symbols(res)
        for i in range(6):
            self.escapes[i] += classes[i]
        if pred >= 6:
            return False
        ent = entropy(nodes, c2, c8)
        observed = int(np.unique(res & 0xFF).size)
        esc_bits = 2 * classes[0] + 4 * classes[1] + 8 * classes[3] + 16 * classes[4] + 24 * classes[5]
        for k in (pred, 5):
            self._add(k, len(packing) - 6, n, bits, observed, ent)
        self.stats[pred]["sum_escape_bits"] += esc_bits
        self.stats[5]["sum_escape_bits"] += esc_bits
        return True


def assert_matches(got, escapes, twin):
    """got: the codec's analysis_data(), escapes: its escape_counts()."""
    import pytest
    for k in range(6):
        have = {f: int(got[k][f]) for f in FIELDS}
        assert have == twin.stats[k], (k, have, twin.stats[k])
        assert float(got[k]["sum_entropy"]) == pytest.approx(twin.entropy[k], rel=1e-12, abs=1e-12), k
    assert [int(x) for x in escapes] == twin.escapes
