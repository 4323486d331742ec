"""The numpy model of symbol tables merged and of strips accumulated onto a table (gf_tab_symbols_merge[_dev],
gf_block_tabulate_symbols_acc[_dev]), written from the Java text of the reference beside tests/tabulate_ref.py:
  the counter per symbol is a Java int that `count + 1` wraps      demo/.../entropy/EntropyTabulator.java:239-240
  the scalars are taken over the counters > 0 alone                :278-292
  a SHORT cell's symbol is its sign-extended int                   :230-235 (readValueInt)
A table is (symbols uint32 strictly ascending, counts int32, summary dict with tabulate_ref.symbols' keys).  n_symbols is the
number of entries: the library's one stated deviation from the reference, whose nSymbols counts a symbol once more when its counter
comes back to 0 after 2^32 occurrences (strips_literal below keeps the reference's number beside it)."""
import numpy as np

import tabulate_ref as R

TRUNCATED = 1                                      # GF_TAB_SYM_INPUT_TRUNCATED


def summary_of(counts, n_samples, reserved=0):
    """the summary of a whole table with these counts: the scalars over counts > 0"""
    c = np.asarray(counts, np.int32)
    pos = c[c > 0]
    return dict(n_samples=int(n_samples), n_symbols=int(c.size), n_unique=int((pos == 1).sum()), n_repeated=int((pos != 1).sum()),
                n_written=int(c.size), max_count=int(pos.max()) if pos.size else 0, reserved=int(reserved))


def table(symbols, counts, n_samples=None, **over):
    """a hand-built table; n_samples None: the sum of the counts; over: summary fields set by hand (a truncated table's n_symbols)"""
    sym, cnt = np.asarray(symbols, np.uint32).ravel(), np.asarray(counts, np.int32).ravel()
    assert sym.size == cnt.size and (sym.size < 2 or (np.diff(sym.astype(np.int64)) > 0).all())
    s = summary_of(cnt, int(cnt.sum(dtype=np.int64)) if n_samples is None else n_samples)
    s.update(over)
    return sym, cnt, s


EMPTY = table([], [])


def entries(t, cap=None):
    """the entries of a table that count: the first min(n_written, cap)"""
    n = max(0, min(int(t[2]["n_written"]), t[0].size if cap is None else min(cap, t[0].size)))
    return t[0][:n], t[1][:n], n


def merge(a, b, cap_a=None, cap_b=None):
    """the merged table, whole (not cut to any capacity): the union of the symbols in ascending unsigned order, the count of a
    symbol of both the sum with int32 wrap; entries whose count wrapped to <= 0 stay"""
    (sa, ca, na), (sb, cb, nb) = entries(a, cap_a), entries(b, cap_b)
    sym, inv = np.unique(np.concatenate([sa, sb]), return_inverse=True)
    total = np.zeros(sym.size, np.int64)
    np.add.at(total, inv, np.concatenate([ca, cb]).astype(np.int64))
    cnt = ((total + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int32)
    flag = (a[2]["reserved"] | b[2]["reserved"]) & TRUNCATED
    flag |= int(na < a[2]["n_symbols"]) | int(nb < b[2]["n_symbols"])
    return sym.astype(np.uint32), cnt, summary_of(cnt, R._wrap64(a[2]["n_samples"] + b[2]["n_samples"]), flag)


def cut(t, cap):
    """a table as a call with table_cap = cap leaves it: the first cap entries, the scalars complete"""
    n = min(cap, t[0].size)
    return t[0][:n], t[1][:n], dict(t[2], n_written=n)


def accumulate(strips, elem_type, into=None):
    """the table of the strips' cells counted one strip after another onto `into` (None: empty)"""
    t = EMPTY if into is None else into
    for strip in strips:
        v = np.ascontiguousarray(strip, R.DTYPES[elem_type]).ravel()
        if t[2]["n_samples"] == 0:
            t = EMPTY                              # an in-table without samples is empty
        t = merge(t, R.symbols(v, elem_type)) if v.size else merge(t, EMPTY)
    return t


def strips_literal(strips, elem_type, counts=None):
    """EntropyTabulator's two loops as they stand, run over the strips one after another with a dict for the 16 GB count file
    (counts: the file as an earlier run left it).  Returns (table, the reference's nSymbols, the file)."""
    counts = {} if counts is None else counts
    n_samples = n_symbols_ref = 0
    for strip in strips:
        for bits in R.keys_of(strip, elem_type).tolist():
            count = counts.get(bits, 0)
            counts[bits] = R._wrap32(count + 1)    # count + 1 of a Java int
            n_samples += 1
            if count == 0:
                n_symbols_ref += 1
    sym = sorted(counts)
    cnt = [counts[k] for k in sym]
    return table(sym, cnt, n_samples), n_symbols_ref, counts


def short_order(values):
    """the symbols of SHORT cells in table order: 0 .. 32767 in front of 0xFFFF8000 .. 0xFFFFFFFF"""
    return np.unique(np.asarray(values, np.int16).astype(np.int32).view(np.uint32))


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
