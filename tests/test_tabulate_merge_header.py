"""CPU-only: the merge of two symbol tables as gridfour_amd/csrc/gvrs_tabulate_common.h states it for host and device -- the split
of the merged sequence, the window of a chunk, the run with its pair rule -- compiled with g++ as a stand-alone program
(tests/csrc/tabulate_merge_harness.cpp, under AddressSanitizer and UBSan where the compiler has them) that drives them chunk by
chunk and lane by lane as k_tab_merge does, against the numpy model of tests/tabulate_acc_ref.py: the chunks must tile the merged
sequence exactly, so every table must be the model's entry for entry."""
import itertools

import numpy as np
import pytest

import tabulate_acc_cases as KA
import tabulate_acc_ref as A


@pytest.fixture(scope="module")
def exe():
    return KA.build_merge_harness()


def _check(exe, cases, tmp):
    got = KA.run_merge_harness(exe, cases, tmp)
    for (chunk, per, a, b), (sym, cnt, scalars) in zip(cases, got):
        want = A.merge(a, b)
        assert np.array_equal(sym, want[0]) and np.array_equal(cnt, want[1]), (chunk, per, a[0], b[0], sym, want[0])
        assert scalars == (want[2]["n_unique"], want[2]["n_repeated"], want[2]["max_count"]), (chunk, per, scalars, want[2])
    return got


def test_every_pair_of_small_tables_at_every_small_chunk(exe, tmp_path):
    """all pairs of subsets of {0 .. 5} for chunks of 1 .. 4 positions and lanes of 1 and 2: every way an equal pair can lie on,
    in front of and behind a seam between two chunks and between two lanes"""
    rng = np.random.default_rng(1)
    subsets = [[v for v in range(6) if m >> v & 1] for m in range(64)]
    tables = [A.table(s, rng.integers(1, 50, len(s))) for s in subsets]
    cases = [(chunk, per, a, b) for chunk in (1, 2, 3, 4) for per in (1, 2) if per <= chunk for a, b in itertools.product(tables, tables)]
    assert len(cases) == 7 * 64 * 64
    _check(exe, cases, tmp_path)


def test_corner_symbols_and_wrapping_counts(exe, tmp_path):
    """the four corner symbols in every pair of subsets, with counts that wrap: 0x7FFFFFFF + 1, -1 + 1, INT_MIN + INT_MIN"""
    subsets = [[v for k, v in enumerate(KA.CORNERS) if m >> k & 1] for m in range(16)]
    counts = {0: 2 ** 31 - 1, 0x7FFFFFFF: -1, 0x80000000: -2 ** 31, 0xFFFFFFFF: 7}
    ones = {0: 1, 0x7FFFFFFF: 1, 0x80000000: -2 ** 31, 0xFFFFFFFF: 2 ** 31 - 7}
    cases = [(chunk, 1, A.table(sa, [counts[v] for v in sa]), A.table(sb, [ones[v] for v in sb])) for chunk in (1, 2, 3, 4, 8)
             for sa, sb in itertools.product(subsets, subsets)]
    got = _check(exe, cases, tmp_path)
    full = got[16 * 16 - 1]                                                # chunk 1, both tables hold all four
    assert full[0].tolist() == list(KA.CORNERS) and full[1].tolist() == [-2 ** 31, 0, 0, -2 ** 31] and full[2] == (0, 0, 0)


def test_random_tables_at_the_real_chunk(exe, tmp_path):
    """tables of a few chunks at GF_TAB_MERGE_BLOCK positions a chunk and the kernel's positions a lane: dense symbols (many equal
    pairs), sparse ones over the whole 32-bit range, one table inside a gap of the other, sizes around the chunk's"""
    rng = np.random.default_rng(2)
    B, P = KA.MERGE_BLOCK, KA.MERGE_PER
    cases = []
    for na, nb, span, wrap in ((B - 1, 0, 3 * B, False), (0, B + 1, 3 * B, False), (B // 2, B // 2, B, True), (B, B, 3 * B // 2, True),
                               (2 * B + 1, B - 3, 3 * B, True), (3 * B // 2 + 5, 3 * B // 2 - 4, 2 ** 32, False), (5, 3 * B, 4 * B, True)):
        cases.append((B, P, KA.random_table(rng, na, span, wrap), KA.random_table(rng, nb, span, wrap)))
    lo, hi = KA.random_table(rng, B + 7, 2 * B), KA.random_table(rng, B + 9, 2 * B)
    far = A.table(hi[0] + np.uint32(2 ** 31), hi[1])
    gap = A.table(np.concatenate([lo[0], hi[0] + np.uint32(2 ** 30)]), np.concatenate([lo[1], hi[1]]))
    inside = A.table(hi[0][:B // 2] + np.uint32(2 ** 20), hi[1][:B // 2])
    cases += [(B, P, lo, far), (B, P, far, lo), (B, P, lo, lo), (B, P, gap, inside), (B, P, inside, gap), (B, 1, lo, hi), (B, B, lo, hi)]
    got = _check(exe, cases, tmp_path)
    assert sum(g[0].size for g in got) > 20 * B // 2
