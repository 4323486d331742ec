"""Inputs shared by the tests of merged symbol tables and accumulated strips (tests/test_tabulate_merge_header.py on the CPU,
tests/test_gpu_tabulate_acc.py on the GPU): the implementation's constants, read out of gridfour_amd/csrc/gvrs_tabulate_common.h by
text so that the cases straddle them whatever they become, the build of the CPU harness (tests/csrc/tabulate_merge_harness.cpp),
and tables with a shape."""
import os
import re
import subprocess

import numpy as np

import tabulate_acc_ref as A
import tabulate_cases as K


def _constants():
    text = open(K.HEADER).read()
    out = {}
    for name in ("GF_TAB_MERGE_BLOCK", "GF_TAB_SHORT_MAX_GROUPS", "GF_TAB_SHORT_WIN_LO", "GF_TAB_SHORT_WIN_HI"):
        m = re.search(r"^#define\s+%s\s+\(?(-?\d+)\)?" % name, text, re.M)
        assert m, name
        out[name] = int(m.group(1))
    return out


CONST = _constants()
MERGE_BLOCK, SHORT_MAX_GROUPS = CONST["GF_TAB_MERGE_BLOCK"], CONST["GF_TAB_SHORT_MAX_GROUPS"]
WIN_LO, WIN_HI = CONST["GF_TAB_SHORT_WIN_LO"], CONST["GF_TAB_SHORT_WIN_HI"]
MERGE_PER = MERGE_BLOCK // K.SORT_THREADS          # positions of one lane of k_tab_merge
CORNERS = (0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF)


def build_merge_harness():
    """the stand-alone program, with the sanitizers where g++ has them (it is no code loaded into Python)"""
    src, exe = os.path.join(K.HERE, "csrc", "tabulate_merge_harness.cpp"), os.path.join(K.HERE, "csrc", "tabulate_merge_harness")
    base = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-o", exe, src]
    if subprocess.call(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(base)
    return exe


def run_merge_harness(exe, cases, tmp):
    """cases: [(chunk, per, table a, table b)] -> [(symbols, counts, (unique, repeated, most))]"""
    words = [np.array([len(cases)], np.uint32)]
    for chunk, per, a, b in cases:
        words += [np.array([chunk, per, a[0].size, b[0].size], np.uint32), a[0].astype(np.uint32), a[1].astype(np.int32).view(np.uint32),
                  b[0].astype(np.uint32), b[1].astype(np.int32).view(np.uint32)]
    fin, fout = os.path.join(str(tmp), "merge_in.bin"), os.path.join(str(tmp), "merge_out.bin")
    np.concatenate(words).tofile(fin)
    subprocess.check_call([exe, fin, fout])
    raw, at, out = np.fromfile(fout, np.uint32), 0, []
    for _ in cases:
        n = int(raw[at])
        sym, cnt, sc = raw[at + 1:at + 1 + n], raw[at + 1 + n:at + 1 + 2 * n].view(np.int32), raw[at + 1 + 2 * n:at + 4 + 2 * n]
        out.append((sym, cnt, (int(sc[0]), int(sc[1]), int(sc[2]))))
        at += 4 + 2 * n
    assert at == raw.size
    return out


def random_table(rng, n, span, wrap=False):
    """n distinct symbols below span (spread over the whole 32-bit range when span is 2^32) with counts 1 .. 9; wrap: some counts
    at the edges of an int32"""
    sym = np.sort(rng.choice(span, n, replace=False)).astype(np.uint32) if span < 2 ** 31 else np.unique(
        rng.integers(0, span, n, dtype=np.uint64).astype(np.uint32))
    cnt = rng.integers(1, 10, sym.size).astype(np.int32)
    if wrap and sym.size:
        at = rng.random(sym.size) < 0.05
        cnt[at] = rng.choice(np.array([2 ** 31 - 1, -2 ** 31, -1, 0, 2 ** 31 - 2], np.int64), int(at.sum())).astype(np.int32)
    return A.table(sym, cnt)
