"""ICompressionDecoder.analyze of CodecCanonHuffman (CodecCanonHuffman.java:217-324): the CanonHuffmanStats sums and the escape
table gathered by k_canon_decode<true> + k_canon_stats, against the restatement in canon_analyze_twin.py."""
import io
import struct

import numpy as np
import pytest

import oracle
from canon_analyze_twin import Twin, assert_matches
from tilegen import make_tile

pytestmark = pytest.mark.gpu
NULL = -2 ** 31


def _codec(**kw):
    import gridfour_amd
    return gridfour_amd.CodecCanonHuffmanHip(**kw)


def _twin_of(n_rows, n_cols, packings):
    twin = Twin()
    ok = [twin.analyze(n_rows, n_cols, p) for p in packings]
    return twin, ok


def _mixed_packings(codec, nr=60, nc=90):
    tiles = [make_tile(k, nr, nc, seed=s) for s, k in enumerate(["smooth", "ramp", "noise8", "noise16", "steps", "uniform", "sparse_big",
                                                                   "extremes"])]
    with_nulls = make_tile("smooth", nr, nc, seed=40).copy()
    with_nulls.reshape(nr, nc)[20:30, 10:70] = NULL
    tiles.append(with_nulls)
    r, c = np.arange(nr)[:, None], np.arange(nc)[None, :]
    tiles.append((3 * c * c + 17 * r * r).astype(np.int32).ravel())           # a surface the Linear predictor takes
    packs, preds, st = codec.encode_batch(0, nr, nc, np.stack(tiles))
    assert (st == 0).all()
    return packs, preds


def _differencing_packing(n_rows, n_cols, residuals, seed=12345):
    """A Differencing packing (predictor byte 1) around a text of our choosing: header + CanonicalHuffman.encode."""
    text = np.asarray(residuals, np.int64).astype(np.int32)
    assert text.size == n_rows * n_cols - 1
    data, _, _ = oracle.canon_encode(text, 48, bytes([0, 1]) + struct.pack("<i", seed))
    return data


def test_mixed_set_matches_the_twin():
    codec = _codec()
    nr, nc = 60, 90
    packs, preds = _mixed_packings(codec, nr, nc)
    assert {0, 1, 2, 3, 4} <= set(int(p) for p in preds)          # the uniform form and all four predictors
    codec.clearAnalysisData()
    st = codec.analyze_batch(nr, nc, packs)
    twin, ok = _twin_of(nr, nc, packs)
    assert all(ok) and (st == 0).all()
    assert_matches(codec.analysis_data(), codec.escape_counts(), twin)
    assert int(codec.analysis_data()[0]["n_tiles"]) == 1 and int(codec.analysis_data()[5]["n_tiles"]) == len(packs)


def test_escape_ladder_covers_every_class():
    nr, nc = 40, 50
    n = nr * nc - 1
    rng = np.random.default_rng(7)
    ladder = [5, -300, 400, -1500, 2000, -5000, 8000, -20000, 30000, -1000000, 8000000, -100000000, 2000000000,
              -8350000, -8388608, -8333609, -8333608, NULL, NULL, -2 ** 31 + 1]
    packs = []
    for k in range(4):
        res = rng.integers(-6, 7, n).astype(np.int64)
        pos = rng.choice(n, size=len(ladder) * 3, replace=False)
        res[pos] = np.array(ladder * 3, np.int64)
        packs.append(_differencing_packing(nr, nc, res, seed=k))
    twin, ok = _twin_of(nr, nc, packs)
    assert all(ok)
    assert all(c > 0 for c in twin.escapes), twin.escapes           # every class: 2, 4, 6, 8, 16, 24 bits
    codec = _codec()
    st = codec.analyze_batch(nr, nc, packs)
    assert (st == 0).all()
    assert_matches(codec.analysis_data(), codec.escape_counts(), twin)
    e = codec.escape_counts()
    want_bits = 2 * e[0] + 4 * e[1] + 8 * e[3] + 16 * e[4] + 24 * e[5]          # the 6-bit class left out
    assert int(codec.analysis_data()[1]["sum_escape_bits"]) == want_bits
    assert want_bits != want_bits + 6 * e[2]


def test_predictor_byte_quirks():
    codec = _codec()
    nr, nc = 60, 90
    packs, preds = _mixed_packings(codec, nr, nc)
    base = next(p for p, q in zip(packs, preds) if q == 3)
    patched = {b: base[:1] + bytes([b]) + base[2:] for b in (0, 5, 6, 0x80)}
    # 0 with a text: record 0; 5: "All Predictors" twice
    codec.clearAnalysisData()
    st = codec.analyze_batch(nr, nc, [patched[0], patched[5]])
    assert (st == 0).all()
    twin, ok = _twin_of(nr, nc, [patched[0], patched[5]])
    assert all(ok)
    assert_matches(codec.analysis_data(), codec.escape_counts(), twin)
    got = codec.analysis_data()
    assert int(got[0]["n_tiles"]) == 1 and int(got[5]["n_tiles"]) == 3
    # 6 and 0x80: analyze throws after the escape table was added to; no record changes
    before, esc_before = codec.analysis_data(), codec.escape_counts()
    st = codec.analyze_batch(nr, nc, [patched[6], patched[0x80]])
    assert (st != 0).all()
    assert np.array_equal(codec.analysis_data(), before)
    twin6, ok6 = _twin_of(nr, nc, [patched[6], patched[0x80]])
    assert ok6 == [False, False]
    assert [int(a - b) for a, b in zip(codec.escape_counts(), esc_before)] == twin6.escapes
    assert sum(twin6.escapes) > 0
    with pytest.raises(IOError):
        codec.analyze(nr, nc, patched[6])


def test_damaged_packings_count_nothing():
    codec = _codec()
    nr, nc = 60, 90
    packs, preds = _mixed_packings(codec, nr, nc)
    good = next(p for p, q in zip(packs, preds) if q == 1 and len(p) > 400)
    damaged = [good[:5], good[:2], bytes([0, 3, 1, 2, 3, 4]), good[:6], good[:len(good) // 2], good[:12]]
    codec.clearAnalysisData()
    st = codec.analyze_batch(nr, nc, damaged)
    assert (st != 0).all(), st
    twin, ok = _twin_of(nr, nc, damaged)
    assert not any(ok)
    got = codec.analysis_data()
    assert all(int(got[k]["n_tiles"]) == 0 for k in range(6))
    assert [int(x) for x in codec.escape_counts()] == [0] * 6
    for d in damaged:
        with pytest.raises(IOError):
            codec.analyze(nr, nc, d)


def test_accumulation_report_and_interleaved_decode():
    import gridfour_amd
    codec = _codec()
    nr, nc = 60, 90
    packs, preds = _mixed_packings(codec, nr, nc)
    codec.clearAnalysisData()
    assert codec.analysis_data() is None
    out = io.StringIO()
    codec.reportAnalysisData(out, 10)
    assert out.getvalue().endswith("   Tiles Compressed:  0\n")
    # two batches accumulate, and a decode on the same context between them still decodes
    assert (codec.analyze_batch(nr, nc, packs[:4]) == 0).all()
    vals, st = codec.decode_batch(nr, nc, packs)
    assert (st == 0).all()
    for t, p in enumerate(packs):
        assert np.array_equal(vals[t], oracle.codec_canon_decode(nr, nc, p)), t
    assert (codec.analyze_batch(nr, nc, packs[4:]) == 0).all()
    twin, _ = _twin_of(nr, nc, packs)
    assert_matches(codec.analysis_data(), codec.escape_counts(), twin)
    vals2, st2 = codec.decode_batch(nr, nc, packs)
    assert (st2 == 0).all() and np.array_equal(vals2, vals)
    # one analyze() == a batch of one
    single = _codec(context=codec.ctx)
    for p in packs[:3]:
        single.analyze(nr, nc, p)
    batch = _codec(context=codec.ctx)
    batch.analyze_batch(nr, nc, packs[:3])
    assert np.array_equal(single.analysis_data(), batch.analysis_data())
    assert np.array_equal(single.escape_counts(), batch.escape_counts())
    # the report: "Uniform Value" only where a uniform tile was counted, then the six rows of the escape table
    out = io.StringIO()
    codec.reportAnalysisData(out, len(packs))
    lines = out.getvalue().splitlines()
    assert lines[0].startswith("GVRS Canonical Huffman")
    assert any(line.startswith("   Uniform Value") for line in lines)
    assert "   All Predictors" in out.getvalue() and "Escape sequences" in lines
    i = lines.index("Escape sequences")
    assert lines[i + 1] == "length    count     n/tile  bits/tile"
    esc = codec.escape_counts()
    total = float(codec.analysis_data()[5]["n_tiles"])
    assert lines[i + 2:] == ["  %2d  %10d    %7.2f    %7.2f" % (b, c, c / total, b * (c / total))
                             for b, c in zip((2, 4, 6, 8, 16, 24), esc)]
    nonuniform = _codec(context=codec.ctx)
    nonuniform.analyze_batch(nr, nc, [p for p, q in zip(packs, preds) if q != 0])
    out = io.StringIO()
    nonuniform.reportAnalysisData(out, len(packs))
    assert "Uniform Value" not in out.getvalue() and "Differencing" in out.getvalue()
    codec.clearAnalysisData()
    assert codec.analysis_data() is None and codec.escape_counts() is None
    # the other codecs that have no analysis yet still say so
    with pytest.raises(NotImplementedError):
        gridfour_amd.CodecDeflateHip(context=codec.ctx).analyze_batch(nr, nc, packs[:1])


def test_large_dem_batch_both_prepass_forms():
    """at least GF_CANON_PREPASS_ONE_LANE_MAX + 200 tiles of the bench's tile shape (the code-length pre-pass takes its
    64-tiles-per-wave form), and a small batch of the same tiles (its wave-per-tile form)"""
    codec = _codec()
    nr, nc, nt = 120, 150, 3200
    tiles = oracle.dem_tiles(oracle.DEM_SEED + 2, nr, nc, 144, 0, nt)
    tiles[7, 300:2000] = NULL
    packs, preds, st = codec.encode_batch(0, nr, nc, tiles)
    assert (st == 0).all()
    twin, ok = _twin_of(nr, nc, packs)
    assert all(ok)
    codec.clearAnalysisData()
    assert (codec.analyze_batch(nr, nc, packs) == 0).all()
    assert_matches(codec.analysis_data(), codec.escape_counts(), twin)
    small = _codec(context=codec.ctx)
    assert (small.analyze_batch(nr, nc, packs[:100]) == 0).all()
    twin_s, _ = _twin_of(nr, nc, packs[:100])
    assert_matches(small.analysis_data(), small.escape_counts(), twin_s)
