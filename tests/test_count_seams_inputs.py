"""The helpers of tests/count_seams.py, checked without a GPU: the vectorised framing and its table-driven CRC-32C byte for byte
against the per-record framing of tests/test_gpu_records_dev.py with the oracle's gvo_crc32c in the checksum's place, the sequence
rule's own property, the windowed block model against tests/block_ref.py, and the pool of the partition tests against the oracle's
decoders."""
import struct

import numpy as np
import pytest

import block_ref
import count_seams as S
import oracle
import test_gpu_records_dev as RD


@pytest.fixture()
def oracle_crc(monkeypatch):
    """_frame / _frame_elems with the oracle's CRC-32C where they call the library's"""
    monkeypatch.setattr(RD, "_crc", lambda b: oracle.crc32c(bytes(b)))


def test_crc32c_rows_is_the_oracles():
    rng = np.random.default_rng(1)
    assert S.crc32c_rows(np.frombuffer(b"123456789", np.uint8)[None])[0] == 0xE3069283
    for length in (0, 1, 3, 36, 257):
        rows = rng.integers(0, 256, (50, length), dtype=np.uint8)
        assert S.crc32c_rows(rows).tolist() == [oracle.crc32c(row.tobytes()) for row in rows], length


@pytest.mark.parametrize("length", [1, 16, 19, 1280])          # record sizes 24, 40, 40 (three bytes of padding), 1304
@pytest.mark.parametrize("crc", [True, False])
def test_one_element_framing(oracle_crc, length, crc):
    rng = np.random.default_rng(length)
    n = 300
    elements = rng.integers(0, 256, (n, length), dtype=np.uint8)
    indices = rng.integers(-2**31, 2**31, n)
    got = S.frame_records(indices, elements, crc)
    for t in range(n):
        assert got[t].tobytes() == RD._frame(int(np.int32(indices[t])), elements[t].tobytes(), crc=crc), t
    assert (got[:, -4:] == 0).all() != crc


@pytest.mark.parametrize("lengths", [(16, 8), (5, 7, 3), (640, 1280, 1280), (1,) * 16])
def test_several_elements_framing(oracle_crc, lengths):
    rng = np.random.default_rng(sum(lengths))
    n = 200
    elements = [rng.integers(0, 256, (n, length), dtype=np.uint8) for length in lengths]
    indices = rng.integers(0, 2**31, n)
    for crc in (True, False):
        got = S.frame_records_elems(indices, elements, crc)
        for t in range(n):
            assert got[t].tobytes() == RD._frame_elems(int(indices[t]), [el[t].tobytes() for el in elements], crc=crc), t


def test_assemble_mixed_sizes(oracle_crc):
    rng = np.random.default_rng(7)
    pool = [bytes(rng.integers(0, 256, length, dtype=np.uint8)) for length in (30, 31, 30, 200, 1280, 31)]
    which = rng.integers(0, len(pool), 500)
    indices = rng.permutation(5000)[:500]
    blob, offsets = S.assemble(pool, which, indices)
    want, want_offsets = RD._concat([RD._frame(int(i), pool[k]) for i, k in zip(indices, which)])
    assert np.array_equal(offsets, want_offsets) and np.array_equal(blob, want)
    triples = [[pool[0], pool[3], pool[1]], [pool[2], pool[3], pool[5]], [pool[4], pool[4], pool[4]]]
    which = rng.integers(0, 3, 300)
    blob, offsets = S.assemble(triples, which, indices[:300], crc=False)
    want, want_offsets = RD._concat([RD._frame_elems(int(i), triples[k], crc=False) for i, k in zip(indices, which)])
    assert np.array_equal(offsets, want_offsets) and np.array_equal(blob, want)


def test_a_million_records_take_under_a_second():
    import time
    n = (1 << 20) + 5
    elements = np.random.default_rng(2).integers(0, 256, (n, 16), dtype=np.uint8)
    t0 = time.perf_counter()
    records = S.frame_records(np.arange(n), elements)
    took = time.perf_counter() - t0
    assert records.shape == (n, 40)
    for t in (0, (1 << 20) - 1, 1 << 20, n - 1):
        assert struct.unpack("<I", records[t, -4:].tobytes())[0] == oracle.crc32c(records[t, :-4].tobytes())
    print("framing of %d records: %.2f s" % (n, took))
    assert took < 5.0, took                      # (well under a second on an idle core; the bound leaves room for a loaded one)


@pytest.mark.parametrize("n,period,n_pool", [(1023, 1024, 40), (1025, 1024, 40), (3100, 1024, 40), (70, 8, 12), ((1 << 20) + 7, 1 << 20, 32)])
def test_sequence_rule(n, period, n_pool):
    placed = {t: t % 3 for t in (period - 1, period, period + 1) if t < n}
    seq = S.sequence(5, n, period, n_pool, placed)
    assert seq.shape == (n,) and seq.min() >= 0 and seq.max() < n_pool
    for shift in range(period, n, period):
        assert (seq[shift:] != seq[:n - shift]).all()
    assert all(seq[t] == k for t, k in placed.items())
    assert np.array_equal(seq, S.sequence(5, n, period, n_pool, placed))           # seeded
    assert len(set(seq.tolist())) == n_pool                                         # the whole pool is used
    with pytest.raises(AssertionError):
        S.sequence(5, 4 * period + 1, period, 4)                                    # more periods than contents: cannot hold


def test_sequence_refuses_equal_hand_placed_records():
    with pytest.raises(AssertionError):
        S.sequence(1, 40, 8, 12, {3: 5, 11: 5})


@pytest.mark.parametrize("tile,grid", [((5, 5), (10, 10)), ((6, 6), (10, 10)), ((7, 9), (23, 31)), ((2, 2), (9, 11))])
def test_windowed_block_model(tile, grid):
    rng = np.random.default_rng(tile[0])
    nrt, nct = block_ref.tiles_of(grid, tile)
    nt, cells = nrt * nct, tile[0] * tile[1]
    indices = np.concatenate([rng.permutation(nt), [0, nt - 1, -1, nt, 2**31 - 1, -2**31, 1]])      # duplicates, indices outside
    tiles = rng.integers(-30000, 30000, (indices.size, cells)).astype(np.int16)
    ok = rng.random(indices.size) > 0.2
    ok[-1] = False                                                                  # the later entry of tile 1 failed
    rects = [(0, 0) + grid, (grid[0] - 1, grid[1] - 1, 1, 1), (1, 2, grid[0] - 2, grid[1] - 3), (tile[0] - 1, tile[1] - 1, 2, 2),
             (tile[0], 0, 1, grid[1])]
    for rect in rects:
        for status in (None, ok):
            want = block_ref.block_from_tiles(grid, tile, rect, indices, tiles, -7, ok=status)
            assert np.array_equal(S.block_from_tiles(grid, tile, rect, indices, tiles, -7, ok=status), want), (rect, status is None)


def test_partition_pool_decodes_to_its_tiles():
    tiles, packs = S.partition_pool()
    r, c = S.POOL_SHAPE
    dec = {0: oracle.codec_huffman_decode, 1: oracle.codec_deflate_decode, 3: oracle.codec_canon_decode, 4: oracle.lsop12_decode}
    assert tiles.shape == (40, r * c) and set(packs) == set(S.POOL_SLOTS)
    for slot, ps in packs.items():
        for k, p in enumerate(ps):
            assert np.array_equal(np.asarray(dec[slot](r, c, p)).reshape(-1), tiles[k]), (slot, k)
    assert len(S.standard_form(tiles, "short")[0]) == 2 * r * c and len(S.standard_form(tiles)[0]) == 4 * r * c
