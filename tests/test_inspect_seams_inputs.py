"""The images of tests/inspect_seams.py, checked without a GPU.  gf_file_inspect, the host form, must report of every image what the
builder's ledger predicts (report, bad tiles, records); and every image must cross the seam of gf_file_inspect_dev it is named for,
computed here from the ledger, the image's directory and gf_file_inspect_plan -- so that tests/test_gpu_inspect_seams.py provably
runs the code behind the seam.  The sequential restatement tests/gvrs_inspect_ref.py runs on many_tiles only: it is a Python loop."""
import numpy as np
import pytest

import gvrs_inspect_ref as R
import inspect_seams as S
from gridfour_amd import GvrsFileHip

IDS = ["%s: %s" % c for c in S.CASES]


def built(family, variant):
    image, ledger = S.case(family, variant)
    return image, ledger, S.model(image, ledger)


@pytest.mark.parametrize("family,variant", S.CASES, ids=IDS)
def test_host_form_reports_what_the_ledger_predicts(family, variant):
    image, ledger = S.case(family, variant)
    assert all(a[0] + a[1] <= b[0] for a, b in zip(ledger, ledger[1:])) and ledger[-1][0] + ledger[-1][1] == len(image)
    want = S.expect(ledger, S.checksums_of(family, variant))
    got = GvrsFileHip(image).inspect()
    assert S.differences(got, want) == [] and got.guards_intact
    assert got.tile_dir_located == 1 and got.tile_dir_passed == int(S.checksums_of(family, variant))
    sound = variant.startswith(("sound", "327", "checksums off", "false anchor"))
    assert (got.passed and got.complete and got.termination_pos == len(image)) == sound
    assert got.complete == (0 if "pair" in variant or "double" in variant else 1)


@pytest.mark.parametrize("variant", S.MANY_TILES)
def test_restatement_on_many_tiles(variant):
    image, ledger = S.case("many_tiles", variant)
    f = GvrsFileHip(image)
    want = R.inspect(image, R.facts_of(f))
    assert R.same(f.inspect(), want) == []
    assert want["records"] == S.expect(ledger)["records"] and want["bad_tiles"] == S.expect(ledger)["bad_tiles"]


def test_damage_is_what_the_variant_says():
    crc = lambda fam, var: [k for k, r in enumerate(S.case(fam, var)[1]) if r[4] == "crc"]
    stops = lambda fam, var: [k for k, r in enumerate(S.case(fam, var)[1]) if r[4] == "type9"]
    for k in (1023, 1024, 2047):
        assert crc("many_tiles", "pair %d" % k) == [k, k + 1]
    assert crc("many_tiles", "doubles 2000 and 1100") == [1100, 1101, 2000, 2001]
    assert crc("many_tiles", "doubles 1100 and 2060") == [1100, 1101, 2060, 2061]
    assert (crc("many_tiles", "double in front of a stop"), stops("many_tiles", "double in front of a stop")) == ([1100, 1101], [3000])
    assert (crc("many_tiles", "stop in front of a double"), stops("many_tiles", "stop in front of a double")) == ([3500, 3501], [3000])
    assert crc("many_records", "fails in front of the seam") == [S.CRC_WAVES - 1] and crc("many_records", "fails behind the seam") == [S.CRC_WAVES]
    assert len(crc("many_tiles", "every second tile")) == 2560 and len(crc("many_large", "two fail")) == 2
    for fam, (_, variants) in S.FAMILIES.items():
        for var in variants[1:]:
            if fam in ("large_records", "many_large", "wide_segments"):
                assert len(S.case(fam, var)[0]) == len(S.base(fam)[0]) and S.case(fam, var)[0] != S.base(fam)[0], (fam, var)


# ---- every image crosses the seam it is named for -------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", S.MANY_TILES)
def test_many_tiles_seams(variant):
    image, ledger, m = built("many_tiles", variant)
    # k_inspect_anchors: 18 to 20 workgroups; k_inspect_walk and k_inspect_list: a second one; k_inspect_fold: five rounds of records
    assert m["n_entries"] == (4500 if variant == "sound sub-rectangle" else 5120) and m["n_entries"] > 17 * S.ANCHOR_GROUP
    assert S.SEGMENT_GROUP < m["n_seg"] <= 2 * S.SEGMENT_GROUP and m["seg"] == S.MIN_SEGMENT
    assert max(m["anchors"]) > S.SEGMENT_GROUP and len(m["anchors"]) > 400
    assert len(ledger) == 5124 > 5 * S.CHAIN_ROUND
    assert [r[2] for r in ledger[:3]] == [1, 1, 1] and all(r[2] == 2 for r in ledger[3:-1]) and ledger[-1][2] == 5
    tiles = [r[3] for r in ledger[3:-1]]
    assert sorted(tiles) == list(range(S.N_TILES)) and tiles != sorted(tiles)
    f = GvrsFileHip(image)
    assert bool(f.info["dir_extended"]) == (variant == "sound extended")
    if variant == "sound sub-rectangle":
        assert f.info["dir_n_cols"] == 75 and f.info["dir_n_cols"] % 64 != 0 and f.info["dir_n_cols"] != S.N_TILE_COLS and f.info["dir_col0"] > 0


def test_every_second_tile_rounds():
    """k_inspect_fold compacts the bad tiles a round of 1,024 records at a time: every round holds some, the counts in front of the
    round boundaries are no multiples of 64 (a boundary falls inside a wave's worth of the list), no two are adjacent"""
    _, ledger, _ = built("many_tiles", "every second tile")
    bad = np.array([r[4] == "crc" and r[2] == 2 for r in ledger])
    assert bad.sum() == 2560 and not (bad[1:] & bad[:-1]).any()
    rounds = [int(bad[k:k + S.CHAIN_ROUND].sum()) for k in range(0, len(ledger), S.CHAIN_ROUND)]
    assert len(rounds) == 6 and sum(1 for c in rounds if c) >= 3 and rounds[0] == 511
    carried = np.cumsum(rounds)[:-1]
    assert (carried % 64 != 0).all(), carried
    want = S.expect(ledger)
    assert want["stop"] == S.END and want["complete"] == 1 and want["n_bad_tiles"] == 2560


def test_doubles_and_stops():
    """k_inspect_fold's search strides by 1,024: thread (i - 1) % 1,024 meets the double whose second record is i"""
    def stop_of(variant):
        want = S.expect(S.case("many_tiles", variant)[1])
        return want["stop"], want["n_records"]
    assert stop_of("pair 1023") == (S.TWO_CHECKSUM_FAILURES, 1025)        # the pair across the first round's end
    assert stop_of("pair 1024") == (S.TWO_CHECKSUM_FAILURES, 1026)        # ... behind it: thread 0's second turn
    assert stop_of("pair 2047") == (S.TWO_CHECKSUM_FAILURES, 2049)
    assert stop_of("doubles 2000 and 1100") == (S.TWO_CHECKSUM_FAILURES, 1102)
    assert stop_of("doubles 1100 and 2060") == (S.TWO_CHECKSUM_FAILURES, 1102)
    assert (1101 - 1) // S.CHAIN_ROUND == 1 and (2001 - 1) // S.CHAIN_ROUND == 1                  # both in the second turn
    assert (2061 - 1) % S.CHAIN_ROUND < (1101 - 1) % S.CHAIN_ROUND                                # a lower thread finds the later one
    assert stop_of("double in front of a stop") == (S.TWO_CHECKSUM_FAILURES, 1102)
    assert stop_of("stop in front of a double") == (S.BAD_RECORD_TYPE, 3001)


@pytest.mark.parametrize("variant", S.MANY_RECORDS)
def test_many_records_seams(variant):
    image, ledger, m = built("many_records", variant)
    n = len(ledger)
    assert n == {"32766": 32766, "32767": 32767, "32768": 32768}.get(variant, 33041)
    assert sum(1 for r in ledger if r[2] == 2) == 40 and sum(1 for r in ledger if r[2] == 1 and r[1] == 16) == n - 41
    # k_inspect_crc's work list is the walk's records and the directory slot
    assert (n + 1 > S.CRC_WAVES) == (variant not in ("32766", "32767"))
    assert m["n_seg"] > 2 * S.SEGMENT_GROUP and m["default_room"] < n
    per_segment = np.bincount((np.array([r[0] for r in ledger]) - S.content_pos()) // m["seg"])
    assert per_segment.max() == 64
    if n > S.CRC_WAVES + 1:
        assert ledger[S.CRC_WAVES][2] == 2 and ledger[S.CRC_WAVES - 1][2] == 1


@pytest.mark.parametrize("variant", S.LONG_SPAN)
def test_long_span_seams(variant):
    image, ledger, m = built("long_span", variant)
    seg, content = m["seg"], S.content_pos()
    assert seg == S.MIN_SEGMENT and m["n_seg"] > 2 * S.CHAIN_ROUND
    anchored = sorted(m["anchors"])
    per_round = [sum(1 for s in anchored if s // S.CHAIN_ROUND == r) for r in range(3)]
    assert per_round[0] >= 3 and per_round[1] > 100 and per_round[2] > 100, per_round
    gaps = [(b - a, a) for a, b in zip(anchored, anchored[1:])]
    assert max(gaps)[0] > S.CHAIN_ROUND + 500 and max(gaps)[1] < 5         # more than a round of segments without an anchor
    free = [r for r in ledger if r[2] == 0]
    assert len(free) == 1 and free[0][1] == 3 << 19 > 1 << 20
    seam = content + 2 * S.CHAIN_ROUND * seg
    k = [r[0] for r in ledger].index(seam)                               # a record starts on the round's seam, one ends there
    assert ledger[k - 1][0] + ledger[k - 1][1] == seam and ledger[k - 1][2] == 1 and ledger[k][2] == 2 and m["anchors"][2 * S.CHAIN_ROUND] == seam
    if variant == "sound":
        assert m["closes"] and m["first"] > 2 * S.CHAIN_ROUND and m["first"] == anchored[-1]
        return
    # the link fails in the chain's second round; lane 0 walks the rest, its count starting from two rounds' sum
    assert not m["closes"] and 1100 < m["first"] < 2 * S.CHAIN_ROUND
    nxt = anchored[anchored.index(m["first"]) + 1]
    assert nxt == 1701 and m["anchors"][nxt] not in set(m["walk"]) and m["anchors"][nxt] == content + nxt * seg + (64 if variant.startswith("size") else 16)
    rest = sum(1 for p in m["walk"] if p > m["anchors"][nxt])
    assert 1000 < rest < 20000 and rest + 1 < len(ledger)
    bad = [r for r in ledger if r[4]]
    if variant.startswith("size"):
        assert len(bad) == 1 and bad[0][1] == 80 and (bad[0][0] - content) // seg == 1701 and S.expect(ledger)["n_checksum_failures"] == 1
        (word,) = np.frombuffer(image, "<i4", 1, bad[0][0])
        nxt_rec = ledger[ledger.index(bad[0]) + 1]
        assert word == 80 and nxt_rec[0] == bad[0][0] + 80 and nxt_rec[:3] == (m["anchors"][1701] + 16, 72, 1)
    else:
        assert bad == []


def chunks_of(size, chunk):
    whole = (size - 4) & ~15
    return -(-whole // chunk), whole


def test_large_records_seams():
    image, ledger, m = built("large_records", "sound")
    chunk = m["chunk"]
    assert ledger[-1][2] == 5 and ledger[-1][1] - 4 > S.WAVE_CHUNKS * chunk    # the directory of 5,120 entries is handed on as well, twice:
    large = [r for r in ledger[:-1] if r[1] - 4 > S.WAVE_CHUNKS * chunk]       # as the walk's last record and in the directory slot
    assert [ledger.index(r) for r in large] == list(S.LARGE_AT) and [r[1] for r in large] == S.large_sizes(chunk)
    n_chunks = [chunks_of(r[1], chunk)[0] for r in large]
    assert n_chunks[0] == S.LARGE_WAVES and n_chunks[1] == S.LARGE_WAVES + 1 and n_chunks[2] > 2 * S.LARGE_WAVES and n_chunks[3] == S.WAVE_CHUNKS
    assert large[3][1] - 4 - 4 <= S.WAVE_CHUNKS * chunk                    # (one word less and a wave takes it)
    # the first chunk's weight is a product over the bits of its distance in 16-byte pieces: two[i] up to i = 17
    top = [int((chunks_of(r[1], chunk)[1] - chunk) // 16).bit_length() - 1 for r in large]
    assert top == [16, 17, 17, 9]
    assert all((chunks_of(r[1], chunk)[1] - chunk) // 16 < 1 << 18 for r in large)
    assert sorted((r[1] - 4) % 16 for r in large[:2]) == [4, 12]           # the trailing bytes behind the whole pieces
    assert large[0][1] > 1 << 20 and m["n_seg"] > 8 * S.CHAIN_ROUND         # the walk skips thousands of segments without an anchor
    for variant in S.LARGE_RECORDS[1:]:
        hurt, ledger2 = S.case("large_records", variant)
        (k,) = [i for i, r in enumerate(ledger2) if r[4]]
        (at,) = np.flatnonzero(np.frombuffer(hurt, np.uint8) != np.frombuffer(image, np.uint8)).tolist()
        off, (_, whole) = at - ledger[k][0], chunks_of(ledger[k][1], chunk)
        want = {"first chunk of the third": (S.LARGE_AT[2], off < chunk), "last whole piece of the first": (S.LARGE_AT[0], whole - 16 <= off < whole),
                "trailing bytes of the second": (S.LARGE_AT[1], whole <= off < ledger[k][1] - 4),
                "trailing bytes of the first": (S.LARGE_AT[0], whole <= off < ledger[k][1] - 4)}[variant]
        assert (k, True) == want, variant
        assert S.expect(ledger2)["n_checksum_failures"] == 1 and S.expect(ledger2)["bad_tiles"] == []


def test_many_large_seams():
    image, ledger, m = built("many_large", "sound")
    large = [k for k, r in enumerate(ledger) if r[1] - 4 > S.WAVE_CHUNKS * m["chunk"] and r[2] == 1]
    assert len(large) == S.N_MANY_LARGE > S.CHAIN_ROUND and all(ledger[k][1] == S.WAVE_CHUNKS * m["chunk"] + 8 for k in large)
    assert sum(1 for r in ledger if r[2] == 2) == 103 and 16 << 20 < len(image) < 18 << 20
    _, ledger2 = S.case("many_large", "two fail")
    assert [k for k, r in enumerate(ledger2) if r[4]] == [large[5], large[1027]]      # (1,027: the strided loop's second turn)


def test_wide_segments_seams():
    image, ledger, m = built("wide_segments", "sound")
    seg, content = m["seg"], S.content_pos()
    assert seg > S.MIN_SEGMENT and seg % 8 == 0 and seg & (seg - 1) != 0
    assert len(image) - content > S.WIDE_MARK == S.MIN_SEGMENT * S.MAX_SEGMENTS and m["n_seg"] <= S.MAX_SEGMENTS
    assert 38 << 20 < len(image) < 44 << 20
    named_behind = [s for s, q in m["anchors"].items() if q - content > S.WIDE_MARK]
    behind = [r for r in ledger if r[2] == 2 and r[0] - content > S.WIDE_MARK]
    assert len(behind) >= 200 and len(named_behind) >= 10 and min(named_behind) > S.WIDE_MARK // seg > 26000
    tiles = [r[3] for r in ledger if r[2] == 2]
    assert len(tiles) - len(set(tiles)) == 103                            # the old copies in front of their second copies
    assert sum(1 for r in ledger if r[2] == 0 and r[1] >= 4 << 20) == 6
    assert sum(1 for r in ledger if r[1] - 4 > S.WAVE_CHUNKS * m["chunk"] and r[2] == 1) == S.N_MANY_LARGE
    _, ledger2 = S.case("wide_segments", "flipped tile")
    (k,) = [i for i, r in enumerate(ledger2) if r[4]]
    assert ledger2[k][2] == 2 and ledger2[k][0] - content > S.WIDE_MARK and S.expect(ledger2)["bad_tiles"] == [ledger2[k][3]]


def test_images_are_built_once():
    assert S.base("many_large")[0] is S.base("many_large")[0] and S.case("long_span", "sound")[0] is S.case("long_span", "sound")[0]
