"""gf_file_inspect_dev past its count and segment seams, on the images of tests/inspect_seams.py (tests/test_inspect_seams_inputs.py
proves on the CPU that each crosses the seam it is named for): a second workgroup of directory entries and of segments, a second
and third round of k_inspect_chain's scan, links that fail in a later round with lane 0's walk behind them, k_inspect_crc's stride
over more records than it has waves, records of more chunks than k_inspect_crc_large has waves, more large records and more bad
tiles than k_inspect_fold has threads, a segment size above the smallest.  Every device result is held to the host form
(dev_equals_host of tests/test_gpu_file_inspect.py: report, bad tiles, records, guards) AND to what the builder's ledger
predicts, since the host form shares gfInspectStepWords with the kernels."""
import pytest

import gridfour_amd
from gridfour_amd import GvrsFileHip, _lib

import inspect_seams as S
from test_gpu_file_inspect import dev_equals_host

pytestmark = pytest.mark.gpu
IDS = ["%s: %s" % c for c in S.CASES]


@pytest.fixture(scope="module")
def ctx():
    return gridfour_amd.GvrsHipContext()


def held_to_both(ctx, family, variant):
    image, ledger = S.case(family, variant)
    got = dev_equals_host(ctx, image, (family, variant))
    assert S.differences(got, S.expect(ledger, S.checksums_of(family, variant))) == [], (family, variant)
    return got


@pytest.mark.parametrize("family,variant", S.CASES, ids=IDS)
def test_cases(ctx, family, variant):
    got = held_to_both(ctx, family, variant)
    assert got.tile_dir_passed == int(S.checksums_of(family, variant))


@pytest.mark.parametrize("cap", (0, 1, 63, 64, 65, 1023, 1024, 1025, 2559, 2560, 2561))
def test_bad_tile_capacity(ctx, cap):
    """the list is cut inside a wave, on a wave's end, inside a later round of the compaction and not at all"""
    image, ledger = S.case("many_tiles", "every second tile")
    want = S.expect(ledger)
    got = GvrsFileHip(image).inspect_dev(ctx, bad_cap=cap)
    assert got.n_bad_tiles == 2560 and got.bad_tiles == want["bad_tiles"][:cap] and got.guards_intact
    assert S.differences(got, want, bad_cap=cap) == []


@pytest.mark.parametrize("family,variant", [("many_records", "fails behind the seam"), ("long_span", "sound"), ("long_span", "size word 16 too large")])
def test_record_capacity(ctx, family, variant):
    """one record short of the walk (counted by the chain's scan, or by lane 0's walk from the scan's sum): GF_ERR_CAPACITY, the count
    named and nothing written; the exact room; the binding's default, which asks once more where the plan's guess is too small"""
    image, ledger = S.case(family, variant)
    want = S.expect(ledger)
    n = want["n_records"]
    f = GvrsFileHip(image)
    st, got = f.inspect_dev(ctx, max_records=n - 1, return_code=True)
    assert st == _lib.ERR_CAPACITY and got.status == _lib.ERR_CAPACITY and got.n_records == n
    assert got.guards_intact and got.bad_tiles == [] and (got.records_raw == 0x7f).all(), "a failed call wrote into the list or the records"
    got = f.inspect_dev(ctx, max_records=n)
    assert S.differences(got, want) == [] and got.guards_intact
    assert (f.inspect_plan(len(image))[2] < n) == (family == "many_records")       # (the retry path of test_gpu_file_inspect.test_capacity)
    got = f.inspect_dev(ctx)
    assert S.differences(got, want) == [] and got.guards_intact


@pytest.mark.parametrize("family,variant", [("many_tiles", "every second tile"), ("many_records", "fails behind the seam"), ("long_span", "false anchor"),
                                            ("large_records", "trailing bytes of the second"), ("many_large", "two fail"), ("wide_segments", "flipped tile")])
def test_without_the_record_list(ctx, family, variant):
    image, ledger = S.case(family, variant)
    got = GvrsFileHip(image).inspect_dev(ctx, with_records=False)
    assert S.differences(got, S.expect(ledger), with_records=False) == [] and got.records is None and got.guards_intact


def test_one_context_up_and_down():
    """A context of its own: its buffer grows with every image on the way up and is larger than needed on the way down, where an anchor,
    a count or a large record's sum left by the larger image would show"""
    ctx = gridfour_amd.GvrsHipContext()
    cases = [("many_tiles", "pair 2047"), ("many_records", "fails behind the seam"), ("long_span", "size word 16 too large"),
             ("large_records", "last whole piece of the first"), ("many_large", "two fail"), ("wide_segments", "flipped tile")]
    sizes = [len(S.case(*c)[0]) for c in cases]
    assert sizes == sorted(sizes)
    for family, variant in cases + cases[-2::-1]:
        held_to_both(ctx, family, variant)
