"""The hand-built DEFLATE catalogue (tests/deflate_craft.py) against the host's zlib, on the CPU: every valid stream inflates
to what the assembler's own LZ77 replay says, every rejecting stream provokes the message it was built for, all fifteen
messages of inflate.c are reached, and every stream that ends inside a field makes zlib hand out its prefix and wait.  This
proves that the catalogue reaches each rule before tests/test_gpu_inflate_crafted.py holds the GPU inflater to it."""
import zlib

import pytest

import deflate_craft as dc


@pytest.fixture(scope="module")
def catalogue():
    return dc.cases()


def _zlib(stream):
    """(output, eof, message): one decompressobj fed the whole stream"""
    d = zlib.decompressobj()
    try:
        out = d.decompress(stream)
    except zlib.error as e:
        return None, False, str(e)
    return out, d.eof, None


def test_writer_and_canonical_codes():
    w = dc.BitWriter()
    w.bits(0b101, 3)                     # plain field: LSB first
    w.code(0b110, 3)                     # Huffman code: MSB first, so 1, 1, 0 follow
    assert w.bitpos == 6 and w.getvalue() == bytes([0b011101])
    # RFC 1951 3.2.2's example: lengths (3, 3, 3, 3, 3, 2, 4, 4) -> codes 010 011 100 101 110 00 1110 1111
    assert dc.canonical([3, 3, 3, 3, 3, 2, 4, 4]) == [(2, 3), (3, 3), (4, 3), (5, 3), (6, 3), (0, 2), (14, 4), (15, 4)]
    for k in range(2, 300):
        assert sum(2.0 ** -n for n in dc.complete_lengths(k)) == 1.0
    for n in (30, 286):
        lens = dc.spine_lengths([3, 1, 2], n)
        assert sum(2.0 ** -v for v in lens) == 1.0 and max(lens) == 15 and min(lens) == 1 and lens[3] == 1
    data = bytes(range(256)) * 40
    assert dc.adler32(data) == zlib.adler32(data)


def test_valid_cases_inflate_to_the_model(catalogue):
    n = 0
    for c in catalogue:
        if c.kind != "valid":
            continue
        out, eof, msg = _zlib(c.stream)
        assert msg is None and eof and out == c.expect, (c.name, msg, eof)
        n += 1
    assert n == 19
    names = {c.name for c in catalogue}
    for want in ("every_code_length_1_to_15", "largest_header_286_30", "every_length_symbol", "every_distance_symbol",
                 "overlapping_matches", "hbm_readback_distances", "one_code_distance_set_used", "empty_distance_set_literals_only",
                 "litlen_set_is_only_256", "repeat_runs_from_litlen_into_distance_lengths", "repeat_16_of_a_zero_from_17_18",
                 "many_empty_stored_and_fixed_blocks", "input_across_512_byte_refills", "preset_dictionary_header"):
        assert "valid/" + want in names, want


def test_preset_dictionary_header_is_need_dict(catalogue):
    (c,) = [c for c in catalogue if c.kind == "needdict"]
    out, eof, msg = _zlib(c.stream)
    assert msg is not None and not any(m in msg for m in dc.MESSAGES), msg        # Z_NEED_DICT, not a data error
    assert zlib.decompressobj(zdict=b"some dictionary").decompress(b"") == b""


def test_rejecting_cases_provoke_their_messages(catalogue):
    seen = {}
    for c in catalogue:
        if c.kind != "reject":
            continue
        out, eof, msg = _zlib(c.stream)
        assert msg is not None and c.expect in msg, (c.name, msg)
        seen[c.expect] = seen.get(c.expect, 0) + 1
    assert set(seen) == set(dc.MESSAGES) and len(dc.MESSAGES) == 15
    # the sub-cases the rules have
    assert seen["too many length or distance symbols"] == 4 and seen["invalid code lengths set"] >= 2
    assert seen["invalid bit length repeat"] == 4 and seen["invalid literal/lengths set"] == 3 and seen["invalid distances set"] == 3
    assert seen["invalid literal/length code"] == 2 and seen["invalid distance code"] >= 4 and seen["invalid distance too far back"] == 3


def test_streams_that_end_inside_a_field_make_zlib_wait(catalogue):
    per_kind = {}
    for c in catalogue:
        if c.kind != "ended":
            continue
        out, eof, msg = _zlib(c.stream)
        assert msg is None and not eof and out == c.expect, (c.name, msg, eof, out)
        _, kind, phase, _ = c.name.split("/")
        per_kind.setdefault(kind, set()).add(phase)
    assert set(per_kind) == set(dc.FIELD_KINDS) and len(dc.FIELD_KINDS) == 16
    for kind, phases in per_kind.items():
        assert phases == {"phase%d" % k for k in range(8)}, kind
        assert any(n.startswith("ended/%s/" % kind) for n in dc.ENDS_EXACTLY_IN_FRONT), kind


def test_the_empty_distance_set_waits_for_its_bit(catalogue):
    """lit/len lengths {97: 1, 256: 2, 257: 2}, no distance code, length symbol 257 (no extra bits) whose last bit is the last
    bit of the input: zlib hands out the literals and waits -- it needs one bit before it looks at its invalid-code markers --
    and with any real bit behind it says `invalid distance code`."""
    d = dc.Deflate()
    d.dynamic({97: 1, 256: 2, 257: 2}, [0], final=True)
    n = (-(d.w.bitpos + 2)) % 8                   # one-bit literals up to where the two-bit code of 257 ends a byte
    for _ in range(n):
        d.lit(97)
    d.length(257)
    assert d.w.bitpos % 8 == 0 and n > 0
    assert _zlib(dc.zlib_wrap(d.raw(), adler="none")) == (b"a" * n, False, None)
    for more in (b"\x00", b"\xff"):
        assert "invalid distance code" in _zlib(dc.zlib_wrap(d.raw() + more, adler="none"))[2]
    # the catalogue's own entry of this kind: k shifting literals, the block's literal, 257 -- and nothing behind it
    waits = [c for c in catalogue if c.name.startswith("ended/distance_code_empty_set/") and c.name in dc.ENDS_EXACTLY_IN_FRONT]
    assert waits
    for c in waits:
        k = int(c.name.split("/")[2][len("phase"):])
        assert c.expect == b"a" * (k + 1) and _zlib(c.stream) == (c.expect, False, None)
        assert "invalid distance code" in _zlib(c.stream + b"\x00")[2]


@pytest.mark.parametrize("how", ["stored", "fixed", "dyn_literals", "dyn15", "mixed"])
def test_the_plain_compressors_round_trip(how):
    data = dc.noise(700, 3) + b"abcabcabd" * 30 + bytes(300) + dc.noise(50, 4) * 6
    phases = set()
    for k in range(8):
        z, phase = dc.compress(data, how, phase_blocks=k)
        assert zlib.decompress(z) == data
        phases.add(phase)
    assert phases == ({0} if how == "stored" else set(range(8)))
    assert dc.compress(b"", how)[0] and zlib.decompress(dc.compress(b"", how)[0]) == b""
    assert zlib.decompress(dc.compress(b"q", how)[0]) == b"q"
