"""tests/caller_stream.py's table against include/gvrs_hip_codec.h, by text: every function of the header with a `void *stream`
parameter has a row (or stands in the written list of entry points without a case yet), and no row names a function that is gone.
A new device form cannot be added without a decision about the stream it runs on."""
import os
import re

import caller_stream as CS

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "gvrs_hip_codec.h")


def _stream_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)                      # comments name functions too
    out = []
    for m in re.finditer(r"\bgf_status\s+(\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2)):
            out.append(m.group(1))
    return out


def test_header_parse_finds_the_device_forms():
    names = _stream_functions()
    assert len(names) == len(set(names)) >= 39, names
    for known in ("gf_huffman_decode_batch_i32_dev", "gf_block_write_elems_dev", "gf_timer_start", "gf_timer_stop", "gf_synth_dem_style_dev",
                  "gf_lsop12_encode_batch_i32_dev_ex"):
        assert known in names, known
    assert "gf_context_reserve" not in names and "gf_huffman_decode_batch_i32" not in names


def test_every_stream_function_has_a_row():
    names = set(_stream_functions())
    rows = [r.name for r in CS.TABLE]
    assert len(rows) == len(set(rows)), "a function has two rows"
    listed = set(rows) | set(CS.NOT_COVERED)
    assert not set(rows) & set(CS.NOT_COVERED), sorted(set(rows) & set(CS.NOT_COVERED))
    assert names - listed == set(), "device forms without a row in tests/caller_stream.py: %s" % sorted(names - listed)
    assert listed - names == set(), "rows of tests/caller_stream.py for functions the header no longer has: %s" % sorted(listed - names)


def test_rows_have_a_class_and_cases():
    kinds = (CS.CAPTURE, CS.ENQUEUE, CS.SYNC_ONCE, CS.STREAM_ONLY)
    for r in CS.TABLE:
        assert r.kind in kinds, r.name
        assert r.cases or r.kind == CS.STREAM_ONLY, "%s has a row and no case" % r.name
        for ident, kind, builder in r.cases:
            assert (kind is None or kind in kinds) and callable(builder), (r.name, ident)
    assert all(k in kinds for k in CS.NOT_COVERED.values())
    ids = [c[0] for c in CS.cases(kinds)]
    assert len(ids) == len(set(ids))


def test_no_entry_point_is_left_without_a_case():
    """the list of entry points that have a class and no case is empty, and stays so: a new device form gets a row"""
    assert CS.NOT_COVERED == {}
