"""CPU-only: (1) gf_tile_record_encode_batch_elems[_dev] and gf_tile_record_max_bytes_elems reject what the host can check before a
context or a device is looked at; (2) the input builder of the GPU tests (tests/records_enc_inputs.py) returns batches in which,
by the oracle alone, every situation the record-write kernels must handle occurs."""
import ctypes as C

import numpy as np

import records_enc_inputs as R
from gridfour_amd import _lib
from gridfour_amd.codec import _ELEM_SPEC

INT, SHORT, FLOAT, ICF = 0, 1, 2, 3
HC = np.array([R.HUFFMAN, R.CANON], np.int32)


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _specs(*types, scale=1.0, fill_i=0):
    s = np.zeros(len(types), _ELEM_SPEC)
    s["type"] = types
    s["scale"] = scale
    s["fill_i"] = fill_i
    return s


def _buffers():
    # host memory standing in for device memory, and for a context: the argument checks must come before either is touched
    fake = C.create_string_buffer(8192)
    return dict(ctx=C.cast(fake, C.c_void_p), keep=fake, blob=np.zeros(4096, np.uint8), off=np.zeros(3, np.uint64),
                idx=np.zeros(2, np.int32), val=np.zeros((16, 2 * 16), np.int32), st=np.zeros(2, np.int32), used=np.zeros(34, np.uint8))


def _call(L, b, dev, ctx="ctx", codecs=HC, n_codecs=None, specs=None, n_elems=None, rows=4, cols=4, n=2, idx="idx", values="val",
          null_value=None, blob="blob", off="off", st="st", blob_shift=0, value_shift=0):
    g = lambda k: None if k is None else (b[k] if k == "ctx" else _p(b[k]))
    specs = _specs(INT, SHORT) if specs is None else specs
    n_elems = len(specs) if n_elems is None and specs is not False else n_elems
    n_codecs = (0 if codecs is None else len(codecs)) if n_codecs is None else n_codecs
    ptrs = (C.c_void_p * 17)(*[b["val"][e % 16].ctypes.data + value_shift for e in range(17)])
    if null_value is not None:
        ptrs[null_value] = None
    pv = None if values is None else ptrs
    ps = None if specs is False else _p(specs)
    pb = g(blob)
    if pb is not None and blob_shift:
        pb = C.c_void_p(pb.value + blob_shift)
    pc = None if codecs is None else _p(codecs)
    if dev:
        return L.gf_tile_record_encode_batch_elems_dev(g(ctx), None, pc, n_codecs, ps, n_elems, rows, cols, n, g(idx), pv, 1, pb,
                                                       b["blob"].size - 8, g(off), _p(b["used"]), g(st))
    return L.gf_tile_record_encode_batch_elems(g(ctx), pc, n_codecs, ps, n_elems, rows, cols, n, g(idx), pv, 1, pb, b["blob"].size - 8,
                                               g(off), _p(b["used"]))


def test_argument_checks_come_before_the_device():
    L = _lib.lib()
    b = _buffers()
    nine = np.array([1, 9, 0, 3], np.int32)
    many = np.ones(256, np.int32)
    for dev in (True, False):
        for null in ("ctx", "idx", "blob", "off") + (("st",) if dev else ()):
            assert _call(L, b, dev, **{null: None}) == _lib.ERR_ARG, (dev, null)
        assert _call(L, b, dev, values=None) == _lib.ERR_ARG
        assert _call(L, b, dev, null_value=1) == _lib.ERR_ARG                          # one of the n_elems value pointers
        assert _call(L, b, dev, specs=False, n_elems=2) == _lib.ERR_ARG                # elems == NULL
        assert _call(L, b, dev, codecs=None, n_codecs=2) == _lib.ERR_ARG
        assert _call(L, b, dev, n_elems=0) == _lib.ERR_ARG
        assert _call(L, b, dev, n_elems=-1) == _lib.ERR_ARG
        assert _call(L, b, dev, specs=_specs(*([INT] * 17))) == _lib.ERR_ARG           # > GF_MAX_ELEMS
        assert _call(L, b, dev, specs=_specs(INT, 4)) == _lib.ERR_ARG
        assert _call(L, b, dev, specs=_specs(-1)) == _lib.ERR_ARG
        assert _call(L, b, dev, specs=_specs(INT, ICF, scale=0.0)) == _lib.ERR_ARG
        assert _call(L, b, dev, specs=_specs(ICF, scale=np.nan)) == _lib.ERR_ARG
        assert _call(L, b, dev, specs=_specs(INT, SHORT, fill_i=40000)) == _lib.ERR_ARG   # a SHORT's fill outside int16
        assert _call(L, b, dev, specs=_specs(SHORT, fill_i=-32769)) == _lib.ERR_ARG
        assert _call(L, b, dev, codecs=nine) == _lib.ERR_ARG
        assert _call(L, b, dev, codecs=many, n_codecs=256) == _lib.ERR_ARG
        assert _call(L, b, dev, rows=0) == _lib.ERR_ARG
        assert _call(L, b, dev, cols=0) == _lib.ERR_ARG
    for shift in (1, 2, 4, 7):
        assert _call(L, b, True, blob_shift=shift) == _lib.ERR_ARG                     # d_blob is 8-byte aligned
    assert _call(L, b, True, value_shift=2) == _lib.ERR_ARG                            # d_values[e] is 4-byte aligned
    assert (b["st"] == 0).all() and (b["blob"] == 0).all() and (b["off"] == 0).all() and (b["used"] == 0).all()
    assert L.gf_tile_record_max_bytes_elems(None, 1, 4, 4) == 0
    assert L.gf_tile_record_max_bytes_elems(_p(_specs(INT)), 17, 4, 4) == 0


def test_unsupported_lists_and_counts_are_decided_from_the_arguments():
    L = _lib.lib()
    b = _buffers()
    arr = lambda *c: np.array(c, np.int32)
    # the device form: CodecDeflate, LSOP12 (its Deflate alternative), CodecFloat at work
    assert _call(L, b, True, codecs=arr(R.HUFFMAN, R.DEFLATE)) == _lib.ERR_UNSUPPORTED
    assert _call(L, b, True, codecs=arr(R.LSOP, R.CANON)) == _lib.ERR_UNSUPPORTED
    assert _call(L, b, True, codecs=arr(R.HUFFMAN, R.NONE), specs=_specs(INT, FLOAT)) == _lib.ERR_UNSUPPORTED
    assert _call(L, b, True, codecs=arr(R.HUFFMAN, R.DEFLATE), specs=_specs(INT, 7)) == _lib.ERR_ARG      # the argument checks come first
    for dev in (True, False):
        assert _call(L, b, dev, specs=_specs(INT), n=2**31) == _lib.ERR_UNSUPPORTED
        assert _call(L, b, dev, specs=_specs(*([SHORT] * 16)), n=2**27) == _lib.ERR_UNSUPPORTED
        assert _call(L, b, dev, specs=_specs(INT, 7), n=2**31) == _lib.ERR_ARG
        assert _call(L, b, dev, rows=2**14, cols=2**14) == _lib.ERR_UNSUPPORTED           # 2^28 cells in a tile
    assert (b["st"] == 0).all() and (b["blob"] == 0).all() and (b["off"] == 0).all()


def test_empty_batch_is_ok_and_valid_arguments_need_a_device():
    L = _lib.lib()
    b = _buffers()
    for dev in (True, False):
        assert _call(L, b, dev, n=0) == _lib.OK
        assert _call(L, b, dev, n=0, codecs=None) == _lib.OK                          # compression disabled
        assert _call(L, b, dev, n=0, specs=_specs(*([ICF] * 16))) == _lib.OK
    if L.gf_device_count() > 0:
        return
    lens = np.array([64, 64], np.uint32)
    off = np.array([0, 64, 128], np.uint64)
    want = L.gf_huffman_decode_batch_i32_dev(b["ctx"], None, 4, 4, 2, _p(b["blob"]), b["blob"].size, _p(off), 0, _p(lens), _p(b["val"]),
                                             _p(b["st"]))
    assert want < 0
    for dev in (True, False):
        assert _call(L, b, dev) == want


def test_max_bytes():
    L = _lib.lib()
    # Sample08: short + float at 5 x 5 -- 4 + (4 + 52) + (4 + 100) + 12 = 176
    assert L.gf_tile_record_max_bytes_elems(_p(_specs(SHORT, FLOAT)), 2, 5, 5) == 176
    for t in (INT, SHORT):
        assert L.gf_tile_record_max_bytes_elems(_p(_specs(t)), 1, 7, 9) == L.gf_tile_record_max_bytes(t, 7, 9)


# ---------------------------------------------------------------- the input builder of the GPU tests

def _walk(batch, codecs):
    """per record: (padding bytes, start of element 1 in the record or None, per-element (index used, why, tie))"""
    plan = batch.plan(codecs)
    out = []
    for t in range(batch.nt):
        lens = [len(plan[e][t][0]) for e in range(len(batch.elems))]
        content = 4 + sum(4 + n for n in lens)
        size = (content + 12 + 7) // 8 * 8
        pad = size - 4 - (12 + sum(4 + n for n in lens))
        start1 = 12 + 4 + lens[0] + 4 if len(lens) > 1 else None                      # element 1's first byte
        out.append((pad, start1, [plan[e][t][1:] for e in range(len(batch.elems))]))
    return out


def test_builder_batches_hold_every_situation():
    codecs = (R.HUFFMAN, R.CANON)
    pads, res4, res16, winners, whys, mixed = set(), set(), set(), set(), set(), 0
    for name in ("three", "short"):
        for shape in R.SHAPES:
            batch = R.pool(name, *shape).head(65)
            for pad, start1, per_elem in _walk(batch, codecs):
                pads.add(pad)
                if start1 is not None:
                    res4.add(start1 % 4)
                    res16.add(start1 % 16)
                winners |= {u for u, _, _ in per_elem if u != 255}
                whys |= {w for _, w, _ in per_elem}
                packed = {u != 255 for el, (u, _, _) in zip(batch.elems, per_elem) if R.kind_of(el) != "float"}
                mixed += packed == {True, False}
    assert pads == set(range(8)), pads                                   # every padding amount
    assert res4 == {0, 1, 2, 3} and len(res16) >= 12, (res4, res16)      # element 1 starts at any byte
    assert winners == {0, 1}                                             # each listed codec wins
    assert {"packed", "not shorter", "declined", "no codec"} <= whys      # noise; the all-null tile; the float element
    assert mixed >= 1                                                    # a record with a packed and a standard-form integer element


def test_builder_has_a_tie_decided_by_list_order():
    """7 x 9: both codecs pack some tiles to the same length; the earlier list entry wins, so the two orders of the list differ"""
    batch = R.pool("int", 7, 9).head(65)
    ties = [t for t, row in enumerate(batch.plan((R.HUFFMAN, R.CANON))[0]) if row[2] == "packed" and row[3]]
    assert ties, "no tie among the first 65 tiles"
    fwd = batch.plan((R.HUFFMAN, R.CANON))[0]
    rev = batch.plan((R.CANON, R.HUFFMAN))[0]
    for t in ties:
        assert fwd[t][1] == 0 and rev[t][1] == 0 and fwd[t][0][0] == 0 and rev[t][0][0] == 0
        assert len(fwd[t][0]) == len(rev[t][0]) and fwd[t][0][1:] != rev[t][0][1:]      # two different codecs' bytes


def test_expected_records_parse_back():
    """the expected records are well-formed by the walker the read-side tests use: sizes, type, lengths, CRC"""
    import struct
    from test_gpu_records_dev import _crc
    batch = R.pool("three", 7, 9).head(8)
    records, used = batch.expected((R.CANON, R.HUFFMAN))
    assert used.shape == (3, 8) and (used[2] == 255).all()
    for t, r in enumerate(records):
        size, rtype, index = struct.unpack_from("<iB3xi", r, 0)
        assert size == len(r) and size % 8 == 0 and rtype == 2 and index == int(batch.indices[t])
        pos = 12
        for e in range(3):
            (n,) = struct.unpack_from("<i", r, pos)
            assert n <= R.std_size(batch.elems[e], 63)
            pos += 4 + n
        assert 0 <= size - 4 - pos < 8 and r[pos:size - 4] == b"\0" * (size - 4 - pos)
        assert struct.unpack_from("<I", r, size - 4)[0] == _crc(r[:size - 4])
    assert R.std_size("short", 63) == 128 and len(R.standard_form("short", batch.values[0][0])) == 128
