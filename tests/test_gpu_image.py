"""ARGB images on the GPU (gf_image_split / _join / _reduce / _write / _read and their _dev forms): every word, every plane item,
every record byte and every status against the numpy model of tests/image_ref.py (the records: tests/block_write_ref.py on the
model's planes with the oracle's encoders behind it), BIT FOR BIT, at the smallest shapes at which the kernels can still go wrong.
Every output lies between guard bands of 0xA5 bytes that must survive, and is pre-filled with 0xA5 itself."""
import ctypes as C

import numpy as np
import pytest

import block_write_ref as W
import caller_stream as CS
import image_cases as K
import image_ref as M
import records_enc_inputs as RI
from test_gpu_records_dev import _flip, ctx      # noqa: F401  (ctx: fixture)

pytestmark = pytest.mark.gpu
KINDS = [(m, t) for m in M.MODELS for t in (M.INT, M.SHORT)]
KIND_IDS = ["%s-%s" % (("rgb", "ycocg")[m], ("int", "short")[t]) for m, t in KINDS]
ERR_FORMAT = -1


class Held:
    """nbytes of output in device memory, `shift` bytes behind a 256-byte boundary, everything around it 0xA5"""

    def __init__(self, ctx, nbytes, shift=0):
        self.nbytes, self.shift = int(nbytes), shift
        self.g = CS.Guarded(ctx, self.nbytes + 16)

    @property
    def ptr(self):
        return C.c_void_p(self.g.ptr.value + self.shift)

    def get(self, dtype, stream=None):
        raw = self.g.get(stream)
        assert (raw[:self.shift] == CS.FILL).all() and (raw[self.shift + self.nbytes:] == CS.FILL).all(), "bytes beside the output overwritten"
        return raw[self.shift:self.shift + self.nbytes].copy().view(dtype)

    def untouched(self, stream=None):
        return (self.get(np.uint8, stream) == CS.FILL).all()

    def free(self):
        self.g.free()


class Inp:
    """an array in device memory, `shift` bytes behind a 256-byte boundary"""

    def __init__(self, ctx, values, shift=0):
        import gridfour_amd
        self.values, self.shift = np.ascontiguousarray(values), shift
        self.buf = gridfour_amd.DeviceBuffer(ctx, self.values.nbytes + shift + 32)
        self.put(self.values)

    def put(self, values):
        self.values = np.ascontiguousarray(values)
        if self.values.size:
            self.buf.upload(self.values, self.shift)

    @property
    def ptr(self):
        return C.c_void_p(self.buf.ptr.value + self.shift)

    def unchanged(self):
        v = self.values
        return v.size == 0 or np.array_equal(self.buf.download(np.uint8, v.nbytes, self.shift), v.reshape(-1).view(np.uint8))

    def free(self):
        self.buf.free()


def _shifts(elem_type, c):
    """byte shifts of the words and of the three planes of combination c: the words at 0, 4, 8, 12 of a 16-byte line; c < 4: the
    first plane in the words' phase (its vectors line up with the quads), the other two out of it; c >= 4: all three in phase"""
    ws = 4 * (c % 4)
    item, line = (2, 8) if elem_type == M.SHORT else (4, 16)
    same = ws // 2 if elem_type == M.SHORT else ws
    return ws, [same] * 3 if c >= 4 else [(same + item * k) % line for k in range(3)]


def _combos(n):
    return (1, 4) if n > 100000 else range(6)


def _fill(elem_type):
    return -32768 if elem_type == M.SHORT else M.INT_MIN


@pytest.mark.parametrize("model,elem_type", KINDS, ids=KIND_IDS)
def test_split(ctx, model, elem_type):
    rng = np.random.default_rng(100 + 2 * model + elem_type)
    dt = M.plane_dtype(elem_type)
    for n in K.COUNTS:
        for c in _combos(n):
            ws, ps = _shifts(elem_type, c)
            w = K.random_words(rng, n)
            src = Inp(ctx, w, ws)
            outs = [Held(ctx, n * dt().itemsize, s) for s in ps]
            try:
                ctx.image_split_dev(model, elem_type, n, src.ptr, [o.ptr for o in outs])
                ctx.synchronize()
                for k, want in enumerate(M.split(model, w)):
                    assert np.array_equal(outs[k].get(dt), want.astype(dt)), (n, c, k)
                assert src.unchanged()
            finally:
                for b in [src] + outs:
                    b.free()


@pytest.mark.parametrize("model,elem_type", KINDS, ids=KIND_IDS)
def test_join(ctx, model, elem_type):
    rng = np.random.default_rng(200 + 2 * model + elem_type)
    for n in K.COUNTS:
        for c in _combos(n):
            ws, ps = _shifts(elem_type, c)
            planes = K.join_planes(rng, n, _fill(elem_type) if c % 2 else 12345, elem_type)
            srcs = [Inp(ctx, p, s) for p, s in zip(planes, ps)]
            out = Held(ctx, n * 4, ws)
            try:
                ctx.image_join_dev(model, elem_type, n, [s.ptr for s in srcs], out.ptr)
                ctx.synchronize()
                assert np.array_equal(out.get(np.int32), M.join(model, planes)), (n, c)
                assert all(s.unchanged() for s in srcs)
            finally:
                for b in srcs + [out]:
                    b.free()


def test_join_of_int_min_planes(ctx):
    """three planes of INT_MIN, what a missing tile under fill INT_MIN reads as: 0xff000000 in both models (worked out by hand in
    include/gvrs_hip_codec.h)"""
    n = 77
    srcs = [Inp(ctx, np.full(n, M.INT_MIN, np.int32)) for _ in range(3)]
    out = Held(ctx, n * 4)
    try:
        for model in M.MODELS:
            ctx.image_join_dev(model, M.INT, n, [s.ptr for s in srcs], out.ptr)
            ctx.synchronize()
            assert (out.get(np.uint32) == 0xff000000).all()
    finally:
        for b in srcs + [out]:
            b.free()


def test_host_forms_of_split_and_join(ctx):
    rng = np.random.default_rng(300)
    w = K.random_words(rng, 3 * 1025).reshape(3, 1025)
    for model, elem_type in KINDS:
        planes = ctx.image_split(w, model, elem_type)
        assert all(p.shape == w.shape and p.dtype == M.plane_dtype(elem_type) for p in planes)
        assert all(np.array_equal(p, q.astype(p.dtype)) for p, q in zip(planes, M.split(model, w)))
        assert np.array_equal(ctx.image_join(planes, model, elem_type).view(np.uint32), w | np.uint32(0xff000000))
        any_ints = K.join_planes(rng, 999, _fill(elem_type), elem_type)
        assert np.array_equal(ctx.image_join(any_ints, model, elem_type), M.join(model, any_ints))


def _reduce_dev(ctx, img, f, shift=0):
    """the reduced image through gf_image_reduce_dev, the input `shift` bytes behind a 256-byte boundary"""
    w, h = ctx.image_reduce_size(img.shape[1], img.shape[0], f)
    src = Inp(ctx, img, shift)
    out = Held(ctx, w * h * 4)
    try:
        ctx.image_reduce_dev(img.shape[1], img.shape[0], f, src.ptr, out.ptr)
        ctx.synchronize()
        assert src.unchanged()
        return out.get(np.int32).reshape(h, w)
    finally:
        src.free(), out.free()


@pytest.mark.parametrize("f", K.REDUCE_FACTORS)
def test_reduce(ctx, f):
    """both data paths (a lane per output word up to f = 8, strips through LDS above), more than one workgroup per output row,
    partial rows and columns, windows at the rounding boundary, random alpha; a pitch and a base that allow one load per window
    row (f = 2, 4) and ones that do not"""
    rng = np.random.default_rng(400 + f)
    n_cols = 300 if f <= 16 else 70                      # f = 60: 68 output words a workgroup
    img = K.boundary_image(f, 3, n_cols, rng)
    want = M.reduce(img, f)
    assert want.shape == (3, n_cols)
    assert np.array_equal(_reduce_dev(ctx, img, f), want)                           # (a pitch of n_cols * f + f - 1 words)
    even = np.ascontiguousarray(img[:, :n_cols * f])
    assert np.array_equal(_reduce_dev(ctx, even, f), want)
    assert np.array_equal(_reduce_dev(ctx, even, f, shift=4), want)
    assert np.array_equal(ctx.image_reduce(img, f), want)                           # the host form
    white = np.full((2 * f + 1, 5 * f + 2), 0x00ffffff, np.uint32)
    assert (_reduce_dev(ctx, white, f).view(np.uint32) == 0xffffffff).all()


def test_reduce_of_nothing(ctx):
    """width < f or height < f: GF_OK and nothing written"""
    src = Inp(ctx, np.zeros((5, 9), np.uint32))
    out = Held(ctx, 64)
    try:
        for width, height, f in ((9, 5, 6), (5, 9, 6), (9, 5, 10), (1, 1, 2)):
            assert ctx.image_reduce_size(width, height, f)[0] * ctx.image_reduce_size(width, height, f)[1] == 0
            ctx.image_reduce_dev(width, height, f, src.ptr, out.ptr)
        ctx.synchronize()
        assert out.untouched()
        ctx.image_split_dev(M.RGB, M.INT, 0, src.ptr, [out.ptr] * 3)
        ctx.image_join_dev(M.RGB, M.SHORT, 0, [src.ptr] * 3, out.ptr)
        ctx.synchronize()
        assert out.untouched()
    finally:
        src.free(), out.free()


def test_reduce_by_the_largest_factor(ctx):
    """f = 2899, the largest the call takes: a window row no longer shares the LDS stage with another (one output word a workgroup,
    one source row a stage), two workgroups, a partial row and column.  A window wider than the stage itself would need f > 4096,
    which gf_image_reduce refuses.  About 67 MB of words: the one large case."""
    f = M.MAX_FACTOR
    rng = np.random.default_rng(500)
    img = K.random_words(rng, (f + 2) * (2 * f + 3)).reshape(f + 2, 2 * f + 3)
    img[:f, :f] |= np.uint32(0x00ffffff)                                            # the first window: every sum at its largest
    want = M.reduce(img, f)
    assert want.shape == (1, 2) and want.view(np.uint32)[0, 0] == 0xffffffff
    assert np.array_equal(_reduce_dev(ctx, img, f), want)


# ---- the record forms ----
GRID, TILE = (100, 200), (30, 40)                      # the last tile row and column overhang
RECTS = {"whole": (0, 0, 100, 200), "interior": (17, 33, 50, 101), "cell": (45, 87, 1, 1)}
LISTS = ((), (RI.HUFFMAN, RI.CANON))


def _picture(rng, shape):
    """a smooth picture with a little noise and random alpha: its planes pack"""
    r, c = np.mgrid[0:shape[0], 0:shape[1]]
    ch = [np.clip((a * r + b * c) // 3 + rng.integers(0, 3, shape), 0, 255).astype(np.uint32) for a, b in ((2, 1), (1, 3), (3, 2))]
    return (rng.integers(0, 256, shape).astype(np.uint32) << 24) | ch[0] << 16 | ch[1] << 8 | ch[2]


def _elems(elem_type):
    name = "short" if elem_type == M.SHORT else "int"
    rng = (-32768, 32767) if elem_type == M.SHORT else (M.INT_MIN, M.INT_MAX)
    return [name] * 3, [_fill(elem_type)] * 3, [rng] * 3


def _encoder(elems, codecs, crc):
    """the reference-pinned record writer of tests/records_enc_inputs.py on the tiles handed to it"""
    def encode(indices, tiles):
        b = RI.Batch.__new__(RI.Batch)
        b.elems, b.nr, b.nc, b.nt = elems, TILE[0], TILE[1], len(indices)
        b.values, b.indices, b._cand = [np.ascontiguousarray(t) for t in tiles], np.asarray(indices, np.int32), {}
        recs, used = b.expected(codecs, crc=crc)
        return recs, used, np.zeros(len(indices), np.int32)
    return encode


def _master(ctx, codecs):
    import gridfour_amd
    return gridfour_amd.CodecMasterHip(codec_list=list(codecs), context=ctx)


def _planes(model, elem_type, pic):
    return [p.astype(M.plane_dtype(elem_type)) for p in M.split(model, pic)]


def _same_write(got, want, what):
    idx, records, used, status = got
    w_idx, w_records, _, w_used, w_status = want
    assert np.array_equal(status, w_status), (what, status.tolist(), w_status.tolist())
    assert np.array_equal(idx, w_idx) and np.array_equal(used, w_used), what
    assert records == w_records, what


@pytest.mark.parametrize("model,elem_type", KINDS, ids=KIND_IDS)
def test_write_dev(ctx, model, elem_type):
    """n_old == 0: the records byte for byte the model's, and byte for byte what gf_block_write_elems_dev writes for the model's
    planes; the blob behind the last record untouched"""
    elems, fills, ranges = _elems(elem_type)
    rng = np.random.default_rng(600 + 2 * model + elem_type)
    for name, rect in RECTS.items():
        pic = _picture(rng, rect[2:])
        planes = _planes(model, elem_type, pic)
        for codecs in LISTS:
            master = _master(ctx, codecs)
            for crc in (True, False):
                want = W.expected(_encoder(elems, codecs, crc), GRID, TILE, rect, planes, elems, fills, ranges)
                assert (want[4] == 0).all()
                got = master.image_write_dev(TILE[0], TILE[1], GRID, rect, pic, model, elem_type, fills[0], checksums=crc)
                _same_write(got, want, (name, codecs, crc))
                other = master.write_block_dev(TILE[0], TILE[1], GRID, rect, planes, elems, fills, ranges, checksums=crc)
                assert got[1] == other[1] and all(np.array_equal(a, b) for a, b in zip((got[0], got[2], got[3]), (other[0], other[2], other[3])))
            idx, blob, offsets, used, status = master.image_write_dev(TILE[0], TILE[1], GRID, rect, pic, model, elem_type, fills[0], raw=True)
            assert (blob[int(offsets[-1]):] == 0xA5).all(), name


@pytest.mark.parametrize("model,elem_type", KINDS, ids=KIND_IDS)
def test_write_dev_over_old_records(ctx, model, elem_type):
    """a second picture written into the interior rectangle over the records of a first: the partly covered tiles keep the old
    cells outside the rectangle"""
    elems, fills, ranges = _elems(elem_type)
    rng = np.random.default_rng(700 + 2 * model + elem_type)
    codecs = LISTS[1]
    master = _master(ctx, codecs)
    first, second = _picture(rng, GRID), _picture(rng, RECTS["interior"][2:])
    old_idx, old_tiles, _ = W.cut(GRID, TILE, RECTS["whole"], _planes(model, elem_type, first), elems, fills, ranges)
    _, old_records, _, old_status = master.image_write_dev(TILE[0], TILE[1], GRID, RECTS["whole"], first, model, elem_type, fills[0])
    assert (old_status == 0).all()
    order = rng.permutation(len(old_records))
    old = _blob([old_records[i] for i in order])
    before = {int(i): [t[j] for t in old_tiles] for j, i in enumerate(old_idx)}
    planes = _planes(model, elem_type, second)
    for crc in (True, False):
        want = W.expected(_encoder(elems, codecs, crc), GRID, TILE, RECTS["interior"], planes, elems, fills, ranges, before=before)
        got = master.image_write_dev(TILE[0], TILE[1], GRID, RECTS["interior"], second, model, elem_type, fills[0], old=old, checksums=crc)
        _same_write(got, want, crc)
        other = master.write_block_dev(TILE[0], TILE[1], GRID, RECTS["interior"], planes, elems, fills, ranges, old=old, checksums=crc)
        assert got[1] == other[1] and np.array_equal(got[3], other[3])
    fresh = W.expected(_encoder(elems, codecs, crc), GRID, TILE, RECTS["interior"], planes, elems, fills, ranges)
    assert fresh[1] != want[1]                                                      # (the old cells made a difference)


def _blob(records):
    offsets = np.zeros(len(records) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(r) for r in records])
    return np.frombuffer(b"".join(records) + b"\0" * 16, np.uint8), offsets


@pytest.mark.parametrize("model,elem_type", KINDS, ids=KIND_IDS)
def test_read_dev(ctx, model, elem_type):
    """the records just written read back into words; a record list with a tile missing; a record with a flipped payload byte"""
    elems, fills, ranges = _elems(elem_type)
    rng = np.random.default_rng(800 + 2 * model + elem_type)
    pic = _picture(rng, GRID)
    shown = (pic | np.uint32(0xff000000)).view(np.int32)
    gone = M.join(model, [np.array([f], np.int32) for f in fills])[0]              # what three fills join to
    if elem_type == M.INT:
        assert gone.view(np.uint32) == 0xff000000
    for codecs in LISTS:
        master = _master(ctx, codecs)
        idx, records, _, status = master.image_write_dev(TILE[0], TILE[1], GRID, RECTS["whole"], pic, model, elem_type, fills[0])
        assert (status == 0).all() and len(records) == 20
        blob, offsets = _blob(records)
        for rect in RECTS.values():
            argb, st = master.image_read_dev(TILE[0], TILE[1], GRID, rect, blob, offsets, model, elem_type, fills[0])
            assert np.array_equal(st, np.zeros((3, 20), np.int32))
            assert np.array_equal(argb, shown[rect[0]:rect[0] + rect[2], rect[1]:rect[1] + rect[3]]), (codecs, rect)
        # tile 7 (tile row 1, tile column 2) is not in the list
        kept = [r for i, r in zip(idx, records) if i != 7]
        argb, st = master.image_read_dev(TILE[0], TILE[1], GRID, RECTS["whole"], *_blob(kept), model, elem_type, fills[0])
        want = shown.copy()
        want[30:60, 80:120] = gone
        assert np.array_equal(st, np.zeros((3, 19), np.int32)) and np.array_equal(argb, want), codecs
        # record 3 (tile 3: tile row 0, tile column 3) with a flipped payload byte: the checksum notices, all three elements fail
        hurt = list(records)
        hurt[3] = _flip(hurt[3], len(hurt[3]) // 2, 5)
        argb, st = master.image_read_dev(TILE[0], TILE[1], GRID, RECTS["whole"], *_blob(hurt), model, elem_type, fills[0])
        want_st = np.zeros((3, 20), np.int32)
        want_st[:, 3] = ERR_FORMAT
        want = shown.copy()
        want[0:30, 120:160] = gone
        assert idx[3] == 3 and np.array_equal(st, want_st) and np.array_equal(argb, want), codecs


@pytest.mark.parametrize("model,elem_type", KINDS, ids=KIND_IDS)
def test_host_record_forms(ctx, model, elem_type):
    """gf_image_write / gf_image_read: with the lists of the device form, the model's records; with the standard list (CodecDeflate
    has no model here) what gf_block_write_elems writes for the model's planes, and the picture back"""
    import gridfour_amd
    elems, fills, ranges = _elems(elem_type)
    rng = np.random.default_rng(900 + 2 * model + elem_type)
    rect = RECTS["interior"]
    pic = _picture(rng, rect[2:])
    planes = _planes(model, elem_type, pic)
    for codecs in LISTS:
        master = _master(ctx, codecs)
        want = W.expected(_encoder(elems, codecs, True), GRID, TILE, rect, planes, elems, fills, ranges)
        _same_write(master.image_write(TILE[0], TILE[1], GRID, rect, pic, model, elem_type, fills[0]), want, codecs)
    master = _master(ctx, gridfour_amd.STANDARD_CODEC_LIST)
    assert tuple(int(c) for c in master.codecs) == (1, 2, 0, 3)
    got = master.image_write(TILE[0], TILE[1], GRID, rect, pic, model, elem_type, fills[0])
    other = master.write_block(TILE[0], TILE[1], GRID, rect, planes, elems, fills, ranges)
    assert (got[3] == 0).all() and got[1] == other[1] and all(np.array_equal(a, b) for a, b in zip((got[0], got[2], got[3]), (other[0], other[2], other[3])))
    argb, st = master.image_read(TILE[0], TILE[1], GRID, rect, *_blob(got[1]), model, elem_type, fills[0])
    assert not st.any() and np.array_equal(argb, (pic | np.uint32(0xff000000)).view(np.int32))


def test_capture_on_the_contexts_stream(ctx):
    """after one warm-up call, split -> join -> reduce captured on gf_context_stream(ctx): nothing runs during the capture (the
    outputs are still 0xA5), and the replay on a second input gives the model's words"""
    rng = np.random.default_rng(1000)
    h, w, f = 37, 1031, 3
    first, second = K.random_words(rng, h * w).reshape(h, w), K.random_words(rng, h * w).reshape(h, w)
    src = Inp(ctx, first)
    planes = [Held(ctx, h * w * 2) for _ in range(3)]
    words = Held(ctx, h * w * 4)
    small = Held(ctx, (h // f) * (w // f) * 4)
    outs = planes + [words, small]
    stream = CS.Stream(ctx.stream)

    def chain():
        ctx.image_split_dev(M.YCOCG, M.SHORT, h * w, src.ptr, [p.ptr for p in planes])
        ctx.image_join_dev(M.YCOCG, M.SHORT, h * w, [p.ptr for p in planes], words.ptr)
        ctx.image_reduce_dev(w, h, f, words.ptr, small.ptr)

    try:
        chain()                                                                     # the warm-up
        ctx.synchronize()
        for o in outs:
            o.g.refill()
        _, gexec = stream.capture(chain)
        stream.synchronize()
        assert all(o.untouched() for o in outs)
        src.put(second)
        stream.launch(gexec)
        stream.synchronize()
        for k, want in enumerate(M.split(M.YCOCG, second)):
            assert np.array_equal(planes[k].get(np.int16), want.astype(np.int16).reshape(-1)), k
        full = (second | np.uint32(0xff000000)).view(np.int32)
        assert np.array_equal(words.get(np.int32).reshape(h, w), full)
        assert np.array_equal(small.get(np.int32).reshape(h // f, w // f), M.reduce(full, f))
    finally:
        stream.close()
        for b in [src] + outs:
            b.free()
