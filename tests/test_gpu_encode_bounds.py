"""Where the encoders write.  Every packer path of the slot-writing encoders (gf_huffman_*, gf_canon_*, gf_lsop12_*, gf_lsop08_*,
gf_m32_encode_batch_i32_dev) gets packings of S - 3 .. S + 1 bytes around its slot stride S (tests/slot_edges.py; the CPU test
tests/test_slot_edges_oracle.py proves that every family reaches them), in a slot array that lies inside a larger allocation filled
with a sentinel byte: lengths, predictors and statuses are the oracle's, a packing that fits is the oracle's byte for byte, a tile
reported GF_OVERFLOW or GF_DECLINED leaves its whole slot untouched (the contract of include/gvrs_hip_codec.h), and nothing outside
the slot array is written (LSOP08: nor outside the caller's residuals, coefficient records and scratch statuses).  Then gf_compact_dev on what the encoders leave behind -- tiles with d_lengths[t] > slot_stride take no
room -- on hand-made slots at every alignment and at blob_cap's edges, and the out_cap / blob_cap rule of the host-memory encoders.

No test here depends on an access outside an allocation: guards are sized from the oracle's lengths before any kernel runs."""
import ctypes as C

import numpy as np
import pytest

import lsop08_ref
import oracle
import route_plan as rp
import slot_edges as se
from slot_edges import DECLINED, OK, SENTINEL

pytestmark = pytest.mark.gpu
META_GUARD = 64
LSOP = ("lsop", "lsop08")
ERR_CAPACITY = -3


def _ctx():
    import gridfour_amd
    return gridfour_amd.GvrsHipContext(0)


class Guarded:
    """[guard | shift | payload | guard] in one device allocation, every byte the sentinel; ptr = the payload (16-byte aligned
    for shift 0: allocations are, and the guards are multiples of 16)"""

    def __init__(self, ctx, nbytes, guard, shift=0):
        from gridfour_amd import DeviceBuffer
        assert guard % 16 == 0
        self.nbytes, self.guard, self.off = int(nbytes), guard, guard + shift
        self.buf = DeviceBuffer(ctx, self.off + self.nbytes + guard)
        assert self.buf.ptr.value % 16 == 0
        self.buf.fill(SENTINEL)
        self.ptr = C.c_void_p(self.buf.ptr.value + self.off)

    def upload(self, a):
        a = np.ascontiguousarray(a)
        assert a.nbytes <= self.nbytes
        self.buf.upload(a, self.off)
        return self

    def download(self, dtype=np.uint8):
        """(payload as dtype, guards intact)"""
        raw = self.buf.download(np.uint8, self.buf.nbytes)
        intact = bool((raw[:self.off] == SENTINEL).all() and (raw[self.off + self.nbytes:] == SENTINEL).all())
        return raw[self.off:self.off + self.nbytes].view(dtype), intact

    def free(self):
        self.buf.free()


class Encoded:
    pass


def _encode(ctx, f, tiles=None, index=None):
    """one encode call of family f (or of `tiles`, rows of f's tiles picked by `index`) with slot_stride = f.stride into guarded
    buffers; returns the device buffers and their downloads"""
    from gridfour_amd import DeviceBuffer, lib
    from gridfour_amd._lib import check
    L = lib()
    index = list(range(f.n)) if index is None else list(index)
    vals = f.values() if tiles is None else tiles
    nt, S, sub = len(index), f.stride, 3 if f.codec == "m32" else 1
    e = Encoded()
    e.index, e.nt = index, nt
    e.values = DeviceBuffer(ctx, vals.nbytes).upload(vals)
    e.slots = Guarded(ctx, nt * sub * S, f.guard())
    e.lengths = Guarded(ctx, nt * sub * 4, META_GUARD)
    e.preds = Guarded(ctx, nt * sub, META_GUARD) if f.codec not in LSOP else None   # (the LSOP encoders report no predictor)
    e.work_ok = True
    e.status = Guarded(ctx, nt * 4, META_GUARD)
    ctx.reserve(f.nr, f.nc, nt)
    if f.codec in ("huffman", "canon"):
        fn = getattr(L, "gf_%s_encode_batch_i32_dev" % f.codec)
        check(fn(ctx.handle, None, 0, f.nr, f.nc, nt, e.values.ptr, e.slots.ptr, S, e.lengths.ptr, e.preds.ptr, e.status.ptr, f.mask),
              "encode")
    elif f.codec == "lsop":
        n = int(L.gf_lsop12_residual_count(f.nr, f.nc))
        e.res_stride = (n + 3) // 4 * 4
        e.residuals, e.coefs = DeviceBuffer(ctx, nt * e.res_stride * 4 + 16), DeviceBuffer(ctx, nt * 64)
        e.scratch = DeviceBuffer(ctx, nt * 4)
        if f.lsop_flags:
            check(L.gf_lsop12_encode_batch_i32_dev_ex(ctx.handle, None, 0, f.nr, f.nc, nt, e.values.ptr, f.lsop_flags, e.slots.ptr, S,
                                                      e.lengths.ptr, e.status.ptr, e.residuals.ptr, e.res_stride, e.coefs.ptr,
                                                      e.scratch.ptr), "lsop encode (ex)")
        else:                            # the form without flags
            check(L.gf_lsop12_encode_batch_i32_dev(ctx.handle, None, 0, f.nr, f.nc, nt, e.values.ptr, e.slots.ptr, S, e.lengths.ptr,
                                                   e.status.ptr, e.residuals.ptr, e.res_stride, e.coefs.ptr, e.scratch.ptr),
                  "lsop encode")
    elif f.codec == "lsop08":            # the caller's work buffers lie between guards too: residuals, coefficient records, statuses
        n = int(L.gf_lsop08_residual_count(f.nr, f.nc))
        e.res_stride = (n + 3) // 4 * 4
        e.residuals, e.coefs = Guarded(ctx, nt * e.res_stride * 4, META_GUARD), Guarded(ctx, nt * 64, META_GUARD)
        e.scratch = Guarded(ctx, nt * 4, META_GUARD)
        check(L.gf_lsop08_encode_batch_i32_dev(ctx.handle, 0, f.nr, f.nc, nt, e.values.ptr, e.slots.ptr, S, e.lengths.ptr, e.status.ptr,
                                               e.residuals.ptr, e.res_stride, e.coefs.ptr, e.scratch.ptr), "lsop08 encode")
        ctx.synchronize()
        e.work_ok = all(g.download()[1] for g in (e.residuals, e.coefs, e.scratch))
    else:
        e.seeds = Guarded(ctx, nt * 4, META_GUARD)
        check(L.gf_m32_encode_batch_i32_dev(ctx.handle, None, f.nr, f.nc, nt, e.values.ptr, e.slots.ptr, S, e.lengths.ptr,
                                            e.preds.ptr, e.seeds.ptr, e.status.ptr), "m32 encode")
    ctx.synchronize()
    e.h_slots, e.slots_ok = e.slots.download()
    e.h_slots = e.h_slots.reshape(nt * sub, S)
    e.h_lengths, e.lengths_ok = e.lengths.download(np.uint32)
    e.h_preds, e.preds_ok = e.preds.download() if e.preds is not None else (None, True)
    e.h_status, e.status_ok = e.status.download(np.int32)
    return e


def _check(f, e):
    """the assertions of the module's docstring on one encode call; every mismatch is collected before the test fails"""
    S, bad = f.stride, []
    if not (e.slots_ok and e.lengths_ok and e.status_ok and e.preds_ok and e.work_ok):
        bad.append(("guards", e.slots_ok, e.lengths_ok, e.preds_ok, e.status_ok, e.work_ok))
    for i, t in enumerate(e.index):
        want = f.expected_status(t)
        if e.h_status[i] != want:
            bad.append(("status", i, t, int(e.h_status[i]), want))
        if f.codec == "m32":
            for p in range(3):
                stream, slot = f.packs[t][p], e.h_slots[3 * i + p]
                if int(e.h_lengths[3 * i + p]) != f.lengths[t][p] or int(e.h_preds[3 * i + p]) != f.preds[t][p]:
                    bad.append(("length/model", i, t, p, int(e.h_lengths[3 * i + p]), f.lengths[t][p], int(e.h_preds[3 * i + p])))
                if stream is not None and len(stream) + 8 <= S:
                    if slot[:len(stream)].tobytes() != stream:
                        bad.append(("stream", i, t, p))
                    # what the packer's whole-word flushes may touch: up to 8 bytes behind the stream, never the next sub-slot
                    if not (slot[len(stream) + 8:] == SENTINEL).all():
                        bad.append(("behind the margin", i, t, p))
                elif not (slot == SENTINEL).all():
                    bad.append(("unwritten sub-slot touched", i, t, p, f.lengths[t][p]))
            continue
        if int(e.h_lengths[i]) != f.lengths[t]:
            bad.append(("length", i, t, int(e.h_lengths[i]), f.lengths[t]))
        if f.codec not in LSOP and want != DECLINED and int(e.h_preds[i]) != f.preds[t]:
            bad.append(("predictor", i, t, int(e.h_preds[i]), f.preds[t]))
        if want == OK:
            if e.h_slots[i, :f.lengths[t]].tobytes() != f.packs[t]:
                bad.append(("packing", i, t, f.lengths[t]))
        elif not (e.h_slots[i] == SENTINEL).all():
            bad.append(("slot of a tile that wrote nothing", i, t, want, f.lengths[t], int((e.h_slots[i] != SENTINEL).sum())))
    if f.codec == "m32":
        seeds, ok = e.seeds.download(np.int32)
        if not ok or [int(x) for x in seeds] != [f.seeds[t] for t in e.index]:
            bad.append(("seeds", ok))
    assert not bad, (f.name, S, len(bad), bad[:12])


def _decode(ctx, f, e):
    """the slots as the encoder left them decode to the values of every GF_OK tile (the lengths of the others set to 0 for this
    call; what the decoder says about those is not asserted)"""
    from gridfour_amd import DeviceBuffer, lib
    from gridfour_amd._lib import check
    L = lib()
    nt, S = e.nt, f.stride
    ok = np.array([f.expected_status(t) == OK for t in e.index])
    d_vals, d_st = DeviceBuffer(ctx, nt * f.cells * 4).fill(0), DeviceBuffer(ctx, nt * 4 + 16)
    if f.codec == "m32":                 # raw containers (header + the stream as the encoder wrote it) of every written candidate
        from test_gpu_inflate import _upload_packings
        import struct
        packs, want = [], []
        for i, t in enumerate(e.index):
            for p in range(3):
                n = f.lengths[t][p]
                if f.packs[t][p] is not None and n + 8 <= S:
                    packs.append(bytes([0, f.preds[t][p]]) + struct.pack("<iI", f.seeds[t], n) + e.h_slots[3 * i + p, :n].tobytes())
                    want.append(f.tiles[t])
        d_blob, d_off, d_len, total = _upload_packings(ctx, packs)
        d_vals, d_st = DeviceBuffer(ctx, len(packs) * f.cells * 4).fill(0), DeviceBuffer(ctx, len(packs) * 4 + 16)
        check(L.gf_m32_decode_batch_i32_dev(ctx.handle, None, f.nr, f.nc, len(packs), d_blob.ptr, total + 32, d_off.ptr, 0, d_len.ptr,
                                            d_vals.ptr, d_st.ptr), "m32 decode")
        ctx.synchronize()
        assert (d_st.download(np.int32, len(packs)) == 0).all()
        assert np.array_equal(d_vals.download(np.int32, len(packs) * f.cells).reshape(len(packs), f.cells), np.stack(want))
        return
    lengths = np.where(ok, e.h_lengths, 0).astype(np.uint32)
    d_len = DeviceBuffer(ctx, nt * 4 + 16).upload(lengths)
    if f.codec == "lsop":
        check(L.gf_lsop12_decode_batch_i32_dev(ctx.handle, None, f.nr, f.nc, nt, e.slots.ptr, nt * S, None, S, d_len.ptr, d_vals.ptr,
                                               d_st.ptr, e.residuals.ptr, e.res_stride, e.coefs.ptr, e.scratch.ptr), "lsop decode")
    elif f.codec == "lsop08":
        check(L.gf_lsop08_decode_batch_i32_dev(ctx.handle, f.nr, f.nc, nt, e.slots.ptr, nt * S, None, S, d_len.ptr, d_vals.ptr, d_st.ptr,
                                               e.residuals.ptr, e.res_stride, e.coefs.ptr, e.scratch.ptr), "lsop08 decode")
    else:
        fn = getattr(L, "gf_%s_decode_batch_i32_dev" % f.codec)
        check(fn(ctx.handle, None, f.nr, f.nc, nt, e.slots.ptr, nt * S, None, S, d_len.ptr, d_vals.ptr, d_st.ptr), "decode")
    ctx.synchronize()
    st = d_st.download(np.int32, nt)
    got = d_vals.download(np.int32, nt * f.cells).reshape(nt, f.cells)
    want = f.values()[np.array(e.index)]
    assert (st[ok] == 0).all(), (f.name, st[ok])
    assert np.array_equal(got[ok], want[ok]), f.name


def _assert_route(ctx, f, e):
    """the route report names the packer the family is called after"""
    rep = rp.report(ctx)
    n_ok = sum(f.expected_status(t) == OK for t in e.index)
    if f.codec == "huffman":
        p = rp.plan(rp.KIND_HUFFMAN, f.nr, f.nc, e.nt)
        assert rep.encKind == rp.KIND_HUFFMAN and rep.encBits == p.encBits, (hex(rep.encBits), hex(p.encBits))
        assert rep.encBits & rp.ENC_PACK and rep.encBits & rp.ENC_PACK_RARE
        if "general" in f.name:
            assert rep.encBits & rp.ENC_GENERAL and not rep.encBits & rp.ENC_SPLIT
        else:
            assert rep.encBits & rp.ENC_SPLIT and rep.encBits & rp.ENC_PLANE
        # word 5: the tiles k_huffman_pack left to k_huffman_pack_rare -- every tile that fits of the rare family, none of the others
        assert rep.flags[5] == (n_ok if "rare" in f.name else 0), (f.name, list(rep.flags), n_ok)
    elif f.codec == "canon":
        p = rp.plan(rp.KIND_CANON, f.nr, f.nc, e.nt)
        assert rep.encKind == rp.KIND_CANON and rep.encBits == p.encBits, (hex(rep.encBits), hex(p.encBits))
        assert rep.encBits & rp.CANON_ENC_1 and rep.encBits & rp.CANON_PACK
    # (the LSOP12, the LSOP08 and the M32 kernels are not in the route report: slot_edges.lsop16_eligible restates what selects k_canon_pack2's
    # histogram form, and gf_m32_encode_batch_i32_dev has one kernel)


# ---------------------------------------------------------------- every family at its stride


@pytest.mark.parametrize("entry", se.SMALL_FAMILIES + [(se.m32, (0,)), (se.m32, (1,))], ids=se.family_id)
def test_family_at_its_stride(entry):
    f = entry[0](*entry[1])
    ctx = _ctx()
    e = _encode(ctx, f)
    print(f.name, "S", f.stride, "tiles", f.n, "status", np.bincount(e.h_status.clip(0, 3), minlength=3).tolist())
    _check(f, e)
    _assert_route(ctx, f, e)
    _decode(ctx, f, e)


def test_general_encoder_at_its_stride():
    """k_huffman_encode<false>: five tiles of about 1.4 M cells, one packing within 16 bytes under S and one within 16 bytes over"""
    f = se.huffman_general()
    ctx = _ctx()
    e = _encode(ctx, f)
    _check(f, e)
    _assert_route(ctx, f, e)
    _decode(ctx, f, e)


def test_uniform_tiles_at_the_smallest_stride():
    """slot_stride = 16, the smallest the ABI takes (slotWords = 4): the uniform tiles (6 bytes, predictor 0) are the only ones
    that fit; every varied tile reports GF_OVERFLOW with its full length, the all-null tiles are declined, and their slots hold the
    sentinel.  A uniform packing is two 32-bit words: bytes 8 .. 15 of its slot are untouched too."""
    f = se.canon_uniform()
    ctx = _ctx()
    e = _encode(ctx, f)
    _check(f, e)
    for t in range(f.n):
        if f.expected_status(t) == OK:
            assert f.lengths[t] == 6 and (e.h_slots[t, 8:] == SENTINEL).all(), (t, e.h_slots[t].tolist())
    _assert_route(ctx, f, e)
    _decode(ctx, f, e)


def _shuffled(f, n_min):
    """f's tiles repeated to n_min tiles and more, in a shuffled order (fixed seed)"""
    index = np.tile(np.arange(f.n), -(-n_min // f.n))
    np.random.default_rng(n_min).shuffle(index)
    return index


@pytest.mark.parametrize("entry", [(se.huffman_plane, (1,)), (se.canon_plain, (1,)), (se.lsop08, (False,))], ids=se.family_id)
def test_large_batch(entry):
    """the family repeated to 2,100 tiles and more in a shuffled order: several tiles per workgroup, the tile loop's `continue`
    paths between tiles that are written"""
    f = entry[0](*entry[1])
    index = _shuffled(f, 2100)
    ctx = _ctx()
    e = _encode(ctx, f, f.values()[index], index.tolist())
    assert e.nt >= 2100
    _check(f, e)
    _assert_route(ctx, f, e)
    _decode(ctx, f, e)


# ---------------------------------------------------------------- gf_compact_dev


def _compact(ctx, n, d_slots, stride, d_lengths, blob_bytes, blob_cap, shift=0, guard=4096):
    """gf_compact_dev into a guarded blob of blob_bytes (>= blob_cap) at `shift` bytes past a 16-byte boundary;
    returns (offsets[n + 1], blob bytes, guards intact)"""
    from gridfour_amd import lib
    from gridfour_amd._lib import check
    blob = Guarded(ctx, blob_bytes, guard, shift)
    off = Guarded(ctx, (n + 1) * 8, META_GUARD)
    check(lib().gf_compact_dev(ctx.handle, None, n, d_slots, stride, d_lengths, off.ptr, blob.ptr, blob_cap), "gf_compact_dev")
    ctx.synchronize()
    h_off, off_ok = off.download(np.uint64)
    h_blob, blob_ok = blob.download()
    blob.free()
    off.free()
    return h_off, h_blob, off_ok and blob_ok


@pytest.mark.parametrize("n_min", [0, 2100], ids=["family", "large-batch"])
def test_compact_skips_overflowed_tiles(n_min):
    """encode -> compact with the lengths as the encoder left them (some > S, "length is still reported"): a tile that did not fit
    takes no room in the blob, which is the concatenation of the packings that fit.  On the plane family and on the large batch's
    result (2,100 tiles and more: the scan carries across its 1,024-wide rounds, the gather copies real packings at every
    alignment).  The region behind the slots is as long as the longest reported length: whatever a compaction that trusted those
    lengths reads lies inside the allocation."""
    f = se.huffman_plane(1)
    index = _shuffled(f, n_min) if n_min else np.arange(f.n)
    ctx = _ctx()
    e = _encode(ctx, f, f.values()[index], index.tolist())
    _check(f, e)
    n = e.nt
    assert n >= n_min and (e.h_lengths > f.stride).any() and f.guard() >= int(e.h_lengths.max())
    fit = [f.lengths[t] if f.expected_status(t) == OK else 0 for t in index]
    cat = b"".join(f.packs[t] for t in index if f.expected_status(t) == OK)
    room = int(e.h_lengths.sum())                     # room for every reported length: no compaction writes behind the blob's guard
    off, blob, intact = _compact(ctx, n, e.slots.ptr, f.stride, e.lengths.ptr, room, room, guard=f.guard())
    print("tiles", n, "d_offsets[n]", int(off[n]), "sum of the fitting lengths", len(cat), "sum of all reported lengths", room)
    assert intact
    assert off[0] == 0 and int(off[n]) == len(cat), (int(off[n]), len(cat))
    assert np.diff(off.astype(np.int64)).tolist() == fit
    assert blob[:len(cat)].tobytes() == cat and (blob[len(cat):] == SENTINEL).all()


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_compact_handmade_slots_at_every_alignment(shift):
    """slots of stride 48 with lengths 0 .. 48 in an order that starts short and long tiles at every destination misalignment,
    d_blob itself 0 .. 3 bytes past a 16-byte boundary"""
    from gridfour_amd import DeviceBuffer
    lengths = se.compact_order()
    slots, cat = se.compact_slots(lengths)
    n = len(lengths)
    ctx = _ctx()
    d_slots = DeviceBuffer(ctx, slots.nbytes).upload(slots)
    d_len = DeviceBuffer(ctx, n * 4).upload(np.array(lengths, np.uint32))
    off, blob, intact = _compact(ctx, n, d_slots.ptr, se.COMPACT_STRIDE, d_len.ptr, len(cat), len(cat), shift)
    assert intact and off.tolist() == [0] + np.cumsum(lengths).tolist()
    assert blob.tobytes() == cat


@pytest.mark.parametrize("short", [1, 0, None], ids=["one-short", "exact", "zero"])
def test_compact_blob_cap_edges(short):
    """blob_cap one byte short of the total, exactly the total, and 0: a tile that would end behind blob_cap is skipped, every
    other one is copied; d_offsets is complete and d_offsets[n] > blob_cap tells the caller"""
    from gridfour_amd import DeviceBuffer
    lengths = se.compact_order()
    slots, cat = se.compact_slots(lengths)
    n, total = len(lengths), len(cat)
    cap = 0 if short is None else total - short
    ctx = _ctx()
    d_slots = DeviceBuffer(ctx, slots.nbytes).upload(slots)
    d_len = DeviceBuffer(ctx, n * 4).upload(np.array(lengths, np.uint32))
    off, blob, intact = _compact(ctx, n, d_slots.ptr, se.COMPACT_STRIDE, d_len.ptr, total, cap)
    ends = np.cumsum(lengths)
    assert intact and off.tolist() == [0] + ends.tolist() and (int(off[n]) > cap) == (cap < total)
    want = np.full(total, SENTINEL, np.uint8)
    for t, L in enumerate(lengths):
        if ends[t] <= cap:
            want[ends[t] - L:ends[t]] = slots[t, :L]
    assert lengths[-1] > 0 or short != 1                      # (one byte short: the last tile is the one that is skipped)
    assert np.array_equal(blob, want), np.nonzero(blob != want)[0][:8]


@pytest.mark.parametrize("n", [0, 1, 1024, 1025, 2049])
def test_compact_scan_carry(n):
    """the scan's carry across its 1,024-wide rounds: tiny slots (stride 16), lengths 0 .. 16 and a few beyond the stride"""
    from gridfour_amd import DeviceBuffer
    rng = np.random.default_rng(n + 1)
    stride = 16
    lengths = rng.integers(0, 17, n).astype(np.uint32)
    lengths[rng.random(n) < 0.05] = 17 + 1000                 # reported by an encoder, not written: no room in the blob
    slots = rng.integers(0, 255, (max(n, 1), stride)).astype(np.uint8)
    fit = np.where(lengths <= stride, lengths, 0)
    cat = b"".join(slots[t, :fit[t]].tobytes() for t in range(n))
    ctx = _ctx()
    d_slots = Guarded(ctx, slots.nbytes, 4096).upload(slots)   # (behind the slots: room for the longest reported length)
    d_len = DeviceBuffer(ctx, max(n, 1) * 4).upload(lengths if n else np.zeros(1, np.uint32))
    room = int(lengths.sum()) + 16
    off, blob, intact = _compact(ctx, n, d_slots.ptr, stride, d_len.ptr, room, room)
    assert intact and off.tolist() == [0] + np.cumsum(fit).tolist()
    assert blob[:len(cat)].tobytes() == cat and (blob[len(cat):] == SENTINEL).all()


# ---------------------------------------------------------------- host memory: out_cap and blob_cap


def _host_tile(kind):
    nr, nc = se.SMALL
    v = se.ladder(nr, nc)(300)
    if kind == "float":
        f = (v.astype(np.float32) * np.float32(0.1)).astype(np.float32)
        return f, oracle.codec_float_encode(0, nr, nc, f.view(np.uint32), 6)
    enc = {"huffman": lambda: oracle.codec_huffman_encode(0, nr, nc, v)[0], "canon": lambda: oracle.codec_canon_encode(0, nr, nc, v)[0],
           "deflate": lambda: oracle.codec_deflate_encode(0, nr, nc, v)[0], "lsop12": lambda: oracle.lsop12_encode(0, nr, nc, v, True)[0],
           "lsop08": lambda: lsop08_ref.encode(0, nr, nc, v)[0]}
    return v, enc[kind]()


def _call_one(L, ctx, kind, v, out, cap, n):
    from gridfour_amd.codec import _ptr
    nr, nc = se.SMALL
    if kind == "float":
        return L.gf_float_encode_f32(ctx.handle, 0, nr, nc, _ptr(v), 6, _ptr(out), cap, C.byref(n))
    if kind == "lsop12":
        return L.gf_lsop12_encode_i32(ctx.handle, 0, nr, nc, _ptr(v), 1, _ptr(out), cap, C.byref(n))
    if kind == "lsop08":
        return L.gf_lsop08_encode_i32(ctx.handle, 0, nr, nc, _ptr(v), _ptr(out), cap, C.byref(n))
    return getattr(L, "gf_%s_encode_i32" % kind)(ctx.handle, 0, nr, nc, _ptr(v), _ptr(out), cap, C.byref(n))


@pytest.mark.parametrize("kind", ["huffman", "canon", "deflate", "lsop12", "lsop08", "float"])
def test_one_tile_out_cap_edges(kind):
    """out_cap = L - 1, L, L + 1: GF_ERR_CAPACITY with *out_len == L ("out_len = needed") and nothing written behind out_cap, or
    GF_OK with the oracle's bytes.  The Huffman and the canonical calls are made twice each: the second one replays the captured
    one-tile graph (test_gpu_routes.test_one_tile_path_at_the_lean_limit)."""
    from gridfour_amd import lib
    L = lib()
    v, ref = _host_tile(kind)
    need = len(ref)
    ctx = _ctx()
    for cap in (need - 1, need, need + 1, need - 1):
        for call in range(2 if kind in ("huffman", "canon") else 1):
            out = np.full(need + 64, SENTINEL, np.uint8)
            n = C.c_size_t(0)
            rc = _call_one(L, ctx, kind, v, out, cap, n)
            assert n.value == need, (kind, cap, call, rc, n.value, need)
            assert (out[cap:] == SENTINEL).all(), (kind, cap, call, "written behind out_cap")
            if cap < need:
                assert rc == ERR_CAPACITY, (kind, cap, call, rc)
            else:
                assert rc == 0 and out[:need].tobytes() == ref, (kind, cap, call, rc)


@pytest.mark.parametrize("kind", ["huffman", "canon", "deflate", "lsop12", "lsop08", "float"])
def test_batch_blob_cap_edges(kind):
    """blob_cap = total - 1 and total: GF_ERR_CAPACITY with offsets complete and nothing written behind blob_cap, or the exact blob"""
    from gridfour_amd import lib
    from gridfour_amd.codec import _ptr
    L = lib()
    nr, nc = se.SMALL
    ints = np.stack([se.ladder(nr, nc)(k) for k in (0, 100, 333, 640)] + [np.full(nr * nc, se.NULL, np.int32)])
    nt = len(ints)
    if kind == "float":
        vals = (ints[:4].astype(np.float32) * np.float32(0.1)).astype(np.float32)
        nt = 4
        refs = [oracle.codec_float_encode(0, nr, nc, x.view(np.uint32), 6) for x in vals]
    else:
        vals = ints
        enc = {"huffman": lambda x: oracle.codec_huffman_encode(0, nr, nc, x)[0], "canon": lambda x: oracle.codec_canon_encode(0, nr, nc, x)[0],
               "deflate": lambda x: oracle.codec_deflate_encode(0, nr, nc, x)[0], "lsop12": lambda x: oracle.lsop12_encode(0, nr, nc, x, True)[0],
               "lsop08": lambda x: lsop08_ref.encode(0, nr, nc, x)[0]}[kind]
        refs = [enc(x) or b"" for x in vals]
    cat = b"".join(refs)
    total = len(cat)
    want_off = [0] + np.cumsum([len(r) for r in refs]).tolist()
    ctx = _ctx()
    for cap in (total - 1, total):
        blob = np.full(total + 64, SENTINEL, np.uint8)
        off = np.full(nt + 1, 0xA5A5A5A5, np.uint64)
        if kind == "float":
            rc = L.gf_float_encode_batch_f32(ctx.handle, 0, nr, nc, nt, _ptr(vals), 6, _ptr(blob), cap, _ptr(off))
        elif kind == "lsop12":
            rc = L.gf_lsop12_encode_batch_i32(ctx.handle, 0, nr, nc, nt, _ptr(vals), 1, _ptr(blob), cap, _ptr(off), None, None)
        elif kind == "lsop08":
            rc = L.gf_lsop08_encode_batch_i32(ctx.handle, 0, nr, nc, nt, _ptr(vals), _ptr(blob), cap, _ptr(off), None, None)
        else:
            rc = getattr(L, "gf_%s_encode_batch_i32" % kind)(ctx.handle, 0, nr, nc, nt, _ptr(vals), _ptr(blob), cap, _ptr(off), None, None)
        assert off.tolist() == want_off, (kind, cap, rc, off.tolist(), want_off)
        assert (blob[cap:] == SENTINEL).all(), (kind, cap, "written behind blob_cap")
        if cap < total:
            assert rc == ERR_CAPACITY, (kind, cap, rc)
        else:
            assert rc == 0 and blob[:total].tobytes() == cat, (kind, cap, rc)
