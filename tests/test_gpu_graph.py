"""The device-resident entry points only enqueue work (include/gvrs_hip_codec.h: "never synchronise, never allocate
(gf_context_reserve first) -> safe for hipGraph capture"): an encode + decode of a batch is captured into a hipGraph on
the context's stream and replayed on new tile data."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _hip():
    for name in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
        try:
            return C.CDLL(name)
        except OSError:
            continue
    pytest.skip("libamdhip64 not loadable")


@pytest.mark.parametrize("codec", ["huffman", "canon"])
def test_encode_decode_replayed_from_a_graph(codec):
    import gridfour_amd
    hip = _hip()
    ctx = gridfour_amd.GvrsHipContext(0)
    nr, nc, nt = 60, 80, 256
    ctx.reserve(nr, nc, nt)
    b = gridfour_amd.DeviceTileBatch(ctx, nr, nc, nt, codec=codec)
    b.synth_dem(0x9E3779B97F4A7C15 + 1, 16)
    b.encode()                                   # warm-up outside the capture (module load, LDS attributes)
    b.decode()
    ctx.synchronize()
    stream = C.c_void_p(ctx.stream)
    graph, gexec = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamBeginCapture(stream, 0) == 0               # hipStreamCaptureModeGlobal
    b.encode()
    b.decode()
    assert hip.hipStreamEndCapture(stream, C.byref(graph)) == 0 and graph.value
    assert hip.hipGraphInstantiate(C.byref(gexec), graph, None, None, C.c_size_t(0)) == 0
    for k in range(3):
        b.synth_dem(0x9E3779B97F4A7C15 + 10 + k, 16, tile0=1000 * k)           # new tiles, same buffers
        b.decoded.fill(0)
        ctx.synchronize()
        assert hip.hipGraphLaunch(gexec, stream) == 0
        ctx.synchronize()
        assert (b.get_enc_status() == 0).all() and (b.get_dec_status() == 0).all()
        assert np.array_equal(b.get_decoded(), b.get_values()), k
    hip.hipGraphExecDestroy(gexec)
    hip.hipGraphDestroy(graph)


def _raw_m32_slots(ctx, r, c, values):
    """raw containers (10-byte header + the Differencing candidate's M32 bytes) of the tiles in device buffer `values`, one per
    slot: (slots [nt, stride] uint8, lengths uint32)"""
    import gridfour_amd
    from gridfour_amd import DeviceBuffer, lib
    nt = values.nbytes // (r * c * 4)
    sub = int(lib().gf_m32_max_stream(r, c))
    ds, dl, dm = DeviceBuffer(ctx, nt * 3 * sub + 16), DeviceBuffer(ctx, nt * 12), DeviceBuffer(ctx, nt * 3)
    dsd, dst = DeviceBuffer(ctx, nt * 4), DeviceBuffer(ctx, nt * 4)
    gridfour_amd._lib.check(lib().gf_m32_encode_batch_i32_dev(ctx.handle, None, r, c, nt, values.ptr, ds.ptr, sub, dl.ptr, dm.ptr, dsd.ptr,
                                                               dst.ptr), "gf_m32_encode_batch_i32_dev")
    ctx.synchronize()
    assert (dst.download(np.int32, nt) == 0).all()
    lens, models = dl.download(np.uint32, nt * 3)[0::3], dm.download(np.uint8, nt * 3)[0::3]
    assert (models == 1).all()                                     # (terrain without nulls: Differencing in sub-slot 0)
    streams = ds.download(np.uint8, nt * 3 * sub).reshape(nt, 3 * sub)[:, :sub]
    stride = (10 + sub + 15) // 16 * 16
    slots = np.zeros((nt, stride), np.uint8)
    slots[:, 1] = models
    slots[:, 2:6] = dsd.download(np.uint32, nt).view(np.uint8).reshape(nt, 4)
    slots[:, 6:10] = lens.copy().view(np.uint8).reshape(nt, 4)
    slots[:, 10:10 + sub] = streams
    for b in (ds, dl, dm, dsd, dst):
        b.free()
    return slots, (lens + 10).astype(np.uint32)


def test_reserved_scratch_stays_put_under_every_device_form():
    """include/gvrs_hip_codec.h: a _dev call after gf_context_reserve never allocates.  16 x 16 tiles, 4,096 of them: trees and
    packRecs are tens of MiB, so the buffers' rounding to a MiB cannot hide a need that reserve did not cover.  After the reserve
    a Huffman and a canonical encode + decode and a raw M32 decode of 4,096, 64 and 1 tiles leave workspace, trees and packRecs at
    their sizes and move no buffer of the context; LSOP12 leaves the three sizes (its inflate scratch, which the header excludes,
    may grow)."""
    import gridfour_amd
    from gridfour_amd import DeviceBuffer, lib
    import scratch_plan as sp
    r = c = 16
    big = 4096
    # the probe is not blind: a larger reserve grows the three buffers and counts their moves
    probe = gridfour_amd.GvrsHipContext(0)
    probe.reserve(r, c, 64)
    small_sizes, _, small_moves = sp.context_scratch(probe)
    probe.reserve(r, c, big)
    sizes, _, moves = sp.context_scratch(probe)
    assert all(b > a for a, b in zip(small_sizes, sizes)) and moves >= small_moves + 3, (small_sizes, sizes, small_moves, moves)
    probe.close()

    ctx = gridfour_amd.GvrsHipContext(0)
    ctx.reserve(r, c, big)
    sizes, _, moves = sp.context_scratch(ctx)
    assert all(have >= need for have, need in zip(sizes, sp.reserve(r, c, big)))
    assert sizes[1] > 10 << 20 and sizes[2] > 20 << 20, sizes
    raw = None
    for nt in (big, 64, 1):
        for codec in ("huffman", "canon"):
            b = gridfour_amd.DeviceTileBatch(ctx, r, c, nt, codec=codec)
            b.synth_dem(0x9E3779B97F4A7C15 + 3, 64)
            b.encode()
            b.decode()
            ctx.synchronize()
            assert (b.get_enc_status() == 0).all() and (b.get_dec_status() == 0).all(), (codec, nt)
            assert np.array_equal(b.get_decoded(), b.get_values()), (codec, nt)
            assert sp.context_scratch(ctx)[0] == sizes and sp.context_scratch(ctx)[2] == moves, (codec, nt, sp.context_scratch(ctx))
            if raw is None:
                raw = _raw_m32_slots(ctx, r, c, b.values) + (b.get_values(),)
            b.free()
        slots, lengths, values = raw
        d_slots, d_len = DeviceBuffer(ctx, nt * slots.shape[1] + 32).upload(slots[:nt]), DeviceBuffer(ctx, nt * 4).upload(lengths[:nt])
        d_vals, d_st = DeviceBuffer(ctx, nt * r * c * 4), DeviceBuffer(ctx, nt * 4)
        gridfour_amd._lib.check(lib().gf_m32_decode_batch_i32_dev(ctx.handle, None, r, c, nt, d_slots.ptr, nt * slots.shape[1] + 32, None,
                                                                   slots.shape[1], d_len.ptr, d_vals.ptr, d_st.ptr), "gf_m32_decode_batch_i32_dev")
        ctx.synchronize()
        assert (d_st.download(np.int32, nt) == 0).all() and np.array_equal(d_vals.download(np.int32, nt * r * c).reshape(nt, -1), values[:nt]), nt
        assert sp.context_scratch(ctx)[0] == sizes and sp.context_scratch(ctx)[2] == moves, ("m32", nt, sp.context_scratch(ctx))
        for d in (d_slots, d_len, d_vals, d_st):
            d.free()
    for nt in (big, 64, 1):
        b = gridfour_amd.DeviceTileBatch(ctx, r, c, nt, codec="lsop")
        b.synth_dem(0x9E3779B97F4A7C15 + 3, 64)
        b.encode()
        b.decode()
        ctx.synchronize()
        assert (b.get_enc_status() == 0).all() and (b.get_dec_status() == 0).all(), nt
        assert np.array_equal(b.get_decoded(), b.get_values()), nt
        assert sp.context_scratch(ctx)[0] == sizes, ("lsop", nt, sp.context_scratch(ctx))
        b.free()
    ctx.close()
