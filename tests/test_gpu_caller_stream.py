"""Every device-form entry point on a CALLER'S stream (tests/caller_stream.py has the table, the two detectors and the cases).

include/gvrs_hip_codec.h: the *_dev entry points "only enqueue work" on the stream they are handed, and "a caller that hands them
another stream orders that stream itself".  Everywhere else in the suite that stream is NULL, i.e. the context's own, where a step
sent to `c->stream` instead of the caller's stream cannot show.  Here the stream is the test's, created hipStreamNonBlocking through
ctypes (once: torch's), and every expectation is a model's: the oracle, or the numpy models of tests/."""
import pytest

import caller_stream as CS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import gridfour_amd
    c = gridfour_amd.GvrsHipContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def backlog(ctx):
    """the scratch buffer of detector 2's memsets"""
    import gridfour_amd
    b = gridfour_amd.DeviceBuffer(ctx, CS.BACKLOG_BYTES)
    yield b
    b.free()


def _ids(rows):
    return [r[0] for r in rows]


CAPTURE_CASES = CS.cases((CS.CAPTURE,))
ALL_CASES = CS.cases((CS.CAPTURE, CS.ENQUEUE, CS.SYNC_ONCE))


@pytest.mark.parametrize("case", CAPTURE_CASES, ids=_ids(CAPTURE_CASES))
def test_captured_on_a_callers_stream(ctx, case):
    """detector 1: nothing runs while the caller's stream captures, and the graph alone gives the models' results for new inputs"""
    _, _, _, builder = case
    k = builder(ctx)
    try:
        with CS.Stream() as s:
            CS.capture_replay(k, s)
    finally:
        ctx.synchronize()
        k.free()


@pytest.mark.parametrize("case", ALL_CASES, ids=_ids(ALL_CASES))
def test_behind_a_backlog_on_a_callers_stream(ctx, backlog, case):
    """detector 2: the call's every step waits for the caller's stream"""
    _, _, kind, builder = case
    k = builder(ctx)
    try:
        with CS.Stream() as s:
            CS.behind_backlog(k, s, backlog, synchronising=kind == CS.SYNC_ONCE)
    finally:
        ctx.synchronize()
        k.free()


def test_pre_pass_builds_of_the_table():
    """both builds of the tree / code-length pre-pass appear among the decode cases: one tile per wave up to 4,096 tiles (the cases
    of 1 to 1,024 tiles), 64 tiles per wave beyond (the side-stream case and the canonical case of 4,160 tiles) -- by the route plan
    for the shapes the table uses; the cases themselves hold the route report to it"""
    import route_plan as RP
    for kind, one, many, big in ((RP.KIND_HUFFMAN, RP.TREES_1, RP.TREES_64, CS.ROOMY_SHAPE + (CS.ROOMY_TILES,)),
                                 (RP.KIND_CANON, RP.LENGTHS_1, RP.LENGTHS_64, (16, 16, 4160))):
        for nt in (1, 64, 256, 1024):
            assert RP.plan(kind, CS.NR, CS.NC, nt).decBits & one, (kind, nt)
        assert RP.plan(kind, *big).decBits & many, (kind, big)
    ids = [c[0] for c in ALL_CASES]
    assert "gf_huffman_decode_batch_i32_dev-side_stream" in ids and "gf_canon_decode_batch_i32_dev-t4160" in ids


def test_timer_on_a_callers_stream(ctx, backlog):
    """gf_timer_start / gf_timer_stop with a caller's stream record on THAT stream: around a backlog they measure the backlog, as the
    test's own event pair around them does; around nothing they measure next to nothing.  The test's pair lies outside the timer's,
    so it is the longer one, by two event records' worth of an in-order queue: the bound below is half a millisecond (HIP events
    tick far below a microsecond; what separates two neighbouring records is the queue's command processing, microseconds)."""
    import gridfour_amd
    timer, empty = gridfour_amd.GpuTimer(ctx), gridfour_amd.GpuTimer(ctx)
    with CS.Stream() as s:
        e0, e1 = s.event(), s.event()
        s.memset(backlog.ptr, 0, CS.BACKLOG_BYTES)                         # warm-up
        s.synchronize()
        s.record(e0)
        timer.start(s.handle)
        for _ in range(CS.BACKLOG_N):
            s.memset(backlog.ptr, 0x5A, CS.BACKLOG_BYTES)
        timer.stop(s.handle)
        s.record(e1)
        empty.start(s.handle)
        empty.stop(s.handle)
        s.synchronize()
        own, full, none = s.elapsed_ms(e0, e1), timer.elapsed_ms(), empty.elapsed_ms()
    print("caller-stream timer: backlog %.3f ms by gf_timer, %.3f ms by the test's events, %.4f ms around nothing" % (full, own, none))
    assert full > none >= 0
    assert full > 1.0, "the backlog is no backlog: %.3f ms" % full
    assert -0.01 <= own - full <= 0.5, (own, full)


def test_chained_calls_as_one_graph(ctx, backlog):
    """five entry points of different families chained on the caller's stream without a host synchronisation, captured as ONE graph
    and replayed on new inputs, then once more behind a backlog: every output against its model at the end"""
    k = CS.chain_case(ctx)
    try:
        with CS.Stream() as s:
            CS.capture_replay(k, s)
            CS.behind_backlog(k, s, backlog, synchronising=False)
    finally:
        ctx.synchronize()
        k.free()


def test_torch_stream_is_a_callers_stream(ctx, backlog):
    """the PyTorch plumbing's claim: a torch.cuda.Stream's handle is a caller's stream like any other (one codec row and one block
    row through both detectors, one more codec row through the second)"""
    import torch
    assert torch.cuda.is_available()
    ts = torch.cuda.Stream()
    for builder, capture in ((lambda c: CS.decode_case(c, "huffman", 64), True), (lambda c: CS.interp_case(c, "lattice"), True),
                             (lambda c: CS.encode_case(c, "canon", 64), False)):
        k = builder(ctx)
        try:
            with CS.Stream(ts.cuda_stream) as s:
                if capture:
                    CS.capture_replay(k, s)
                CS.behind_backlog(k, s, backlog, synchronising=False)
        finally:
            ctx.synchronize()
            k.free()
    ts.synchronize()
