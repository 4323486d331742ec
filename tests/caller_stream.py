"""Device-form entry points on a CALLER'S stream: the table of every function of include/gvrs_hip_codec.h that takes a
`void *stream`, the two detectors of tests/test_gpu_caller_stream.py, and the case builders.

Every `*_dev` entry point promises to put all of its work on the stream it is handed.  With stream == NULL the promise cannot be
seen to break: `c->stream` and `streamOf(c, NULL)` are the same stream.  The detectors hand each entry point a stream S of the
test's own, created hipStreamNonBlocking like the context's, and make a step that went to the context's stream show:

  detector 1, `capture_replay` (rows of class "capture"): while S captures, work enqueued on S does not run and work enqueued
      anywhere else runs at once and is missing from the graph.  The outputs must still be 0xA5 after the capture, and the graph,
      replayed on inputs B and then C, must give the models' results for B and C.
  detector 2, `behind_backlog` (every row): S holds a backlog of memsets, then copies that turn the inputs from A into B, then
      memsets that turn the outputs into 0xA5, then the call, then copies of the outputs.  A step on the context's idle stream runs
      ahead of all that, on A (valid input, never garbage).  An enqueue-only form must return while the backlog still runs
      (hipEventQuery == hipErrorNotReady, else the test FAILS: the backlog was too short); for a form that synchronises S once the
      backlog must be at least four times as long as the same call on the idle context stream.

A case (class Case) is the device buffers of one call, three input sets A, B, C of one shape with the models' results for each, and
the call itself.  The models are the oracle and the numpy models of tests/; no expectation comes from a run of the library.
Every case asserts on the CPU, on the models' results, that its input sets can be told apart: an output with `items` has NO item
equal between two sets (the cells of a decode, the packing of a tile, z, the shade, ...: the sets are lifted apart to that end);
an output with `differs` is another as a whole -- counters, ARGB words and the cells of records whose tiles hold fill and null
blocks repeat values by their nature.  A case without one or the other is refused.  Entry points without device input (the
synthetic terrain) have one input set; their stale-result form is caught by the 0xA5 refill that every replay and every backlog
puts in front of the call on the caller's stream.

TABLE has one row per entry point; tests/test_caller_stream_table.py holds it to the header.  NOT_COVERED would name entry points
that have a class and no case; it is empty and the table test keeps it so."""
import ctypes as C
import time

import numpy as np

BAND = 256                       # guard bytes on both sides of every output (as tests/test_gpu_tabulate.py's Guarded)
FILL = 0xA5
HIP_NOT_READY = 600              # hipErrorNotReady
# the backlog of detector 2: BACKLOG_N memsets over BACKLOG_BYTES.  Sized on an MI355X ("Caller's streams")
BACKLOG_BYTES = 1 << 30
BACKLOG_N = 192
SEED = 0x9E3779B97F4A7C15 + 77

_hip = None


def hip():
    """libamdhip64 through ctypes, the route of the graph tests, with the argument types of the calls used here"""
    global _hip
    if _hip is None:
        L = None
        for name in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
            try:
                L = C.CDLL(name)
                break
            except OSError:
                continue
        assert L is not None, "libamdhip64 not loadable"
        vp, sz = C.c_void_p, C.c_size_t
        for name, args in {"hipStreamCreateWithFlags": [C.POINTER(vp), C.c_uint], "hipStreamDestroy": [vp], "hipStreamSynchronize": [vp],
                           "hipStreamBeginCapture": [vp, C.c_int], "hipStreamEndCapture": [vp, C.POINTER(vp)],
                           "hipGraphInstantiate": [C.POINTER(vp), vp, vp, vp, sz], "hipGraphLaunch": [vp, vp],
                           "hipGraphExecDestroy": [vp], "hipGraphDestroy": [vp], "hipMemsetAsync": [vp, C.c_int, sz, vp],
                           "hipMemcpyAsync": [vp, vp, sz, C.c_int, vp], "hipEventCreate": [C.POINTER(vp)], "hipEventDestroy": [vp],
                           "hipEventRecord": [vp, vp], "hipEventQuery": [vp], "hipEventElapsedTime": [C.POINTER(C.c_float), vp, vp]}.items():
            fn = getattr(L, name)
            fn.argtypes, fn.restype = args, C.c_int
        _hip = L
    return _hip


def _ok(status, what):
    assert status == 0, "%s: hipError %d" % (what, status)


def _addr(p):
    return p.value if isinstance(p, C.c_void_p) else int(p)


class Stream:
    """A stream of the test's own (hipStreamNonBlocking, or one handed in: torch's), with the stream-ordered copies, memsets and
    events the detectors need.  close() ends an open capture, destroys graphs and events, synchronises and destroys the stream."""

    def __init__(self, handle=None):
        self.owned = handle is None
        self.capturing = False
        self._graphs, self._events, self._keep = [], [], []
        if handle is None:
            h = C.c_void_p()
            _ok(hip().hipStreamCreateWithFlags(C.byref(h), 1), "hipStreamCreateWithFlags")        # hipStreamNonBlocking
            handle = h.value
        self.handle = C.c_void_p(handle)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def synchronize(self):
        _ok(hip().hipStreamSynchronize(self.handle), "hipStreamSynchronize")
        self._keep = []

    def memset(self, ptr, value, nbytes):
        _ok(hip().hipMemsetAsync(C.c_void_p(_addr(ptr)), value, nbytes, self.handle), "hipMemsetAsync")

    def copy(self, dst, src, nbytes):
        _ok(hip().hipMemcpyAsync(C.c_void_p(_addr(dst)), C.c_void_p(_addr(src)), nbytes, 3, self.handle), "hipMemcpyAsync d2d")

    def upload(self, dst, array):
        a = np.ascontiguousarray(array)
        self._keep.append(a)                                   # alive until the next synchronize()
        _ok(hip().hipMemcpyAsync(C.c_void_p(_addr(dst)), C.c_void_p(a.ctypes.data), a.nbytes, 1, self.handle), "hipMemcpyAsync h2d")

    def download(self, src, nbytes):
        """nbytes from device memory, copied on this stream; synchronises this stream and nothing else"""
        out = np.empty(nbytes, np.uint8)
        _ok(hip().hipMemcpyAsync(C.c_void_p(out.ctypes.data), C.c_void_p(_addr(src)), nbytes, 2, self.handle), "hipMemcpyAsync d2h")
        self.synchronize()
        return out

    def event(self):
        e = C.c_void_p()
        _ok(hip().hipEventCreate(C.byref(e)), "hipEventCreate")
        self._events.append(e)
        return e

    def record(self, e):
        _ok(hip().hipEventRecord(e, self.handle), "hipEventRecord")

    @staticmethod
    def elapsed_ms(e0, e1):
        ms = C.c_float(0)
        _ok(hip().hipEventElapsedTime(C.byref(ms), e0, e1), "hipEventElapsedTime")
        return ms.value

    def capture(self, fn):
        """fn() while this stream captures (global mode); the capture is ended whatever fn does.  Returns (fn's result, gexec)."""
        graph = C.c_void_p()
        _ok(hip().hipStreamBeginCapture(self.handle, 0), "hipStreamBeginCapture")          # hipStreamCaptureModeGlobal
        self.capturing = True
        try:
            result = fn()
        finally:
            self.capturing = False
            end = hip().hipStreamEndCapture(self.handle, C.byref(graph))
            if graph.value:
                self._graphs.append(("graph", graph))
        _ok(end, "hipStreamEndCapture")
        assert graph.value
        gexec = C.c_void_p()
        _ok(hip().hipGraphInstantiate(C.byref(gexec), graph, None, None, 0), "hipGraphInstantiate")
        self._graphs.append(("exec", gexec))
        return result, gexec

    def launch(self, gexec):
        _ok(hip().hipGraphLaunch(gexec, self.handle), "hipGraphLaunch")

    def close(self):
        if self.capturing:
            graph = C.c_void_p()
            hip().hipStreamEndCapture(self.handle, C.byref(graph))
            self.capturing = False
            if graph.value:
                self._graphs.append(("graph", graph))
        hip().hipStreamSynchronize(self.handle)
        for kind, g in reversed(self._graphs):
            (hip().hipGraphExecDestroy if kind == "exec" else hip().hipGraphDestroy)(g)
        for e in self._events:
            hip().hipEventDestroy(e)
        self._graphs, self._events, self._keep = [], [], []
        if self.owned and self.handle:
            hip().hipStreamDestroy(self.handle)
            self.handle = C.c_void_p()


class Guarded:
    """nbytes of device memory, pre-filled with 0xA5, between two guard bands (the layout of tests/test_gpu_tabulate.py's Guarded;
    this one can be read and refilled on a caller's stream)"""

    def __init__(self, ctx, nbytes):
        import gridfour_amd
        self.nbytes = int(nbytes)
        self.total = self.nbytes + 2 * BAND
        self.buf = gridfour_amd.DeviceBuffer(ctx, self.total)
        self.refill()

    @property
    def ptr(self):
        return C.c_void_p(self.buf.ptr.value + BAND)

    def refill(self, stream=None):
        if stream is None:
            self.buf.upload(np.full(self.total, FILL, np.uint8))
        else:
            stream.memset(self.buf.ptr, FILL, self.total)

    def get(self, stream=None):
        """the nbytes between the bands, the bands checked; stream None: through the context (synchronises the context's stream)"""
        raw = self.buf.download(np.uint8, self.total) if stream is None else stream.download(self.buf.ptr, self.total)
        assert (raw[:BAND] == FILL).all() and (raw[BAND + self.nbytes:] == FILL).all(), "guard band overwritten"
        return raw[BAND:BAND + self.nbytes].copy()

    def free(self):
        self.buf.free()


class Inp:
    """one input buffer of a call and its contents for the input sets A, B, C"""

    def __init__(self, ctx, name, sets, pad=32):
        import gridfour_amd
        self.name = name
        self.sets = [np.ascontiguousarray(s).reshape(-1).view(np.uint8) for s in sets]
        assert len({s.size for s in self.sets}) == 1, name
        self.nbytes = self.sets[0].size
        self.buf = gridfour_amd.DeviceBuffer(ctx, self.nbytes + pad).fill(0)
        self.stage = None
        self.buf.upload(self.sets[0])

    @property
    def ptr(self):
        return self.buf.ptr

    def free(self):
        self.buf.free()
        if self.stage is not None:
            self.stage.free()


class Out:
    """one output buffer of a call and the models' bytes for A, B, C.  mask[k]: the bytes the call specifies (None: all of them);
    items[k]: the output's items as the model has them, when no item may be equal between two input sets"""

    def __init__(self, ctx, name, want, mask=None, items=None, differs=False):
        self.name, self.differs = name, differs                # differs: the output as a whole is another for each input set
        self.want = [np.ascontiguousarray(w).reshape(-1).view(np.uint8) for w in want]
        assert len({w.size for w in self.want}) == 1, name
        self.mask = mask
        self.items = items
        self.dev = Guarded(ctx, self.want[0].size)
        self.kept = None

    @property
    def ptr(self):
        return self.dev.ptr

    def check(self, got, k, where):
        want = self.want[k]
        bad = got != want
        if self.mask is not None:
            bad &= np.ascontiguousarray(self.mask[k]).reshape(-1)
        assert not bad.any(), "%s: output %s differs from the model for input set %s at bytes %s (%d in all)" % (
            where, self.name, "ABC"[k], np.flatnonzero(bad)[:8].tolist(), int(bad.sum()))

    def free(self):
        self.dev.free()
        if self.kept is not None:
            self.kept.free()


class Case:
    """the buffers, input sets, models and call of one entry point.  call(stream) makes the call with stream = None or a stream
    handle and returns its gf_status; reserve() is what the header asks for before a capture (may be None)."""

    def __init__(self, ctx, name, inputs, outputs, call, reserve=None, sets=3):
        self.ctx, self.name, self.inputs, self.outputs, self.call, self.reserve, self.sets = ctx, name, inputs, outputs, call, reserve, sets
        self.extra = []                                        # further buffers to free with the case
        self.route = None                                      # route(report): the route a call on the caller's stream must take
        if inputs:
            assert sets == 3
        self.assert_distinct()

    def assert_distinct(self):
        """no output item equal between A, B and C, on the models' results"""
        n = 0
        for o in self.outputs:
            if o.differs:
                n += 1
                w = o.want if o.mask is None else [x[np.ascontiguousarray(m).reshape(-1)] for x, m in zip(o.want, o.mask)]
                assert all(w[a].size != w[b].size or (w[a] != w[b]).any() for a, b in ((0, 1), (0, 2), (1, 2))), (self.name, o.name)
            if o.items is None:
                continue
            n += 1
            for a, b in ((0, 1), (0, 2), (1, 2)):
                ia, ib = o.items[a], o.items[b]
                if isinstance(ia, np.ndarray):
                    same = np.flatnonzero(ia.reshape(-1) == ib.reshape(-1))
                else:
                    same = [i for i, (x, y) in enumerate(zip(ia, ib)) if x == y]
                assert len(same) == 0 and len(ia) == len(ib), "%s: output %s has items equal between input sets %s and %s: %s" % (
                    self.name, o.name, "ABC"[a], "ABC"[b], list(same[:8]))
        assert n > 0 or not self.inputs, "%s: no output with items to tell the input sets apart" % self.name

    def check(self, k, where, stream=None):
        for o in self.outputs:
            o.check(o.dev.get(stream), k, "%s, %s" % (self.name, where))

    def untouched(self, where):
        for o in self.outputs:
            got = o.dev.get()
            assert (got == FILL).all(), "%s, %s: output %s was written (%d bytes): something ran" % (
                self.name, where, o.name, int((got != FILL).sum()))

    def check_route(self):
        if self.route:
            import route_plan
            self.route(route_plan.report(self.ctx))

    def free(self):
        for b in self.inputs + self.outputs + self.extra:
            b.free()


# ---------------------------------------------------------------------------------------------------------------- detectors

def capture_replay(case, stream):
    """detector 1 (module docstring); `stream` a Stream"""
    from gridfour_amd import _lib
    ctx = case.ctx
    if case.reserve:
        case.reserve()
    assert case.call(stream.handle) == _lib.OK, "%s outside the capture: %s" % (case.name, _lib.lib().gf_last_error())
    stream.synchronize()
    case.check(0, "on the caller's stream, outside the capture", stream)
    for o in case.outputs:
        o.dev.refill()
    ctx.synchronize()
    status, gexec = stream.capture(lambda: case.call(stream.handle))
    assert status == _lib.OK, "%s while its stream captures: status %d %s" % (case.name, status, _lib.lib().gf_last_error())
    ctx.synchronize()
    case.check_route()                                          # (host-side records of the launch sites: nothing ran)
    case.untouched("after the capture, before any launch")
    for k in (1, 2) if case.inputs else (0, 0):
        for o in case.outputs:
            o.dev.refill(stream)
        for i in case.inputs:
            stream.upload(i.ptr, i.sets[k])
        stream.launch(gexec)
        stream.synchronize()
        case.check(k, "graph replayed on input set %s" % "ABC"[k], stream)


def idle_call(case):
    """the call on the idle context stream (stream = NULL), inputs A: its wall time in ms (to the end of the device work), the
    result held to the model"""
    from gridfour_amd import _lib
    ctx = case.ctx
    ctx.synchronize()
    t0 = time.perf_counter()
    status = case.call(None)
    ctx.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    assert status == _lib.OK, "%s on the context's stream: %s" % (case.name, _lib.lib().gf_last_error())
    case.check(0, "on the context's own stream")
    return ms


def behind_backlog(case, stream, backlog, synchronising):
    """detector 2 (module docstring); `backlog` a DeviceBuffer of BACKLOG_BYTES.  Prints the measured backlog and idle-call times."""
    import gridfour_amd
    from gridfour_amd import _lib
    ctx = case.ctx
    if case.reserve:
        case.reserve()
    for i in case.inputs:
        i.buf.upload(i.sets[0])                                 # (the device buffers hold A, whatever ran before)
    idle_ms = idle_call(case)                                   # also the warm-up: module load, scratch growth
    idle_ms = min(idle_ms, idle_call(case))
    for i in case.inputs:
        i.stage = i.stage or gridfour_amd.DeviceBuffer(ctx, i.nbytes + 32).upload(i.sets[1])
    for o in case.outputs:
        o.kept = o.kept or gridfour_amd.DeviceBuffer(ctx, o.dev.total)
        o.kept.fill(0)
    ctx.synchronize()
    k = 1 if case.inputs else 0
    e0, produced = stream.event(), stream.event()
    stream.record(e0)
    for _ in range(BACKLOG_N):
        stream.memset(backlog.ptr, 0x5A, BACKLOG_BYTES)
    for i in case.inputs:
        stream.copy(i.ptr, i.stage.ptr, i.nbytes)
    for o in case.outputs:
        o.dev.refill(stream)
    stream.record(produced)
    status = case.call(stream.handle)
    query = hip().hipEventQuery(produced)
    for o in case.outputs:
        stream.copy(o.kept.ptr, o.dev.buf.ptr, o.dev.total)
    stream.synchronize()
    case.check_route()
    assert status == _lib.OK, "%s behind a backlog: status %d %s" % (case.name, status, _lib.lib().gf_last_error())
    backlog_ms = stream.elapsed_ms(e0, produced)
    print("caller-stream %-52s backlog %7.2f ms   idle call %7.3f ms" % (case.name, backlog_ms, idle_ms))
    if synchronising:
        assert backlog_ms >= 4 * idle_ms, "%s: the backlog (%.2f ms) is too short for a call of %.3f ms" % (case.name, backlog_ms, idle_ms)
    else:
        assert query == HIP_NOT_READY, ("%s: the backlog of %.2f ms had drained when the call returned (hipEventQuery %d): the backlog is "
                                        "too short, or the call waited for its stream" % (case.name, backlog_ms, query))
    for o in case.outputs:
        raw = stream.download(o.kept.ptr, o.dev.total)
        assert (raw[:BAND] == FILL).all() and (raw[BAND + o.dev.nbytes:] == FILL).all(), "%s: guard band of %s overwritten" % (case.name, o.name)
        o.check(raw[BAND:BAND + o.dev.nbytes], k, "%s, behind a backlog on the caller's stream" % case.name)


# ---------------------------------------------------------------------------------------------------------------- tile codecs

NR, NC = 60, 80
LIFT = 100000            # added to input sets B (once) and C (twice): no cell of one set equals the same cell of another


def dem_sets(nt, nr=NR, nc=NC, style=0):
    """three batches of nt tiles from oracle.dem_tiles, different terrain each, lifted apart"""
    import oracle
    sets = [oracle.dem_tiles(SEED, nr, nc, 16, 3000 * k, nt, style=style) + np.int32(LIFT * k) for k in range(3)]
    assert all(np.abs(s - LIFT * k).max() < LIFT // 2 for k, s in enumerate(sets))
    return sets


def _slots(packings, stride):
    """(slots [nt, stride] uint8 with the packings, lengths uint32, mask of the packings' bytes)"""
    nt = len(packings)
    slots, lengths = np.zeros((nt, stride), np.uint8), np.zeros(nt, np.uint32)
    for t, p in enumerate(packings):
        slots[t, :len(p)] = np.frombuffer(p, np.uint8)
        lengths[t] = len(p)
    return slots, lengths, np.arange(stride)[None, :] < lengths[:, None]


_MODELS = {}


def _model_packings(codec, nr, nc, tiles, flags=0):
    """per tile (packing, predictor) of the reference encoder: the oracle's batch forms.  Computed once per batch of tiles and
    shared by the tests that need it; nobody changes it."""
    key = (codec, nr, nc, flags, tiles.shape, hash(tiles.tobytes()))
    if key not in _MODELS:
        _MODELS[key] = _model_packings_of(codec, nr, nc, tiles, flags)
    return _MODELS[key]


def _model_packings_of(codec, nr, nc, tiles, flags):
    import oracle
    if codec == "lsop":
        return [oracle.lsop12_encode(0, nr, nc, t, False, bool(flags & 2)) for t in tiles]
    slots, lengths, preds = (oracle.batch_huffman_encode if codec == "huffman" else oracle.batch_canon_encode)(0, nr, nc, tiles)
    return [(bytes(slots[t, :lengths[t]]), int(preds[t])) for t in range(len(tiles))]


def _stride(nr, nc):
    from gridfour_amd import lib
    return int(lib().gf_huffman_default_stride(nr, nc))


def _reserve(ctx, nr, nc, nt):
    return lambda: ctx.reserve(nr, nc, nt)


def encode_case(ctx, codec, nt, nr=NR, nc=NC):
    """gf_huffman_ / gf_canon_encode_batch_i32_dev: slots (the packing's bytes), lengths, predictors, statuses"""
    from gridfour_amd import lib
    sets = dem_sets(nt, nr, nc)
    stride = _stride(nr, nc)
    model = [_model_packings(codec, nr, nc, s) for s in sets]
    packed = [_slots([p for p, _ in m], stride) for m in model]
    v = Inp(ctx, "values", sets)
    o_slots = Out(ctx, "slots", [p[0] for p in packed], mask=[p[2] for p in packed], items=[[p for p, _ in m] for m in model])
    o_len = Out(ctx, "lengths", [p[1] for p in packed])
    o_pred = Out(ctx, "predictors", [np.array([u for _, u in m], np.uint8) for m in model])
    o_st = Out(ctx, "status", [np.zeros(nt, np.int32)] * 3)
    fn = getattr(lib(), "gf_%s_encode_batch_i32_dev" % codec)
    call = lambda s: fn(ctx.handle, s, 0, nr, nc, nt, v.ptr, o_slots.ptr, stride, o_len.ptr, o_pred.ptr, o_st.ptr, 0xF)
    return Case(ctx, "gf_%s_encode_batch_i32_dev[%d]" % (codec, nt), [v], [o_slots, o_len, o_pred, o_st], call, _reserve(ctx, nr, nc, nt))


def decode_case(ctx, codec, nt, nr=NR, nc=NC, sets=None, repeat=1, name=None, route=None):
    """gf_huffman_ / gf_canon_ / gf_m32_decode_batch_i32_dev from slots: the cells and the statuses.  sets: the three batches of
    tiles (default dem_sets); repeat: the batch is the sets' tiles that many times over (a large batch of few different tiles);
    route(report): what the context's route report must say after a call on the caller's stream"""
    from gridfour_amd import lib
    sets = dem_sets(nt // repeat, nr, nc) if sets is None else sets
    assert len(sets[0]) * repeat == nt
    stride = _stride(nr, nc)
    if codec == "m32":
        packed = [_slots(_raw_m32(nr, nc, s), stride) for s in sets]
    else:
        packed = [_slots([p for p, _ in _model_packings(codec, nr, nc, s)], stride) for s in sets]
    if repeat > 1:
        sets = [np.tile(s, (repeat, 1)) for s in sets]
        packed = [(np.tile(p[0], (repeat, 1)), np.tile(p[1], repeat)) for p in packed]
    slots, lengths = Inp(ctx, "slots", [p[0] for p in packed]), Inp(ctx, "lengths", [p[1] for p in packed])
    o_val = Out(ctx, "values", sets, items=sets)
    o_st = Out(ctx, "status", [np.zeros(nt, np.int32)] * 3)
    fn = getattr(lib(), "gf_%s_decode_batch_i32_dev" % codec)
    call = lambda s: fn(ctx.handle, s, nr, nc, nt, slots.ptr, nt * stride + 32, None, stride, lengths.ptr, o_val.ptr, o_st.ptr)
    case = Case(ctx, name or "gf_%s_decode_batch_i32_dev[%d]" % (codec, nt), [slots, lengths], [o_val, o_st], call, _reserve(ctx, nr, nc, nt))
    case.route = route
    return case


ROOMY_SHAPE, ROOMY_TILES, ROOMY_BASE = (80, 100), 4160, 64


def roomy_case(ctx):
    """a Huffman decode that takes the roomy run on the context's SIDE stream, as tests/test_gpu_roomy.py chooses it: at least 4,096
    tiles, some of them with an M32 stream beyond the fast run's LDS buffer, on a context whose last batch listed such tiles (the
    detectors' first calls see to that).  The fork and join events of the side stream are recorded on the caller's stream.  More
    than 4,096 tiles: the pre-pass build of 64 tiles per wave as well.  64 different tiles, 65 times over."""
    import route_plan as RP
    nr, nc = ROOMY_SHAPE
    p = RP.plan(RP.KIND_HUFFMAN, nr, nc, ROOMY_TILES, roomy_seen=2)
    assert p.roomyForm == RP.ROOMY_BESIDE and p.prepass == 64 and p.decBits & RP.TREES_64, (p.roomyForm, p.prepass, hex(p.decBits))
    sets = []
    for k, dem in enumerate(dem_sets(ROOMY_BASE, nr, nc)):
        rough = np.stack(RP.roomy_tiles(nr, nc, 8, 11 + k, p)).astype(np.int32) + np.int32(LIFT * k)
        dem[::8] = rough
        sets.append(dem)

    def route(r):
        assert r.decKind == RP.KIND_HUFFMAN and r.roomyForm == RP.ROOMY_BESIDE and r.prepass == 64, (r.decKind, r.roomyForm, r.prepass)
        assert r.decBits & RP.dec_bit(RP.DEC_FAST_ROOMY, p.decThreads) and r.decBits & RP.TREES_64, hex(r.decBits)
        assert r.roomySeen > 1, r.roomySeen                     # the pre-pass listed tiles for the roomy run
    return decode_case(ctx, "huffman", ROOMY_TILES, nr, nc, sets=sets, repeat=ROOMY_TILES // ROOMY_BASE, name="gf_huffman_decode_batch_i32_dev[side stream]",
                       route=route)


def canon_many_case(ctx):
    """more than 4,096 tiles: the canonical pre-pass build of 64 tiles per wave (16 x 16 tiles keep the batch small)"""
    import route_plan as RP
    assert RP.plan(RP.KIND_CANON, 16, 16, 4160).decBits & RP.LENGTHS_64

    def route(r):
        assert r.decKind == RP.KIND_CANON and r.decBits & RP.LENGTHS_64, hex(r.decBits)
    return decode_case(ctx, "canon", 4160, 16, 16, route=route)


def canon_fast_route(r):
    """the canonical cases of 60 x 80 tiles go through the canonical run of the fast kernel (viaFast)"""
    import route_plan as RP
    p = RP.plan(RP.KIND_CANON, NR, NC, 64)
    assert p.viaFast and r.decKind == RP.KIND_CANON and r.decBits & RP.dec_bit(RP.DEC_FAST_CANON, p.decThreads), (p.viaFast, hex(r.decBits))


def _raw_m32(nr, nc, tiles):
    """raw containers of gf_m32_decode_batch_i32_dev: the 10-byte header (codec index, predictor, seed, nM32) and the M32 bytes of
    the Differencing residuals, from the oracle's predictor (which writes M32)"""
    import oracle
    out = []
    for t in tiles:
        m32, seed = oracle.predictor_encode(1, nr, nc, t)
        out.append(bytes([0, 1]) + int(seed).to_bytes(4, "little", signed=True) + len(m32).to_bytes(4, "little") + m32)
    return out


def m32_encode_case(ctx, nt, nr=NR, nc=NC):
    """gf_m32_encode_batch_i32_dev: three candidate streams per tile (Differencing, Linear, Triangle), lengths, models, seeds"""
    import oracle
    from gridfour_amd import lib
    sets = dem_sets(nt, nr, nc)
    assert not any((x == np.int32(-2 ** 31)).any() for x in sets)
    sub = int(lib().gf_m32_max_stream(nr, nc))
    streams, masks, lens, models, seeds, items = [], [], [], [], [], []
    for s in sets:
        st, mk = np.zeros((nt, 3, sub), np.uint8), np.zeros((nt, 3, sub), bool)
        ln, md, sd = np.zeros((nt, 3), np.uint32), np.zeros((nt, 3), np.uint8), np.zeros(nt, np.uint32)
        it = []
        for t in range(nt):
            for j, m in enumerate((1, 2, 3)):                  # Differencing, Linear, Triangle: tiles without nulls
                c, seed = oracle.predictor_encode(m, nr, nc, s[t])
                b = np.frombuffer(c, np.uint8)
                st[t, j, :b.size], mk[t, j, :b.size], ln[t, j], md[t, j] = b, True, b.size, m
            sd[t] = int(seed) & 0xFFFFFFFF
            it.append((bytes(st[t, 0, :ln[t, 0]]), int(sd[t])))
        streams.append(st), masks.append(mk), lens.append(ln), models.append(md), seeds.append(sd), items.append(it)
    v = Inp(ctx, "values", sets)
    o = [Out(ctx, "streams", streams, mask=masks, items=items), Out(ctx, "lengths", lens), Out(ctx, "models", models),
         Out(ctx, "seeds", seeds), Out(ctx, "status", [np.zeros(nt, np.int32)] * 3)]
    call = lambda s: lib().gf_m32_encode_batch_i32_dev(ctx.handle, s, nr, nc, nt, v.ptr, o[0].ptr, sub, o[1].ptr, o[2].ptr, o[3].ptr, o[4].ptr)
    return Case(ctx, "gf_m32_encode_batch_i32_dev[%d]" % nt, [v], o, call, _reserve(ctx, nr, nc, nt))


def compact_case(ctx, nt, nr=NR, nc=NC):
    """gf_compact_dev: offsets (the exclusive scan of the lengths) and the packings end to end"""
    from gridfour_amd import lib
    sets = dem_sets(nt, nr, nc)
    stride = _stride(nr, nc)
    packed = [_slots([p for p, _ in _model_packings("huffman", nr, nc, s)], stride) for s in sets]
    cap = max(int(p[1].sum()) for p in packed) + 64
    offs, blobs, masks = [], [], []
    for sl, ln, _ in packed:
        off = np.concatenate([[0], np.cumsum(ln.astype(np.uint64))]).astype(np.uint64)
        blob = np.zeros(cap, np.uint8)
        blob[:int(off[-1])] = np.concatenate([sl[t, :ln[t]] for t in range(nt)])
        offs.append(off), blobs.append(blob), masks.append(np.arange(cap) < int(off[-1]))
    slots, lengths = Inp(ctx, "slots", [p[0] for p in packed]), Inp(ctx, "lengths", [p[1] for p in packed])
    o_off = Out(ctx, "offsets", offs)
    o_blob = Out(ctx, "blob", blobs, mask=masks, items=[[bytes(b[:4096])] for b in blobs])
    call = lambda s: lib().gf_compact_dev(ctx.handle, s, nt, slots.ptr, stride, lengths.ptr, o_off.ptr, o_blob.ptr, cap)
    return Case(ctx, "gf_compact_dev[%d]" % nt, [slots, lengths], [o_off, o_blob], call)


def synth_case(ctx, form, nt=64, nr=NR, nc=NC):
    """gf_synth_dem[_masked|_style]_dev: no device input, the tiles of oracle.dem_tiles for the same arguments"""
    import oracle
    from gridfour_amd import lib
    seed, per_row, tile0 = SEED & (2 ** 64 - 1), 16, 40
    mask, style = {"": (0, 0), "_masked": (150, 0), "_style": (100, oracle.DEM_STYLE_ROUGH)}[form]
    want = oracle.dem_tiles(seed, nr, nc, per_row, tile0, nt, mask_per_mille=mask, style=style)
    o = Out(ctx, "values", [want] * 3)
    L = lib()
    call = {"": lambda s: L.gf_synth_dem_dev(ctx.handle, s, seed, nr, nc, per_row, tile0, nt, o.ptr),
            "_masked": lambda s: L.gf_synth_dem_masked_dev(ctx.handle, s, seed, nr, nc, per_row, tile0, nt, mask, o.ptr),
            "_style": lambda s: L.gf_synth_dem_style_dev(ctx.handle, s, seed, nr, nc, per_row, tile0, nt, mask, style, o.ptr)}[form]
    return Case(ctx, "gf_synth_dem%s_dev" % form, [], [o], call, sets=1)


def _float_sets(nt, nr, nc):
    """three batches of float tiles as raw bits, no cell's bits equal between two of them"""
    sets = [(s.astype(np.float32) * np.float32(0.25) + np.float32(0.125 * k)).view(np.uint32) for k, s in enumerate(dem_sets(nt, nr, nc))]
    return sets


def float_planes_case(ctx, direction, nt=64, nr=NR, nc=NC):
    """gf_float_planes_encode_dev / _decode_dev against oracle.float_planes_encode"""
    import oracle
    from gridfour_amd import lib
    L = lib()
    pb = int(L.gf_float_planes_bytes(nr, nc))
    stride = (pb + 15) // 16 * 16
    cells = _float_sets(nt, nr, nc)
    planes, masks = [], []
    for s in cells:
        p = np.zeros((nt, stride), np.uint8)
        for t in range(nt):
            p[t, :pb] = oracle.float_planes_encode(nr, nc, s[t])[:pb]
        planes.append(p), masks.append(np.broadcast_to(np.arange(stride)[None, :] < pb, (nt, stride)).copy())
    if direction == "encode":
        v = Inp(ctx, "values", cells)
        o = Out(ctx, "planes", planes, mask=masks, items=[[bytes(p[t, :pb]) for t in range(nt)] for p in planes])
        call = lambda s: L.gf_float_planes_encode_dev(ctx.handle, s, nr, nc, nt, v.ptr, o.ptr, stride)
    else:
        v = Inp(ctx, "planes", planes)
        o = Out(ctx, "values", cells, items=cells)
        call = lambda s: L.gf_float_planes_decode_dev(ctx.handle, s, nr, nc, nt, v.ptr, stride, o.ptr)
    return Case(ctx, "gf_float_planes_%s_dev" % direction, [v], [o], call)


# ---------------------------------------------------------------------------------------------------------------- LSOP12

def _lsop_model(nr, nc, tiles, rs):
    """(residuals [nt, rs] int32, coefs [nt, 16] uint32) of oracle.lsop12_residuals: what gf_lsop12_predict_dev writes"""
    import oracle
    nt = len(tiles)
    res, co = np.zeros((nt, rs), np.int32), np.zeros((nt, 16), np.uint32)
    for t in range(nt):
        seed, u, init, inter = oracle.lsop12_residuals(nr, nc, tiles[t])
        both = np.concatenate([init, inter])
        res[t, :both.size] = both
        co[t, 0] = np.int32(seed).view(np.uint32)
        co[t, 1:13] = u.view(np.uint32)
    return res, co


def lsop_stage_case(ctx, stage, nt=64, nr=NR, nc=NC):
    """gf_lsop12_predict_dev (tiles -> residual streams + coefficients) and gf_lsop12_reconstruct_dev (the inverse)"""
    from gridfour_amd import lib
    L = lib()
    n = int(L.gf_lsop12_residual_count(nr, nc))
    rs = (n + 3) // 4 * 4
    sets = dem_sets(nt, nr, nc)
    models = [_lsop_model(nr, nc, s, rs) for s in sets]
    used = np.broadcast_to(np.arange(rs)[None, :] < n, (nt, rs)).repeat(4, axis=1)
    ok = [np.zeros(nt, np.int32)] * 3
    if stage == "predict":
        v = Inp(ctx, "values", sets)
        o = [Out(ctx, "residuals", [m[0] for m in models], mask=[used] * 3),
             Out(ctx, "coefs", [m[1] for m in models], items=[[m[1][t].tobytes() for t in range(nt)] for m in models]), Out(ctx, "status", ok)]
        call = lambda s: L.gf_lsop12_predict_dev(ctx.handle, s, nr, nc, nt, v.ptr, o[0].ptr, rs, o[1].ptr, o[2].ptr)
        ins = [v]
    else:
        r, c = Inp(ctx, "residuals", [m[0] for m in models]), Inp(ctx, "coefs", [m[1] for m in models])
        o = [Out(ctx, "values", sets, items=sets), Out(ctx, "status", ok)]
        call = lambda s: L.gf_lsop12_reconstruct_dev(ctx.handle, s, nr, nc, nt, r.ptr, rs, c.ptr, None, o[0].ptr, o[1].ptr)
        ins = [r, c]
    return Case(ctx, "gf_lsop12_%s_dev" % stage, ins, o, call, _reserve(ctx, nr, nc, nt))


class _Work:
    """the caller-provided work buffers of the LSOP12 batch forms (their contents are the library's business)"""

    def __init__(self, ctx, nt, nr, nc):
        from gridfour_amd import DeviceBuffer, lib
        n = int(lib().gf_lsop12_residual_count(nr, nc))
        self.rs = (n + 3) // 4 * 4
        self.res, self.co, self.st = DeviceBuffer(ctx, nt * self.rs * 4 + 16), DeviceBuffer(ctx, nt * 64), DeviceBuffer(ctx, nt * 4)
        self.nbytes, self.sets, self.stage = 0, [], None

    def free(self):
        for b in (self.res, self.co, self.st):
            b.free()


def lsop_encode_case(ctx, ex, nt=64, nr=NR, nc=NC):
    """gf_lsop12_encode_batch_i32_dev and its _ex form with GF_LSOP_VALUE_CHECKSUM: the current container, against the oracle"""
    from gridfour_amd import lib
    L = lib()
    sets = dem_sets(nt, nr, nc)
    stride = _stride(nr, nc)
    flags = 2 if ex else 0
    model = [_model_packings("lsop", nr, nc, s, flags) for s in sets]
    packed = [_slots([p for p, _ in m], stride) for m in model]
    v, w = Inp(ctx, "values", sets), _Work(ctx, nt, nr, nc)
    o = [Out(ctx, "slots", [p[0] for p in packed], mask=[p[2] for p in packed], items=[[p for p, _ in m] for m in model]),
         Out(ctx, "lengths", [p[1] for p in packed]), Out(ctx, "status", [np.zeros(nt, np.int32)] * 3)]
    if ex:
        call = lambda s: L.gf_lsop12_encode_batch_i32_dev_ex(ctx.handle, s, 0, nr, nc, nt, v.ptr, flags, o[0].ptr, stride, o[1].ptr, o[2].ptr,
                                                             w.res.ptr, w.rs, w.co.ptr, w.st.ptr)
    else:
        call = lambda s: L.gf_lsop12_encode_batch_i32_dev(ctx.handle, s, 0, nr, nc, nt, v.ptr, o[0].ptr, stride, o[1].ptr, o[2].ptr,
                                                          w.res.ptr, w.rs, w.co.ptr, w.st.ptr)
    case = Case(ctx, "gf_lsop12_encode_batch_i32_dev%s" % ("_ex" if ex else ""), [v], o, call, _reserve(ctx, nr, nc, nt))
    case.extra.append(w)
    return case


def _stepped_sets(nt, nr, nc):
    """three batches of planes with steps (long runs of equal residuals: the Deflate container wins, as in
    tests/test_gpu_lsop_numeric.py), lifted apart"""
    y, x = np.mgrid[0:nr, 0:nc]
    return [np.stack([((3 + k) * x + (5 + t % 7) * y + 40 * ((x // (8 + t % 9) + y // 16) % 2) + 11 * t + LIFT * k).astype(np.int32).ravel()
                      for t in range(nt)]) for k in range(3)]


def lsop_decode_case(ctx, container, nt=64, nr=NR, nc=NC):
    """gf_lsop12_decode_batch_i32_dev on the current container (type 2), the legacy one (type 0) or Deflate (type 1)"""
    import oracle
    from gridfour_amd import lib
    L = lib()
    sets = _stepped_sets(nt, nr, nc) if container == "deflate" else dem_sets(nt, nr, nc)
    stride = _stride(nr, nc)
    enc = {"current": lambda t: oracle.lsop12_encode(0, nr, nc, t, False)[0], "legacy": lambda t: oracle.lsop12_encode_legacy_huffman(0, nr, nc, t),
           "deflate": lambda t: oracle.lsop12_encode(0, nr, nc, t, True)[0]}[container]
    packs = [[enc(t) for t in s] for s in sets]
    if container == "deflate":                       # (the encoder keeps Deflate only where it is shorter)
        assert all(oracle.lsop12_encode(0, nr, nc, t, True)[1] == 1 for s in sets for t in s), "a tile's Deflate container did not win"
    packed = [_slots(p, stride) for p in packs]
    slots, lengths, w = Inp(ctx, "slots", [p[0] for p in packed]), Inp(ctx, "lengths", [p[1] for p in packed]), _Work(ctx, nt, nr, nc)
    o = [Out(ctx, "values", sets, items=sets), Out(ctx, "status", [np.zeros(nt, np.int32)] * 3)]
    call = lambda s: L.gf_lsop12_decode_batch_i32_dev(ctx.handle, s, nr, nc, nt, slots.ptr, nt * stride + 32, None, stride, lengths.ptr,
                                                      o[0].ptr, o[1].ptr, w.res.ptr, w.rs, w.co.ptr, w.st.ptr)
    case = Case(ctx, "gf_lsop12_decode_batch_i32_dev[%s]" % container, [slots, lengths], o, call, _reserve(ctx, nr, nc, nt))
    case.extra.append(w)
    return case


# ---------------------------------------------------------------------------------------------------------------- grid blocks

BLOCK = (100, 150)               # the block of the interpolation, rendering, downsampling and tabulation cases


def _st(fn):
    """the gf_status of a GvrsHipContext method that raises on a negative one"""
    from gridfour_amd._lib import GvrsHipError
    try:
        fn()
        return 0
    except GvrsHipError as e:
        return e.status


def _smooth_blocks(rng):
    """three float blocks of gentle relief inside -70 .. 70 (every pixel is lit: no shade falls back to the ambient level)"""
    y, x = np.mgrid[0:BLOCK[0], 0:BLOCK[1]]
    return [(20 * np.sin(0.07 * x + k) + 15 * np.cos(0.05 * y + 2 * k) + 9 * k + rng.uniform(-0.01, 0.01, BLOCK)).astype(np.float32) for k in range(3)]


def interp_case(ctx, form):
    """gf_block_interp_points_dev / _lattice_dev, target SECOND: every output array against tests/interp_ref.py"""
    import interp_cases as K
    import interp_ref as R
    rng = np.random.default_rng(4100)
    spec = R.Spec(BLOCK[0], BLOCK[1], None, R.FLOAT, wrap=0, target=R.SECOND, row_spacing=0.9, col_spacing=1.1)
    s = K.lib_spec(spec)
    blocks = [K.random_block(rng, R.FLOAT, BLOCK) for _ in range(3)]
    lattice = (1.7, 2.6, 0.91, 1.37, 100, 100)
    if form == "points":
        n = 700
        coords = [(rng.uniform(1.0, BLOCK[0] - 2.0, n), rng.uniform(1.0, BLOCK[1] - 2.0, n)) for _ in range(3)]
    else:
        n = lattice[4] * lattice[5]
        coords = [R.lattice_coords(*lattice)] * 3
    want = [R.interp(spec, b, r, c) for b, (r, c) in zip(blocks, coords)]
    assert all((w["status"] == R.OK).all() for w in want)
    blk = Inp(ctx, "block", blocks)
    ins = [blk]
    outs = [Out(ctx, k, [np.ascontiguousarray(w[k]) for w in want], items=[w[k].view(np.uint64) for w in want] if k == "z" else None)
            for k in K.FIELDS + ("status",)]
    ptrs = {o.name: o.ptr for o in outs}
    if form == "points":
        rows, cols = Inp(ctx, "rows", [c[0] for c in coords]), Inp(ctx, "cols", [c[1] for c in coords])
        ins += [rows, cols]
        call = lambda st: _st(lambda: ctx.interp_points_dev(s, blk.ptr, n, rows.ptr, cols.ptr, ptrs, stream=st))
    else:
        call = lambda st: _st(lambda: ctx.interp_lattice_dev(s, blk.ptr, lattice, ptrs, stream=st))
    return Case(ctx, "gf_block_interp_%s_dev" % form, ins, outs, call)


def render_case(ctx, form):
    """gf_block_render_cells_dev / _lattice_dev / _points_dev against tests/render_ref.py"""
    import gridfour_amd
    import interp_cases as K
    import interp_ref as R
    import render_cases as RC
    import render_ref as M
    rng = np.random.default_rng(4200)
    records = RC._ramp(9, -70.0, 70.0)
    model, pal = M.Palette(records, 0xff00ff00), gridfour_amd.Palette(ctx, records, 0xff00ff00)
    light = M.Light(-0.2, -0.2, RC.LIGHTS["cog"].sun, 0.25)
    li = RC.lib_light(light)
    spec = R.Spec(BLOCK[0], BLOCK[1], None, R.FLOAT, wrap=0, target=R.FIRST, row_spacing=0.9, col_spacing=1.1)
    s = K.lib_spec(spec)
    blocks = _smooth_blocks(rng)
    blk = Inp(ctx, "block", blocks)
    if form == "cells":
        n = BLOCK[0] * BLOCK[1]
        want = [M.render_cells(model, b.ravel(), R.FLOAT) for b in blocks]
        assert all((w != model.argb_for_null).sum() > n // 2 for w in want)
        o = Out(ctx, "argb", [w.astype(np.uint32) for w in want], differs=True)
        call = lambda st: _st(lambda: ctx.render_cells_dev(pal, "float", blk.ptr, n, o.ptr, stream=st))
        case = Case(ctx, "gf_block_render_cells_dev", [blk], [o], call)
    else:
        lattice = (1.7, 2.6, 0.91, 1.37, 100, 100)
        if form == "lattice":
            coords = [R.lattice_coords(*lattice)] * 3
        else:
            coords = [(rng.uniform(1.0, BLOCK[0] - 2.0, 700), rng.uniform(1.0, BLOCK[1] - 2.0, 700)) for _ in range(3)]
        n = coords[0][0].size
        want = [M.render_points(spec, b, r, c, model, light) for b, (r, c) in zip(blocks, coords)]
        assert all((w["status"] == R.OK).all() and (w["shade"] != light.ambient).all() for w in want)
        outs = [Out(ctx, "argb", [w["argb"].astype(np.uint32) for w in want], differs=True),
                Out(ctx, "shade", [w["shade"] for w in want], items=[w["shade"].view(np.uint64) for w in want]),
                Out(ctx, "status", [w["status"].astype(np.int32) for w in want])]
        ptrs = {o.name: o.ptr for o in outs}
        if form == "lattice":
            call = lambda st: _st(lambda: ctx.render_lattice_dev(s, blk.ptr, lattice, pal, ptrs, li, stream=st))
            ins = [blk]
        else:
            rows, cols = Inp(ctx, "rows", [c[0] for c in coords]), Inp(ctx, "cols", [c[1] for c in coords])
            ins = [blk, rows, cols]
            call = lambda st: _st(lambda: ctx.render_points_dev(s, blk.ptr, pal, ptrs, n_points=n, d_rows=rows.ptr, d_cols=cols.ptr, light=li, stream=st))
        case = Case(ctx, "gf_block_render_%s_dev" % form, ins, outs, call)

    class _Pal:
        free = staticmethod(pal.close)
    case.extra.append(_Pal)
    return case


def downsample_case(ctx, factor=3):
    """gf_block_downsample_elems_dev on three elements (int, short, float) of one rectangle against tests/downsample_ref.py"""
    import downsample_ref as R
    from gridfour_amd.codec import _ELEM_SPEC
    rng = np.random.default_rng(4300)
    block = (4, 6, BLOCK[0], BLOCK[1])
    types = [(R.INT, -2 ** 31), (R.SHORT, -32768), (R.FLOAT, 0)]
    specs = np.zeros(3, _ELEM_SPEC)
    ins, outs = [], []
    for e, (t, fill) in enumerate(types):
        specs[e]["type"], specs[e]["fill_i"], specs[e]["scale"] = t, fill, 1.0
        if t == R.FLOAT:
            sets = [(rng.uniform(-10.0, 10.0, BLOCK) + 1000.0 * k).astype(np.float32) for k in range(3)]
        else:
            sets = [(rng.integers(-40, 41, BLOCK) + 1000 * k).astype(R.DTYPES[t]) for k in range(3)]
        want = [np.ascontiguousarray(R.downsample(v, block, factor, t, fill)) for v in sets]
        ins.append(Inp(ctx, "block%d" % e, sets))
        outs.append(Out(ctx, "coarse%d" % e, want, items=[w.reshape(-1).view({2: np.uint16, 4: np.uint32}[w.itemsize]) for w in want]))
    call = lambda st: _st(lambda: ctx.downsample_dev(specs, block, factor, [i.ptr for i in ins], [o.ptr for o in outs], stream=st))
    return Case(ctx, "gf_block_downsample_elems_dev", ins, outs, call)


def _tab_summary(dtype, d):
    a = np.zeros(1, dtype)
    for k in dtype.names:
        if k in d:
            a[k] = d[k]
    return a


def tabulate_dense_case(ctx, table, strips=False):
    """gf_block_tabulate_dense_dev against tests/tabulate_ref.py: the table in LDS or in global memory (atomics); strips: three
    calls back to back on the stream, the first initialising, the others accumulating"""
    import tabulate_cases as K
    import tabulate_ref as R
    from gridfour_amd.codec import TAB_SUMMARY
    rng = np.random.default_rng(4400)
    n = BLOCK[0] * BLOCK[1]
    window = (-300, 500, 1.0) if table == "lds" else (-300, K.LDS_MAX_BINS + 500, 1.0)
    n_bins = R.plan(*window)["n_bins"]
    assert (n_bins <= K.LDS_MAX_BINS) == (table == "lds")
    sets = [K.dem_like(rng, n, R.INT, -300 + 40 * k, 500 + 60 * k) for k in range(3)]
    want = [R.dense(v, R.INT, *window, first_cell=1000) for v in sets]
    assert all(w[0].size == n_bins for w in want)
    blk = Inp(ctx, "block", sets)
    cnt = Out(ctx, "counter", [w[0].astype(np.int32) for w in want], differs=True)
    summ = Out(ctx, "summary", [_tab_summary(TAB_SUMMARY, w[1]) for w in want], differs=True)
    cuts = [0, K.first_trip(R.INT) + 6, 2 * K.first_trip(R.INT) - 2, n] if strips else [0, n]
    assert cuts == sorted(cuts) and cuts[-2] < n

    def call(st):
        for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            status = _st(lambda: ctx.tabulate_dense_dev(R.INT, C.c_void_p(blk.ptr.value + 4 * a), b - a, *window, cnt.ptr, summ.ptr, accumulate=k > 0,
                                                        first_cell=1000 + a, stream=st))
            if status != 0:
                return status
        return 0
    return Case(ctx, "gf_block_tabulate_dense_dev[%s%s]" % (table, ", three strips" if strips else ""), [blk], [cnt, summ], call)


def tabulate_symbols_case(ctx):
    """gf_block_tabulate_symbols_dev against tests/tabulate_ref.py: the table of symbols, their counts and the scalars"""
    import tabulate_cases as K
    import tabulate_ref as R
    from gridfour_amd.codec import TAB_SYMBOLS
    rng = np.random.default_rng(4500)
    n = BLOCK[0] * BLOCK[1]
    sets = [K.dem_like(rng, n, R.INT, -300 + 40 * k, 500 + 60 * k) for k in range(3)]
    want = [R.symbols(v, R.INT) for v in sets]
    cap = n
    sym, cnt, masks = [], [], []
    for s_, c_, d in want:
        k = d["n_symbols"]
        a, b = np.zeros(cap, np.uint32), np.zeros(cap, np.int32)
        a[:k], b[:k] = s_[:k], c_[:k]
        sym.append(a), cnt.append(b), masks.append((np.arange(cap) < k).repeat(4))
    blk = Inp(ctx, "block", sets)
    outs = [Out(ctx, "symbols", sym, mask=masks, differs=True), Out(ctx, "counts", cnt, mask=masks, differs=True),
            Out(ctx, "summary", [_tab_summary(TAB_SYMBOLS, dict(w[2], n_written=w[2]["n_symbols"])) for w in want], differs=True)]
    call = lambda st: _st(lambda: ctx.tabulate_symbols_dev(R.INT, blk.ptr, n, outs[0].ptr, outs[1].ptr, cap, outs[2].ptr, stream=st))
    return Case(ctx, "gf_block_tabulate_symbols_dev", [blk], outs, call)


def gather_case(ctx, direction):
    """gf_block_from_tiles_dev (capture-safe once the slot table has its size) and gf_tiles_from_block_dev against tests/block_ref.py"""
    import block_ref as B
    rng = np.random.default_rng(4600)
    tile, grid, rect = (40, 60), (100, 200), (13, 27, 80, 150)
    nrt, nct = B.tiles_of(grid, tile)
    nt, cells, fill = nrt * nct, tile[0] * tile[1], 0x80000000
    order = rng.permutation(nt).astype(np.int32)
    idx = Inp(ctx, "indices", [order] * 3)
    g = grid + tile
    if direction == "from_tiles":
        tiles = [(rng.integers(0, 2 ** 30, (nt, cells)) + (k << 30)).astype(np.uint32) for k in range(3)]
        want = [B.block_from_tiles(grid, tile, rect, order, t, fill).astype(np.uint32) for t in tiles]
        src = Inp(ctx, "tiles", tiles)
        o = Out(ctx, "block", want, items=want)
        call = lambda st: _st(lambda: ctx.block_from_tiles_dev(g, rect, 0, fill, nt, idx.ptr, src.ptr, o.ptr, stream=st))
        return Case(ctx, "gf_block_from_tiles_dev", [idx, src], [o], call)
    blocks = [(rng.integers(0, 2 ** 30, (rect[2], rect[3])) + (k << 30)).astype(np.uint32) for k in range(3)]
    want = [B.tiles_from_block(grid, tile, rect, b, order, fill).astype(np.uint32) for b in blocks]
    inside = [w != fill for w in want]
    assert all(m.sum() == rect[2] * rect[3] for m in inside)
    src = Inp(ctx, "block", blocks)
    o = Out(ctx, "tiles", want, items=[w[m] for w, m in zip(want, inside)])
    st_o = Out(ctx, "status", [np.zeros(nt, np.int32)] * 3)
    call = lambda st: _st(lambda: ctx.tiles_from_block_dev(g, rect, 0, fill, src.ptr, nt, idx.ptr, o.ptr, st_o.ptr, stream=st))
    return Case(ctx, "gf_tiles_from_block_dev", [idx, src], [o, st_o], call)


# ------------------------------------------------------------------------------------- packings and records in one blob

def _blobs(packs_sets, gap=0):
    """per input set the packings end to end in one blob (all three blobs of one size, 32 spare bytes behind the longest):
    (blobs, offsets [n + 1] uint64, lengths uint32, blob_bytes)"""
    sizes = [sum(len(p) + gap for p in ps) for ps in packs_sets]
    total = (max(sizes) + 15) // 16 * 16 + 32
    blobs, offs, lens = [], [], []
    for ps in packs_sets:
        blob, off, pos = np.zeros(total, np.uint8), np.zeros(len(ps) + 1, np.uint64), 0
        for i, p in enumerate(ps):
            pos += gap
            off[i] = pos
            blob[pos:pos + len(p)] = np.frombuffer(p, np.uint8)
            pos += len(p)
        off[len(ps)] = pos
        blobs.append(blob), offs.append(off), lens.append(np.array([len(p) for p in ps], np.uint32))
    return blobs, offs, lens, total - 32


def _ints(a):
    a = np.ascontiguousarray(a, np.int32)
    return a, C.c_void_p(a.ctypes.data)


def inflate_case(ctx, nt=64, nr=NR, nc=NC):
    """gf_inflate_batch_dev: zlib streams of the tiles' bytes in slots of one size (the descriptor arrays are host arguments, the
    same for every input set; an Inflater stops at the end of its stream, whatever lies behind it) -> the bytes, their count, OK"""
    import zlib
    from gridfour_amd import lib
    sets = dem_sets(nt, nr, nc)
    raw = nr * nc * 4
    streams = [[zlib.compress(t.astype("<i4").tobytes(), 6) for t in s] for s in sets]
    slot = (max(len(z) for zs in streams for z in zs) + 31) // 16 * 16
    slots = [np.zeros((nt, slot), np.uint8) for _ in sets]
    for sl, zs in zip(slots, streams):
        for t, z in enumerate(zs):
            sl[t, :len(z)] = np.frombuffer(z, np.uint8)
    in_off, in_len = np.arange(nt, dtype=np.uint64) * np.uint64(slot), np.full(nt, slot, np.uint32)
    out_off, out_cap = np.arange(nt, dtype=np.uint64) * np.uint64(raw), np.full(nt, raw, np.uint32)
    d_in = Inp(ctx, "streams", slots)
    o = [Out(ctx, "bytes", sets, items=sets), Out(ctx, "produced", [np.full(nt, raw, np.uint32)] * 3), Out(ctx, "status", [np.zeros(nt, np.int32)] * 3)]
    p = lambda a: C.c_void_p(a.ctypes.data)
    call = lambda st: lib().gf_inflate_batch_dev(ctx.handle, st, nt, d_in.ptr, p(in_off), p(in_len), o[0].ptr, p(out_off), p(out_cap), o[1].ptr, o[2].ptr)
    return Case(ctx, "gf_inflate_batch_dev", [d_in], o, call)


STANDARD_LIST = (1, 2, 0, 3)                 # GF_CODEC_HUFFMAN, _DEFLATE, _NONE (CodecFloat), _CANON_HUFFMAN: the reference's default


def blob_decode_case(ctx, codec, nt=64, nr=NR, nc=NC):
    """gf_deflate_decode_batch_i32_dev, gf_float_decode_batch_f32_dev and gf_codec_master_decode_batch_i32_dev (a batch that mixes
    CodecHuffman, CodecDeflate and CodecCanonHuffman packings) on packings that lie end to end in one blob, from the oracle's
    encoders; the cells themselves are the expectation"""
    import oracle
    from gridfour_amd import lib
    L = lib()
    if codec == "float":
        sets = _float_sets(nt, nr, nc)
        packs = [[oracle.codec_float_encode(2, nr, nc, t, 6) for t in s] for s in sets]
    elif codec == "deflate":
        sets = dem_sets(nt, nr, nc)
        packs = [[oracle.codec_deflate_encode(1, nr, nc, t)[0] for t in s] for s in sets]
    else:
        sets = dem_sets(nt, nr, nc)
        enc = [lambda t: oracle.codec_huffman_encode(0, nr, nc, t)[0], lambda t: oracle.codec_deflate_encode(1, nr, nc, t)[0],
               lambda t: oracle.codec_canon_encode(3, nr, nc, t)[0]]
        packs = [[enc[(t + k) % 3](s[t]) for t in range(nt)] for k, s in enumerate(sets)]
    assert all(p is not None for ps in packs for p in ps)
    blobs, offs, lens, blob_bytes = _blobs(packs)
    d_blob, d_off, d_len = Inp(ctx, "blob", blobs), Inp(ctx, "offsets", offs), Inp(ctx, "lengths", lens)
    o = [Out(ctx, "values", sets, items=sets), Out(ctx, "status", [np.zeros(nt, np.int32)] * 3)]
    if codec == "float":
        call = lambda st: L.gf_float_decode_batch_f32_dev(ctx.handle, st, nr, nc, nt, d_blob.ptr, blob_bytes + 32, d_off.ptr, d_len.ptr, o[0].ptr, o[1].ptr)
        name = "gf_float_decode_batch_f32_dev"
    elif codec == "deflate":
        call = lambda st: L.gf_deflate_decode_batch_i32_dev(ctx.handle, st, nr, nc, nt, d_blob.ptr, blob_bytes + 32, d_off.ptr, 0, d_len.ptr, o[0].ptr, o[1].ptr)
        name = "gf_deflate_decode_batch_i32_dev"
    else:
        codecs, pc = _ints(STANDARD_LIST)
        call = lambda st: (codecs, L.gf_codec_master_decode_batch_i32_dev(ctx.handle, st, pc, 4, nr, nc, nt, d_blob.ptr, blob_bytes, d_off.ptr, d_len.ptr,
                                                                          o[0].ptr, o[1].ptr))[1]
        name = "gf_codec_master_decode_batch_i32_dev"
    return Case(ctx, name, [d_blob, d_off, d_len], o, call)


def record_decode_case(ctx, nt=64, nr=NR, nc=NC):
    """gf_tile_record_decode_batch_dev: records of one INT element, packed by the three integer codecs of the standard list in
    turn and one in four in standard form, framed as RecordManager frames them (tests/test_gpu_records_dev.py's _frame), each at
    another byte alignment: tile indices, cells, statuses"""
    import oracle
    from gridfour_amd import lib
    from test_gpu_records_dev import _frame
    sets = dem_sets(nt, nr, nc)
    enc = [lambda t: oracle.codec_huffman_encode(0, nr, nc, t)[0], lambda t: oracle.codec_deflate_encode(1, nr, nc, t)[0],
           lambda t: oracle.codec_canon_encode(3, nr, nc, t)[0], lambda t: t.astype("<i4").tobytes()]
    index = [((np.arange(nt) * 7 + 100 * k) % 5000).astype(np.int32) for k in range(3)]
    records = [[_frame(int(index[k][t]), enc[(t + k) % 4](s[t])) for t in range(nt)] for k, s in enumerate(sets)]
    blobs, offs, _, blob_bytes = _blobs(records, gap=5)
    for off, rs in zip(offs, records):                       # record t = blob[offsets[t] .. offsets[t + 1]): the filler counts to the record before
        assert all(int(off[t + 1]) - int(off[t]) >= len(r) for t, r in enumerate(rs))
    d_blob, d_off = Inp(ctx, "blob", blobs), Inp(ctx, "offsets", offs)
    o = [Out(ctx, "tile_indices", index, differs=True), Out(ctx, "values", sets, items=sets), Out(ctx, "status", [np.zeros(nt, np.int32)] * 3)]
    codecs, pc = _ints(STANDARD_LIST)
    call = lambda st: (codecs, lib().gf_tile_record_decode_batch_dev(ctx.handle, st, pc, 4, 0, nr, nc, nt, d_blob.ptr, blob_bytes, d_off.ptr, 1, o[0].ptr,
                                                                     o[1].ptr, o[2].ptr))[1]
    return Case(ctx, "gf_tile_record_decode_batch_dev", [d_blob, d_off], o, call)


# the three-element records of tests/test_gpu_blocks.py: a 100 x 200 grid in 40 x 60 tiles, (short, int-coded float, float)
TILE4, GRID4, RECT4 = (40, 60), (100, 200), (13, 27, 80, 150)
FILLS4 = [-123, None, np.float32(-7.5)]


def _record_sets():
    """three batches of twelve three-element tiles (tests/records_enc_inputs.py: its values and, from the oracle's encoders, the
    records the reference would write for the list (CodecHuffman, CodecCanonHuffman)), the tiles of the grid in shuffled order:
    per set (Batch, records, codec_used)"""
    import records_enc_inputs as RI
    key = "records"
    if key not in _MODELS:
        pool = RI.Batch(RI.ELEMS3, TILE4[0], TILE4[1], 36)
        rng = np.random.default_rng(4700)
        out = []
        for k in range(3):
            b = RI.Batch.__new__(RI.Batch)
            b.elems, b.nr, b.nc, b.nt = pool.elems, pool.nr, pool.nc, 12
            b.values = [v[12 * k:12 * k + 12] for v in pool.values]
            b.indices = rng.permutation(12).astype(np.int32)
            b._cand = {}
            out.append((b,) + b.expected((RI.HUFFMAN, RI.CANON)))
        _MODELS[key] = out
    return _MODELS[key]


def _delivered(b):
    """what a read delivers per element of a batch: int16 cells, the int-coded floats as float32, the floats"""
    import test_gpu_records_elems as RE
    return [b.values[0], RE._icf_expect(b.values[1], RE.ICF3), b.values[2]]


def _elem_args(master, fills=None):
    import records_enc_inputs as RI
    specs, dtypes = master._elem_specs(RI.ELEMS3)
    if fills is not None:
        master._fill_specs(specs, RI.ELEMS3, fills)
    return specs, dtypes


def _master(ctx):
    import gridfour_amd
    import records_enc_inputs as RI
    return gridfour_amd.CodecMasterHip(codec_list=[RI.HUFFMAN, RI.CANON], context=ctx)


def _bits32(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def records_encode_case(ctx):
    """gf_tile_record_encode_batch_elems_dev: the records byte for byte, their offsets, the codec used per element, the statuses"""
    from gridfour_amd import lib
    sets = _record_sets()
    master = _master(ctx)
    specs, _ = _elem_args(master)
    specs[0]["fill_i"] = -32768
    nt, ne = 12, 3
    cap = nt * int(lib().gf_tile_record_max_bytes_elems(C.c_void_p(specs.ctypes.data), ne, TILE4[0], TILE4[1]))
    blobs, offs, _, _ = _blobs([r for _, r, _ in sets])
    want_blob, masks = [], []
    for blob, off in zip(blobs, offs):
        w = np.zeros(cap, np.uint8)
        w[:int(off[-1])] = blob[:int(off[-1])]
        want_blob.append(w), masks.append(np.arange(cap) < int(off[-1]))
    vals = [Inp(ctx, "values%d" % e, [b.values[e] for b, _, _ in sets]) for e in range(ne)]
    idx = Inp(ctx, "tile_indices", [b.indices for b, _, _ in sets])
    o = [Out(ctx, "blob", want_blob, mask=masks, differs=True), Out(ctx, "offsets", offs, differs=True),
         Out(ctx, "codec_used", [u for _, _, u in sets]), Out(ctx, "status", [np.zeros(nt, np.int32)] * 3)]
    ptrs = (C.c_void_p * ne)(*[v.ptr.value for v in vals])
    codecs, pc = _ints(master.codecs)
    call = lambda st: (codecs, ptrs, lib().gf_tile_record_encode_batch_elems_dev(
        ctx.handle, st, pc, 2, C.c_void_p(specs.ctypes.data), ne, TILE4[0], TILE4[1], nt, idx.ptr, ptrs, 1, o[0].ptr, cap, o[1].ptr, o[2].ptr, o[3].ptr))[2]
    return Case(ctx, "gf_tile_record_encode_batch_elems_dev", vals + [idx], o, call)


def records_read_case(ctx, form, factor=3):
    """the three-element records read: gf_tile_record_decode_batch_elems_dev (the tiles), gf_block_read_elems_dev (a block, against
    tests/block_ref.py) and gf_block_read_downsampled_elems_dev (the block's box average, against tests/downsample_ref.py)"""
    import block_ref as B
    import downsample_ref as R
    from gridfour_amd import lib
    sets = _record_sets()
    master = _master(ctx)
    nt, ne = 12, 3
    blobs, offs, _, blob_bytes = _blobs([r for _, r, _ in sets], gap=3)
    d_blob, d_off = Inp(ctx, "blob", blobs), Inp(ctx, "offsets", offs)
    codecs, pc = _ints(master.codecs)
    ok = Out(ctx, "status", [np.zeros(ne * nt, np.int32)] * 3)
    tiles = [_delivered(b) for b, _, _ in sets]
    grid, rect = np.array(GRID4 + TILE4, np.int32), np.array(RECT4, np.int32)
    pg, pr = C.c_void_p(grid.ctypes.data), C.c_void_p(rect.ctypes.data)
    if form == "tiles":
        specs, _ = _elem_args(master)
        outs = [Out(ctx, "values%d" % e, [t[e] for t in tiles], differs=True) for e in range(ne)]
        o_idx = Out(ctx, "tile_indices", [b.indices for b, _, _ in sets], differs=True)
        ptrs = (C.c_void_p * ne)(*[x.ptr.value for x in outs])
        call = lambda st: (codecs, ptrs, lib().gf_tile_record_decode_batch_elems_dev(
            ctx.handle, st, pc, 2, C.c_void_p(specs.ctypes.data), ne, TILE4[0], TILE4[1], nt, d_blob.ptr, blob_bytes, d_off.ptr, 1, o_idx.ptr, ptrs,
            ok.ptr))[2]
        return Case(ctx, "gf_tile_record_decode_batch_elems_dev", [d_blob, d_off], outs + [o_idx, ok], call)
    specs, dtypes = _elem_args(master, FILLS4)
    fills = [np.int16(FILLS4[0]), np.float32(np.nan), FILLS4[2]]
    blocks = []
    for (b, _, _), t in zip(sets, tiles):
        per = []
        for e in range(ne):
            v = _bits32(t[e])
            fill = np.asarray(fills[e], t[e].dtype).reshape(1).view(v.dtype)[0]
            per.append(B.block_from_tiles(GRID4, TILE4, RECT4, b.indices, v, fill))
        blocks.append(per)
    if form == "block":
        outs = [Out(ctx, "block%d" % e, [blk[e] for blk in blocks], differs=True) for e in range(ne)]
        ptrs = (C.c_void_p * ne)(*[x.ptr.value for x in outs])
        call = lambda st: (codecs, ptrs, grid, rect, lib().gf_block_read_elems_dev(
            ctx.handle, st, pc, 2, C.c_void_p(specs.ctypes.data), ne, pg, pr, nt, d_blob.ptr, blob_bytes, d_off.ptr, 1, ptrs, ok.ptr))[4]
        return Case(ctx, "gf_block_read_elems_dev", [d_blob, d_off], outs + [ok], call)
    # downsampled: the int-coded float element is averaged as the int32 codes it is stored as, filled with its fill code
    import test_gpu_records_elems as RE
    coarse = []
    for (b, _, _), blk in zip(sets, blocks):
        codes = B.block_from_tiles(GRID4, TILE4, RECT4, b.indices, b.values[1], np.int32(RE.ICF3[3]))
        coarse.append([R.downsample(blk[0], RECT4, factor, R.SHORT, FILLS4[0]), R.downsample(codes, RECT4, factor, R.INT, RE.ICF3[3]),
                       R.downsample(blk[2].view(np.float32), RECT4, factor, R.FLOAT)])
    outs = [Out(ctx, "coarse%d" % e, [np.ascontiguousarray(c[e]) for c in coarse], differs=True) for e in range(ne)]
    ptrs = (C.c_void_p * ne)(*[x.ptr.value for x in outs])
    call = lambda st: (codecs, ptrs, grid, rect, lib().gf_block_read_downsampled_elems_dev(
        ctx.handle, st, pc, 2, C.c_void_p(specs.ctypes.data), ne, pg, pr, factor, nt, d_blob.ptr, blob_bytes, d_off.ptr, 1, ptrs, ok.ptr))[4]
    return Case(ctx, "gf_block_read_downsampled_elems_dev", [d_blob, d_off], outs + [ok], call)


def block_write_case(ctx, old):
    """gf_block_write_elems_dev: three blocks (short, int-coded float values, float) written as tile records, against
    tests/block_write_ref.py with the oracle's record writer behind it.  old False: n_old == 0, the enqueue-only form; old True: the
    twelve records of _record_sets() are what the file holds, and the partly covered tiles are merged into them (synchronises once)"""
    import block_write_ref as W
    import records_enc_inputs as RI
    from gridfour_amd import lib
    master = _master(ctx)
    specs, _ = _elem_args(master)
    master._fill_specs(specs, RI.ELEMS3, None)
    ne = 3
    rng = np.random.default_rng(4800)
    shape = RECT4[2:]
    blocks = [[(rng.integers(-300, 301, shape) + 1000 * k).astype(np.int16),
               (rng.integers(-5000, 5001, shape).astype(np.float32) / np.float32(100.0) + np.float32(-5.25 + 200.0 * k)).astype(np.float32),
               (rng.uniform(-10.0, 10.0, shape) + 1000.0 * k).astype(np.float32)] for k in range(3)]

    def encode(indices, tiles):
        b = RI.Batch.__new__(RI.Batch)
        b.elems, b.nr, b.nc, b.nt = RI.ELEMS3, TILE4[0], TILE4[1], len(indices)
        b.values, b.indices, b._cand = [np.ascontiguousarray(t) for t in tiles], np.asarray(indices, np.int32), {}
        recs, used = b.expected((RI.HUFFMAN, RI.CANON))
        return recs, used, np.zeros(len(indices), np.int32)

    sets = _record_sets()
    want = []
    for k, blk in enumerate(blocks):
        before = None
        if old:
            b = sets[k][0]
            before = {int(i): [b.values[e][t] for e in range(ne)] for t, i in enumerate(b.indices)}
        want.append(W.expected(encode, GRID4, TILE4, RECT4, blk, RI.ELEMS3, before=before))
    n_out = want[0][0].size
    assert n_out == 9 and all((w[4] == 0).all() for w in want)
    cap = n_out * int(lib().gf_tile_record_max_bytes_elems(C.c_void_p(specs.ctypes.data), ne, TILE4[0], TILE4[1]))
    w_blob, masks = [], []
    for w in want:
        joined = np.frombuffer(b"".join(w[1]), np.uint8)
        a = np.zeros(cap, np.uint8)
        a[:joined.size] = joined
        w_blob.append(a), masks.append(np.arange(cap) < joined.size)
    ins = [Inp(ctx, "block%d" % e, [blk[e] for blk in blocks]) for e in range(ne)]
    ptrs = (C.c_void_p * ne)(*[i.ptr.value for i in ins])
    o = [Out(ctx, "blob", w_blob, mask=masks, differs=True), Out(ctx, "offsets", [w[2] for w in want], differs=True),
         Out(ctx, "tile_indices", [w[0].astype(np.int32) for w in want]), Out(ctx, "codec_used", [w[3].astype(np.uint8) for w in want]),
         Out(ctx, "status", [w[4].astype(np.int32) for w in want])]
    grid, rect = np.array(GRID4 + TILE4, np.int32), np.array(RECT4, np.int32)
    pg, pr, ps = C.c_void_p(grid.ctypes.data), C.c_void_p(rect.ctypes.data), C.c_void_p(specs.ctypes.data)
    codecs, pc = _ints(master.codecs)
    n_old, o_blob, o_bytes, o_off = 0, None, 0, None
    if old:
        blobs, offs, _, o_bytes = _blobs([r for _, r, _ in sets], gap=3)
        d_oblob, d_ooff = Inp(ctx, "old_blob", blobs), Inp(ctx, "old_offsets", offs)
        ins += [d_oblob, d_ooff]
        n_old, o_blob, o_off = 12, d_oblob.ptr, d_ooff.ptr
    call = lambda st: (codecs, ptrs, grid, rect, specs, lib().gf_block_write_elems_dev(
        ctx.handle, st, pc, 2, ps, None, ne, pg, pr, ptrs, n_old, o_blob, o_bytes, o_off, 1, 1, o[0].ptr, cap, o[1].ptr, o[2].ptr, o[3].ptr, o[4].ptr))[5]
    return Case(ctx, "gf_block_write_elems_dev[%s]" % ("old records" if old else "n_old == 0"), ins, o, call)


def chain_case(ctx):
    """five families back to back on one stream, no host synchronisation between them: a block written as records (n_old == 0), a
    downsample, an interpolated lattice, rendered cells, a dense tabulation with its table in global memory -- the scratch buffers
    of the context that the families share, on a caller's stream"""
    parts = [block_write_case(ctx, False), downsample_case(ctx), interp_case(ctx, "lattice"), render_case(ctx, "cells"),
             tabulate_dense_case(ctx, "global")]

    def call(st):
        for p in parts:
            status = p.call(st)
            if status != 0:
                return status
        return 0
    case = Case(ctx, "chain of " + ", ".join(p.name for p in parts), [i for p in parts for i in p.inputs], [o for p in parts for o in p.outputs], call)
    case.extra = [x for p in parts for x in p.extra]
    return case


# ---------------------------------------------------------------------------------------------------------------- the table

CAPTURE, ENQUEUE, SYNC_ONCE, STREAM_ONLY = "capture", "enqueue", "sync_once", "stream_only"


class Row:
    """one entry point: the class the header's own sentence gives it, and its cases: (id, class, builder(ctx) -> Case) -- a function
    whose class depends on its arguments (gf_lsop12_decode_batch_i32_dev, gf_block_write_elems_dev) has cases of both classes"""

    def __init__(self, name, kind, cases):
        self.name, self.kind, self.cases = name, kind, cases


def _c(ident, builder, kind=None):
    return (ident, kind, builder)


TABLE = [
    Row("gf_huffman_encode_batch_i32_dev", CAPTURE, [_c("t64", lambda c: encode_case(c, "huffman", 64)), _c("t256", lambda c: encode_case(c, "huffman", 256)),
                                                     _c("t1", lambda c: encode_case(c, "huffman", 1)), _c("t1024", lambda c: encode_case(c, "huffman", 1024))]),
    Row("gf_huffman_decode_batch_i32_dev", CAPTURE, [_c("t64", lambda c: decode_case(c, "huffman", 64)), _c("t256", lambda c: decode_case(c, "huffman", 256)),
                                                     _c("t1", lambda c: decode_case(c, "huffman", 1)), _c("t1024", lambda c: decode_case(c, "huffman", 1024)),
                                                     _c("side_stream", roomy_case)]),
    Row("gf_canon_encode_batch_i32_dev", CAPTURE, [_c("t64", lambda c: encode_case(c, "canon", 64)), _c("t256", lambda c: encode_case(c, "canon", 256))]),
    Row("gf_canon_decode_batch_i32_dev", CAPTURE, [_c("t64_via_fast", lambda c: decode_case(c, "canon", 64, route=canon_fast_route)),
                                                   _c("t256", lambda c: decode_case(c, "canon", 256)), _c("t1", lambda c: decode_case(c, "canon", 1)),
                                                   _c("t1024", lambda c: decode_case(c, "canon", 1024)), _c("t4160", canon_many_case)]),
    Row("gf_compact_dev", CAPTURE, [_c("t64", lambda c: compact_case(c, 64))]),
    Row("gf_m32_encode_batch_i32_dev", CAPTURE, [_c("t64", lambda c: m32_encode_case(c, 64))]),
    Row("gf_m32_decode_batch_i32_dev", CAPTURE, [_c("t64", lambda c: decode_case(c, "m32", 64))]),
    Row("gf_lsop12_predict_dev", CAPTURE, [_c("t64", lambda c: lsop_stage_case(c, "predict"))]),
    Row("gf_lsop12_reconstruct_dev", CAPTURE, [_c("t64", lambda c: lsop_stage_case(c, "reconstruct"))]),
    Row("gf_lsop12_encode_batch_i32_dev", CAPTURE, [_c("t64", lambda c: lsop_encode_case(c, False))]),
    Row("gf_lsop12_encode_batch_i32_dev_ex", CAPTURE, [_c("checksum", lambda c: lsop_encode_case(c, True))]),
    Row("gf_lsop12_decode_batch_i32_dev", CAPTURE, [_c("current", lambda c: lsop_decode_case(c, "current")), _c("legacy", lambda c: lsop_decode_case(c, "legacy")),
                                                    _c("deflate", lambda c: lsop_decode_case(c, "deflate"), SYNC_ONCE)]),
    Row("gf_float_planes_encode_dev", CAPTURE, [_c("t64", lambda c: float_planes_case(c, "encode"))]),
    Row("gf_float_planes_decode_dev", CAPTURE, [_c("t64", lambda c: float_planes_case(c, "decode"))]),
    Row("gf_synth_dem_dev", CAPTURE, [_c("t64", lambda c: synth_case(c, ""))]),
    Row("gf_synth_dem_masked_dev", CAPTURE, [_c("t64", lambda c: synth_case(c, "_masked"))]),
    Row("gf_synth_dem_style_dev", CAPTURE, [_c("t64", lambda c: synth_case(c, "_style"))]),
    Row("gf_block_interp_points_dev", CAPTURE, [_c("b100x150", lambda c: interp_case(c, "points"))]),
    Row("gf_block_interp_lattice_dev", CAPTURE, [_c("b100x150", lambda c: interp_case(c, "lattice"))]),
    Row("gf_block_render_cells_dev", CAPTURE, [_c("b100x150", lambda c: render_case(c, "cells"))]),
    Row("gf_block_render_lattice_dev", CAPTURE, [_c("b100x150", lambda c: render_case(c, "lattice"))]),
    Row("gf_block_render_points_dev", CAPTURE, [_c("b100x150", lambda c: render_case(c, "points"))]),
    Row("gf_block_downsample_elems_dev", CAPTURE, [_c("b100x150_f3", downsample_case)]),
    Row("gf_block_tabulate_dense_dev", CAPTURE, [_c("lds", lambda c: tabulate_dense_case(c, "lds")), _c("global", lambda c: tabulate_dense_case(c, "global")),
                                                 _c("lds_strips", lambda c: tabulate_dense_case(c, "lds", True)),
                                                 _c("global_strips", lambda c: tabulate_dense_case(c, "global", True))]),
    Row("gf_block_tabulate_symbols_dev", ENQUEUE, [_c("b100x150", tabulate_symbols_case)]),
    Row("gf_block_from_tiles_dev", CAPTURE, [_c("g100x200", lambda c: gather_case(c, "from_tiles"))]),
    Row("gf_tiles_from_block_dev", CAPTURE, [_c("g100x200", lambda c: gather_case(c, "from_block"))]),
    Row("gf_inflate_batch_dev", SYNC_ONCE, [_c("s64", inflate_case)]),
    Row("gf_deflate_decode_batch_i32_dev", SYNC_ONCE, [_c("t64", lambda c: blob_decode_case(c, "deflate"))]),
    Row("gf_float_decode_batch_f32_dev", SYNC_ONCE, [_c("t64", lambda c: blob_decode_case(c, "float"))]),
    Row("gf_codec_master_decode_batch_i32_dev", SYNC_ONCE, [_c("mixed64", lambda c: blob_decode_case(c, "master"))]),
    Row("gf_tile_record_decode_batch_dev", SYNC_ONCE, [_c("mixed64", record_decode_case)]),
    Row("gf_tile_record_decode_batch_elems_dev", SYNC_ONCE, [_c("three", lambda c: records_read_case(c, "tiles"))]),
    Row("gf_tile_record_encode_batch_elems_dev", ENQUEUE, [_c("three", records_encode_case)]),
    Row("gf_block_read_elems_dev", SYNC_ONCE, [_c("three", lambda c: records_read_case(c, "block"))]),
    Row("gf_block_read_downsampled_elems_dev", SYNC_ONCE, [_c("three_f3", lambda c: records_read_case(c, "downsampled"))]),
    Row("gf_block_write_elems_dev", ENQUEUE, [_c("n_old_0", lambda c: block_write_case(c, False)),
                                              _c("old_records", lambda c: block_write_case(c, True), SYNC_ONCE)]),
    Row("gf_timer_start", STREAM_ONLY, []),              # test_timer_on_a_callers_stream
    Row("gf_timer_stop", STREAM_ONLY, []),
]

# Entry points with a class from the header's sentence and no case: none (tests/test_caller_stream_table.py keeps it empty)
NOT_COVERED = {}


def cases(kinds):
    """(pytest id, Row, case class, builder) of every case whose class is one of kinds"""
    out = []
    for row in TABLE:
        for ident, kind, builder in row.cases:
            if (kind or row.kind) in kinds:
                out.append(("%s-%s" % (row.name, ident), row, kind or row.kind, builder))
    return out
