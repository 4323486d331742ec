"""GVRS file images inspected on the GPU.  gf_file_inspect_dev is held to gf_file_inspect (which tests/test_file_inspect_host.py holds
to the sequential restatement) on the reference's sample files and on every image of tests/inspect_cases.py: report, bad tiles
and records.  The cases are built around the device form's seams -- records across and on segment seams, segments without an
anchor, anchors behind unnamed records, false anchors, links that do not close, records of more chunks than one wave takes --
with sizes taken from gf_file_inspect_plan.  Then its capacity rules with guard bytes behind every output, images the library
itself wrote and updated, and that the call only enqueues."""
import collections
import glob
import os

import numpy as np
import pytest

import gridfour_amd
from gridfour_amd import GvrsFileHip, _lib
from gridfour_amd.codec import _FILE_INSPECT_REPORT, _FILE_RECORD, _DeviceScope

import gvrs_file_build as B
import gvrs_file_write_ref as W
import gvrs_inspect_ref as R
import gvrs_walk
import inspect_cases as K

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SAMPLES = sorted(glob.glob(os.path.join(HERE, "golden", "ref_samples", "*.gvrs")))


@pytest.fixture(scope="module")
def ctx():
    return gridfour_amd.GvrsHipContext()


def dev_equals_host(ctx, image, name):
    f = GvrsFileHip(image)
    want = f.inspect()
    got = f.inspect_dev(ctx)
    assert got.report() == want.report(), name
    assert got.bad_tiles == want.bad_tiles and got.records == want.records, name
    assert got.guards_intact, name
    return got


def test_samples(ctx):
    assert len(SAMPLES) == 15
    for path in SAMPLES:
        got = dev_equals_host(ctx, open(path, "rb").read(), path)
        assert got.passed and got.complete


@pytest.mark.parametrize("name", sorted(K.all_cases()))
def test_cases(ctx, name):
    got = dev_equals_host(ctx, K.all_cases()[name], name)
    if name.startswith("sound"):
        assert got.passed and got.complete


def test_another_image_than_the_opened_one(ctx):
    """truncations around a record's end: fewer than 13 bytes behind it end the walk, more cut a record short"""
    image = K.all_cases()["sound: shuffled"]
    f = GvrsFileHip(image)
    recs = f.inspect().records
    end = recs[-2][0] + recs[-2][1]
    for n in (f.info["content_pos"], f.info["content_pos"] + 8, end, end + 8, end + 12, end + 13, end + 16, len(image) - 1):
        want, got = f.inspect(image[:n]), f.inspect_dev(ctx, image[:n])
        assert got.report() == want.report() and got.records == want.records and got.guards_intact, n


def test_capacity(ctx):
    image = K.all_cases()["damaged: a good record between"]
    f = GvrsFileHip(image)
    want = f.inspect()
    n = want.n_records
    st, got = f.inspect_dev(ctx, max_records=n - 1, return_code=True)
    assert st == _lib.ERR_CAPACITY and got.status == _lib.ERR_CAPACITY and got.n_records == n
    assert got.guards_intact and (got.records_raw == 0x7f).all(), "a failed call wrote into the list or the records"
    got = f.inspect_dev(ctx, max_records=n)
    assert got.report() == want.report() and got.records == want.records and got.guards_intact
    got = f.inspect_dev(ctx, max_records=3)                        # the binding asks once more with the count the report names
    assert got.report() == want.report() and got.records == want.records
    assert want.n_bad_tiles == 2
    for cap in (0, 1, 2):
        got = f.inspect_dev(ctx, bad_cap=cap)
        assert got.n_bad_tiles == 2 and got.bad_tiles == want.bad_tiles[:cap] and got.guards_intact, cap
    got = f.inspect_dev(ctx, with_records=False)
    assert got.report() == want.report() and got.bad_tiles == want.bad_tiles and got.records is None
    # a stop behind which the walk would need more room than it has: the count is the walk's, up to its structural stop
    hurt = K.all_cases()["damaged: tile and tile"]
    g = GvrsFileHip(hurt)
    st, got = g.inspect_dev(ctx, max_records=g.inspect().n_records, return_code=True)
    assert st == _lib.ERR_CAPACITY and got.n_records == f.inspect(K.all_cases()["sound: shuffled"]).n_records


def counts_by_type(image):
    c = collections.Counter(w[2] for w in gvrs_walk.walk_records(image))
    return [c.get(k, 0) for k in range(7)]


def test_images_the_library_made(ctx):
    grid = (4 * 5 - 1, 5 * 6 - 2, 4, 5)
    elements = [B.element("z", "int", fill=-9999), B.element("s", "short", fill=-1), B.element("c", "icf", fill=-2 ** 31, scale=4.0, offset=8.0)]
    for checksums in (True, False):
        s = W.spec(grid, elements, ["GvrsHuffman"], checksums, time_modified=5)
        rng = np.random.default_rng(3)
        rasters = [rng.integers(-500, 500, grid[:2]).astype(np.int32), rng.integers(-300, 300, grid[:2]).astype(np.int16),
                   (rng.integers(-4000, 4000, grid[:2]) / 4.0).astype(np.float32)]
        image, idx, status, _ = GvrsFileHip.write_image(ctx, W.lib_facts(s), rasters)
        assert (status == _lib.OK).all()
        got = dev_equals_host(ctx, image, "written")
        assert got.passed and got.complete and got.termination_pos == len(image) and got.tile_dir_passed == int(checksums)
        assert got.n_by_type == counts_by_type(image) and got.n_by_type[2] == 30 and got.n_by_type[5] == 1 and got.n_by_type[0] == 0
        f = GvrsFileHip(image)
        u = f.update_begin()
        rect = (4, 10, 8, 10)
        new = [r[4:12, 10:20][::-1].copy() for r in rasters]
        updated, _, ustatus, _ = f.update_image(ctx, u, rect, new, 1_700_000_000_123)
        assert (ustatus == _lib.OK).all()
        got = dev_equals_host(ctx, updated, "updated")
        assert got.passed and got.complete and got.termination_pos == len(updated)
        assert got.n_by_type == counts_by_type(updated) and got.n_by_type[2] == 30 and got.n_by_type[0] >= 1 and got.n_by_type[3] == 1


def test_two_calls_only_enqueue(ctx):
    """Behind a backlog of memsets on the context's stream two calls on different images, enqueued back to back, must return while
    the backlog still runs: an event recorded behind them is not ready.  Both reports are then the host form's."""
    import caller_stream as CS
    from gridfour_amd.codec import lib
    S = CS.Stream(ctx.stream)
    images = [K.all_cases()["sound: long both"], K.all_cases()["damaged: tile and metadata"]]
    files = [GvrsFileHip(i) for i in images]
    wants = [f.inspect() for f in files]
    room = max(w.n_records for w in wants) + 8
    with _DeviceScope(ctx) as s:
        backlog = s.alloc(1 << 30)
        d_images = [s.upload(np.frombuffer(i, np.uint8), slack=32, fill=0) for i in images]
        d_reports = [s.alloc(_FILE_INSPECT_REPORT.itemsize + 16, fill=0x7f) for _ in images]
        d_bad = [s.alloc(64, fill=0x7f) for _ in images]
        d_recs = [s.alloc(room * _FILE_RECORD.itemsize, fill=0x7f) for _ in images]

        def call(k):
            return lib().gf_file_inspect_dev(ctx.handle, files[k]._h, d_images[k].ptr, len(images[k]), room, d_reports[k].ptr, d_bad[k].ptr, 8,
                                             d_recs[k].ptr)

        assert call(0) == _lib.OK and call(1) == _lib.OK           # warm-up: module load, the context's buffer
        ctx.synchronize()
        for d in d_reports:
            d.fill(0x7f)
        ctx.synchronize()
        for _ in range(64):
            S.memset(backlog.ptr, 0, 1 << 30)
        assert call(0) == _lib.OK and call(1) == _lib.OK
        e = S.event()
        S.record(e)
        ready = CS.hip().hipEventQuery(e)
        ctx.synchronize()
        assert ready == CS.HIP_NOT_READY, "the calls returned only when the stream had drained (or the backlog was too short)"
        for k, want in enumerate(wants):
            report = d_reports[k].download(np.uint8, _FILE_INSPECT_REPORT.itemsize).view(_FILE_INSPECT_REPORT)[0]
            got = gridfour_amd.GvrsInspection(report, d_bad[k].download(np.int32, 16), 8, d_recs[k].download(np.uint8, room * _FILE_RECORD.itemsize)
                                              .view(_FILE_RECORD), room)
            assert got.report() == want.report() and got.bad_tiles == want.bad_tiles and got.records == want.records and got.guards_intact, k
    for e in S._events:
        CS.hip().hipEventDestroy(e)
