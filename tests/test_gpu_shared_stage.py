"""Every host-memory form stages through ONE buffer of the context (gf_context::dStage, gridfour_amd/csrc/gvrs_stage.h).  What
sharing one buffer can break and separate buffers could not: a result that depends on what staged before, a "zero" that is an
earlier call's bytes, and recorded one-tile graphs that outlive a buffer that moved.  The inputs are small (a 20 x 28 grid in
8 x 8 tiles, 50 points, a 9 x 11 image, 3 records of 2 elements) and come from the builders of the other tests; every
comparison is bit for bit."""
import numpy as np
import pytest

import damage
import downsample_cases as DK
import downsample_ref as DR
import image_cases as IK
import interp_cases as K
import interp_ref as R
import records_enc_inputs as RI
import render_cases as RC
import scratch_plan as sp
import tabulate_cases as TK
from test_gpu_block_write import rasters

pytestmark = pytest.mark.gpu
GRID, TILE, RECT = (20, 28), (8, 8), (0, 0, 20, 28)
ELEMS, FILLS = ["int", "short", "float"], [0, None, 0.0]
DEVICE_LIST = (RI.HUFFMAN, RI.CANON)
HOST_LIST = (RI.HUFFMAN, RI.DEFLATE, RI.NONE, RI.CANON, RI.LSOP)    # needs the host's zlib: the float, LSOP and codec-master host encoders
REC_ELEMS, REC_SHAPE = ["int", "short"], (16, 20)


def _freeze(x):
    """a result as something that compares bit for bit"""
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, np.ascontiguousarray(x).tobytes())
    if isinstance(x, dict):
        return tuple((k, _freeze(x[k])) for k in sorted(x))
    if isinstance(x, (list, tuple)):
        return tuple(_freeze(v) for v in x)
    if isinstance(x, (float, np.floating)):
        return np.float64(x).tobytes()
    return x


def _blob(records):
    off = np.zeros(len(records) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in records])
    return np.frombuffer(b"".join(records) + b"\0" * 16, np.uint8)[:int(off[-1])], off


def _tiles(seed, nr, nc, n):
    import oracle
    return oracle.dem_tiles(oracle.DEM_SEED + seed, nr, nc, 16, 0, n)


def build_inputs():
    """what the small calls take"""
    import gridfour_amd
    ctx = gridfour_amd.GvrsHipContext(0)
    rng = np.random.default_rng(4100)
    x = {}
    x["rasters"] = rasters(ELEMS, GRID)
    master = gridfour_amd.CodecMasterHip(codec_list=list(DEVICE_LIST), context=ctx)
    _, records, _, status = master.write_block(TILE[0], TILE[1], GRID, RECT, x["rasters"], ELEMS, fills=FILLS)
    assert (status == 0).all() and len(records) == 12
    x["block_records"] = _blob(records)
    x["old_records"] = _blob(records[:5])
    x["batch"] = RI.Batch(REC_ELEMS, REC_SHAPE[0], REC_SHAPE[1], 3)
    recs, _ = master.tile_records_elems(REC_SHAPE[0], REC_SHAPE[1], x["batch"].indices, x["batch"].values, REC_ELEMS)
    x["records"] = recs
    x["spec"] = R.Spec(12, 14, (2, 3, 7, 9), R.FLOAT, 0, wrap=0, target=R.SECOND, row_spacing=1.25, col_spacing=0.8)
    x["block"] = K.random_block(rng, R.FLOAT, (7, 9))
    x["rows"], x["cols"] = rng.uniform(2.0, 9.0, 50), rng.uniform(3.0, 12.0, 50)
    x["spacing"] = rng.uniform(0.5, 2.0, 50)
    x["render_spec"] = R.Spec(12, 14, (2, 3, 7, 9), R.SHORT, -7, row_spacing=1.25, col_spacing=0.8)
    x["render_block"] = (K.random_block(rng, R.SHORT, (7, 9), -7).astype(np.int64) % 90 - 10).astype(np.int16)
    ds_block = (3, 5, 20, 28)
    x["ds_block"] = ds_block
    x["ds_values"] = [DK.random_block(rng, ds_block, 3, DR.FLOAT), DK.random_block(rng, ds_block, 3, DR.SHORT, -32768)]
    x["cells"] = TK.dem_like(rng, 20 * 28, DR.SHORT)
    x["image"] = IK.random_words(rng, 9 * 11).reshape(9, 11)
    x["tiles"] = _tiles(41, 16, 20, 3)
    x["huffman"] = [p for p in gridfour_amd.CodecHuffmanHip(context=ctx).encode_batch(0, 16, 20, x["tiles"])[0]]
    x["canon"] = [p for p in gridfour_amd.CodecCanonHuffmanHip(context=ctx).encode_batch(0, 16, 20, x["tiles"])[0]]
    x["lsop"] = gridfour_amd.LsCodecHip(context=ctx).encode_batch(4, 16, 20, x["tiles"])[0]
    assert all(p for p in x["huffman"] + x["canon"] + x["lsop"])
    x["floats"] = (x["tiles"].astype(np.float32) * np.float32(0.1)).astype(np.float32)
    ctx.close()
    return x


@pytest.fixture(scope="module")
def inputs():
    """built once, on a context of its own, and left unchanged"""
    return build_inputs()


def _small_calls(x):
    """name -> call(ctx): one small call of every host form that stages through the context"""
    import gridfour_amd
    G = gridfour_amd

    def master(ctx, codecs):
        return G.CodecMasterHip(codec_list=list(codecs), context=ctx)

    def analyze(cls, packs):
        def run(ctx):
            codec = cls(context=ctx)
            status = codec.analyze_batch(16, 20, packs)
            more = codec.pair_counts() if cls is G.CodecHuffmanHip else codec.escape_counts()
            return status, codec.analysis_data().tobytes(), more
        return run

    def render(ctx):
        pal = G.Palette(ctx, **RC.lib_palette_args("hsv"))
        try:
            return ctx.render_lattice(K.lib_spec(x["render_spec"]), x["render_block"], (2.2, 3.1, 0.23, 0.11, 5, 7), pal,
                                      RC.lib_light(RC.LIGHTS["cog"]))
        finally:
            pal.close()

    def tab_dense(ctx):
        first = ctx.tabulate_dense("short", x["cells"][:300], *TK.REF_RANGE)
        return first, ctx.tabulate_dense("short", x["cells"][300:], *TK.REF_RANGE, first_cell=300, into=first)    # (... and accumulating)

    blob, off = x["block_records"]
    rec_blob, rec_off = _blob(x["records"])
    return {
        "interp_points": lambda c: c.interp_points(K.lib_spec(x["spec"]), x["block"], x["rows"], x["cols"], x["spacing"]),
        "render_lattice": render,
        "downsample": lambda c: c.downsample(["float", "short"], x["ds_block"], 3, x["ds_values"], fills=[None, -32768]),
        "read_downsampled": lambda c: master(c, DEVICE_LIST).read_block_downsampled(TILE[0], TILE[1], GRID, RECT, 2, blob, off, ELEMS, fills=FILLS),
        "tabulate_dense": tab_dense,
        "tabulate_symbols": lambda c: c.tabulate_symbols("short", x["cells"]),
        "tabulate_symbols_short_table": lambda c: c.tabulate_symbols("short", x["cells"], table_cap=7),
        "image_split": lambda c: c.image_split(x["image"], "ycocg", "short"),
        "image_join": lambda c: c.image_join(c.image_split(x["image"], "rgb", "int"), "rgb", "int"),
        "image_reduce": lambda c: c.image_reduce(x["image"], 2),
        "block_read": lambda c: master(c, DEVICE_LIST).read_block(TILE[0], TILE[1], GRID, RECT, blob, off, ELEMS, fills=FILLS),
        "records_decode": lambda c: master(c, DEVICE_LIST).record_blob_elems(REC_SHAPE[0], REC_SHAPE[1], rec_blob, rec_off, REC_ELEMS),
        "records_encode": lambda c: master(c, DEVICE_LIST).tile_records_elems(REC_SHAPE[0], REC_SHAPE[1], x["batch"].indices, x["batch"].values,
                                                                              REC_ELEMS),
        "block_write": lambda c: master(c, DEVICE_LIST).write_block(TILE[0], TILE[1], GRID, RECT, x["rasters"], ELEMS, fills=FILLS),
        "block_write_over_old": lambda c: master(c, DEVICE_LIST).write_block(TILE[0], TILE[1], GRID, (3, 5, 9, 11),
                                                                             [np.ascontiguousarray(a[3:12, 5:16]) for a in x["rasters"]], ELEMS,
                                                                             fills=FILLS, old=x["old_records"]),
        "block_write_host_list": lambda c: master(c, HOST_LIST).write_block(TILE[0], TILE[1], GRID, RECT, x["rasters"], ELEMS, fills=FILLS),
        "huffman_analyze": analyze(G.CodecHuffmanHip, x["huffman"]),
        "canon_analyze": analyze(G.CodecCanonHuffmanHip, x["canon"]),
        "lsop_encode": lambda c: G.LsCodecHip(context=c).encode_batch(4, 16, 20, x["tiles"]),
        "lsop_encode_no_deflate": lambda c: G.LsCodecHip(context=c, deflate_enabled=False).encode_batch(4, 16, 20, x["tiles"]),
        "lsop_decode": lambda c: G.LsCodecHip(context=c).decode_batch(16, 20, x["lsop"]),
        "float_encode": lambda c: G.CodecFloatHip(context=c, level=6).encode_floats_batch(2, 16, 20, x["floats"]),
    }


def _grow(ctx):
    """a call whose staging exceeds what any small call asks for (the pair tables of the Huffman analysis: 1.5 MB): gf_image_reduce
    of a 1,024 x 1,024 image, 4 MB in.  Every byte of it is non-zero, and so is every byte of the reduced image behind it."""
    big = np.full((1024, 1024), 0x7f7f7f7f, np.uint32)
    assert (ctx.image_reduce(big, 2).view(np.uint32) == 0xff7f7f7f).all()


def test_results_do_not_depend_on_what_staged_before(inputs):
    import gridfour_amd
    calls = _small_calls(inputs)
    fresh = {}
    for name, call in calls.items():
        ctx = gridfour_amd.GvrsHipContext(0)
        fresh[name] = _freeze(call(ctx))
        ctx.close()
    ctx = gridfour_amd.GvrsHipContext(0)
    for name, call in calls.items():
        assert _freeze(call(ctx)) == fresh[name], ("first round", name)
    _, held, moves = sp.context_scratch(ctx)
    _grow(ctx)
    _, held_after, moves_after = sp.context_scratch(ctx)
    assert moves_after > moves and held_after > held, "the probe is blind: the large call moved no buffer"
    for name, call in calls.items():
        assert _freeze(call(ctx)) == fresh[name], ("after the stage grew", name)
    for name in reversed(list(calls)):
        assert _freeze(calls[name](ctx)) == fresh[name], ("in the other order", name)
    assert sp.context_scratch(ctx)[1:] == (held_after, moves_after), "a small call after the large one moved a buffer"
    ctx.close()


def test_a_failed_element_reads_as_zeros_in_a_dirty_stage(inputs):
    """the stage full of 0x7f bytes, then a batch whose middle record has a flipped bit in its record type: it is no tile record,
    both of its elements read as zeros and its tile index stays what the caller handed in"""
    import gridfour_amd
    ctx = gridfour_amd.GvrsHipContext(0)
    master = gridfour_amd.CodecMasterHip(codec_list=list(DEVICE_LIST), context=ctx)
    nr, nc = REC_SHAPE
    good = master.record_blob_elems(nr, nc, *_blob(inputs["records"]), REC_ELEMS)
    assert not good[2].any() and np.array_equal(good[0], inputs["batch"].indices)
    hurt = list(inputs["records"])
    hurt[1] = damage._flip(hurt[1], 8 * 4)                                       # RecordType.Tile (2) -> 3
    _grow(ctx)
    idx, values, status = master.record_blob_elems(nr, nc, *_blob(hurt), REC_ELEMS)
    assert status[:, 1].tolist() == [gridfour_amd.ERR_FORMAT] * 2 and not status[:, (0, 2)].any()
    assert idx.tolist() == [int(good[0][0]), -1, int(good[0][2])]                # (the wrapper hands in -1)
    for e in range(2):
        assert not values[e][1].any(), e
        assert np.array_equal(values[e][(0, 2), :], good[1][e][(0, 2), :]), e
    ctx.close()


def test_pair_counts_add_exactly_once_per_run(inputs):
    """gf_huffman_analyze_batch_h2 twice in a row on a stage that held other bytes: the second run adds the first run's pair counts
    again, and nothing that the first run left in the stage"""
    import gridfour_amd
    ctx = gridfour_amd.GvrsHipContext(0)
    _grow(ctx)
    codec = gridfour_amd.CodecHuffmanHip(context=ctx)
    assert not codec.analyze_batch(16, 20, inputs["huffman"]).any()
    once, stats_once = codec.pair_counts(), codec.analysis_data()
    assert once[5].sum() > 0 and np.array_equal(once[5], once[:5].sum(axis=0))
    assert not codec.analyze_batch(16, 20, inputs["huffman"]).any()
    assert np.array_equal(codec.pair_counts(), 2 * once)
    assert [int(r["n_tiles"]) for r in codec.analysis_data()] == [2 * int(r["n_tiles"]) for r in stats_once]
    ctx.close()


@pytest.mark.parametrize("cls", ["CodecHuffmanHip", "CodecCanonHuffmanHip"])
def test_one_tile_graphs_survive_a_growing_stage(cls, inputs):
    """three one-tile encode and decode calls (the graphs are recorded and replayed), a host form that grows the stage (hipFree +
    hipMalloc: the context's move count rises), the same one-tile calls again"""
    import gridfour_amd
    import oracle
    codec = getattr(gridfour_amd, cls)(device=0)
    enc_ref = oracle.codec_huffman_encode if cls == "CodecHuffmanHip" else oracle.codec_canon_encode
    nr, nc = 120, 150
    few = oracle.dem_tiles(oracle.DEM_SEED + 31, nr, nc, 64, 0, 3)
    ref = [enc_ref(0, nr, nc, few[t])[0] for t in range(3)]

    def one_tile_calls():
        for t in range(3):
            assert codec.encode(0, nr, nc, few[t]) == ref[t], t
            assert np.array_equal(np.asarray(codec.decode(nr, nc, ref[t])).reshape(-1), few[t].reshape(-1)), t

    for _ in range(3):
        one_tile_calls()
    codec.ctx.image_reduce(inputs["image"], 2)                                  # (the stage at its first size)
    one_tile_calls()
    moves = sp.context_scratch(codec.ctx)[2]
    _grow(codec.ctx)
    assert sp.context_scratch(codec.ctx)[2] > moves
    for _ in range(2):
        one_tile_calls()
    codec.ctx.close()
