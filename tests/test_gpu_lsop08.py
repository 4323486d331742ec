"""GPU tests of the LSOP08 path (gf_lsop08_* of the C ABI) against the Python restatement tests/lsop08_ref.py: coefficients bit for bit,
both residual streams, reconstruction, the device encoder's Huffman container, the host encoder's choice, both container types in both
header revisions, damaged and truncated packings, batch sizes around the kernels' grid cap."""
import functools
import struct

import numpy as np
import pytest

import lsop08_ref as R
import oracle
from tilegen import make_tile

pytestmark = pytest.mark.gpu

OK, DECLINED, ERR_FORMAT, ERR_BOUNDS = 0, 1, -1, -2
GRID_CAP = 32768                 # GF_LSOP8_GRID_CAP (gvrs_kernels.h): the three LSOP08 kernels launch at most this many workgroups

SHAPES = [(4, 4), (4, 5), (5, 4), (7, 9), (16, 16), (33, 65), (65, 66), (66, 5), (5, 66), (129, 4), (4, 129), (3, 9), (9, 3)]
KINDS = ("terrain0", "terrain1", "smooth", "noise16", "noise32", "sparse_big", "uniform", "ramp")
ids = lambda s: "%dx%d" % s


@pytest.fixture(scope="module")
def codec():
    import gridfour_amd
    return gridfour_amd.LsCodec08Hip()


def tile(kind, nr, nc):
    if kind.startswith("terrain"):
        return R.terrain(nr, nc, int(kind[7:]))
    return make_tile(kind, nr, nc)


def R_smooth(nr, nc):
    """the smooth terrain of the LSOP12 numeric tests"""
    import lsop_ref
    return lsop_ref.smooth(nr, nc)


@functools.lru_cache(maxsize=None)
def ref(kind, nr, nc):
    """The restatement's output for a tile, computed once per module: (tile, predict() or None, type-0 packing, type-1 packing, chosen type)."""
    v = tile(kind, nr, nc)
    pr = R.predict(nr, nc, v)
    if pr is None:
        return v, None, None, None, None
    p0, p1 = R.encode(6, nr, nc, v, force_type=0)[0], R.encode(6, nr, nc, v, force_type=1)[0]
    return v, pr, p0, p1, 0 if len(p0) < len(p1) else 1


def tiles_of(nr, nc):
    return np.stack([ref(k, nr, nc)[0] for k in KINDS])


@pytest.mark.parametrize("shape", SHAPES + [(120, 150)], ids=ids)
def test_predict_parity(codec, shape):
    nr, nc = shape
    kinds = KINDS if shape != (120, 150) else ("terrain0",)
    seeds, coefs, res, status = codec.predict(nr, nc, np.stack([ref(k, nr, nc)[0] for k in kinds]))
    n_ok = 0
    for t, k in enumerate(kinds):
        v, pr, _, _, _ = ref(k, nr, nc)
        if pr is None:
            assert status[t] == DECLINED, (k, status[t])
            continue
        seed, u, init, inter = pr
        assert status[t] == OK and seeds[t] == seed, (k, status[t])
        assert coefs[t].tobytes() == u.tobytes(), (k, coefs[t], u)
        assert res[t].tolist() == init + inter, k
        n_ok += 1
    assert n_ok >= 1 or nr < 4 or nc < 4


@pytest.mark.parametrize("shape", [s for s in SHAPES if min(s) >= 4] + [(120, 150)], ids=ids)
def test_reconstruct_parity(codec, shape):
    """rows > 64 cross the band seam of k_lsop8_reconstruct (two rows through LDS), columns > 64 its prefix-sum chunks"""
    nr, nc = shape
    kinds = [k for k in (KINDS if shape != (120, 150) else ("terrain0",)) if ref(k, nr, nc)[1] is not None]
    prs = [ref(k, nr, nc)[1] for k in kinds]
    got, status = codec.reconstruct(nr, nc, [p[0] for p in prs], np.stack([p[1] for p in prs]), np.array([p[2] + p[3] for p in prs], np.int32))
    for t, k in enumerate(kinds):
        assert status[t] == OK and np.array_equal(got[t], ref(k, nr, nc)[0]), k


@pytest.mark.parametrize("shape", [(12, 70), (70, 12)], ids=ids)
def test_reconstruct_substituted_coefficients(codec, shape):
    """coefficient sets that push the predictions to the numeric edges: the streams stay, the tile becomes what the coefficients make it"""
    nr, nc = shape
    v = R_smooth(nr, nc)
    init, inter = R.initialisers(nr, nc, v), R.interior(nr, nc, v, R.coefficients(nr, nc, v))
    names = list(R.COEF_SETS)
    want, traces = [], {}
    for name in names:
        tr = []
        want.append(R.reconstruct(nr, nc, int(v[0]), init, inter, R.COEF_SETS[name], trace=tr))
        traces[name] = np.array(tr, np.float32)
    # the sets do what they are there for
    with np.errstate(all="ignore"):
        assert (traces["neg_half_left"] < 0).any() and (traces["minus_up"] < 0).any()
        q = traces["half_left"] + np.float32(0.5)
        assert ((q == np.floor(q)) & (traces["half_left"] != np.floor(traces["half_left"]))).any()          # p + 0.5f lands on an integer
        assert np.isposinf(traces["pos_inf"]).any() and np.isneginf(traces["neg_inf"]).any() and np.isnan(traces["inf_pair"]).any()
        assert np.isnan(traces["nan"]).any()
        assert (traces["sat_pos"] > 3e9).any() and (traces["sat_pos"] < -3e9).any() and (traces["sat_neg"] > 3e9).any()
    got, status = codec.reconstruct(nr, nc, [int(v[0])] * len(names), np.stack([R.COEF_SETS[n] for n in names]),
                                    np.array([init + inter] * len(names), np.int32))
    for t, name in enumerate(names):
        assert status[t] == OK and np.array_equal(got[t], want[t]), name
    # ... and through the decoder: a container with its coefficients replaced
    p0 = R.encode(2, nr, nc, v, force_type=0)[0]
    packs = [R.substitute(p0, R.COEF_SETS[n]) for n in names]
    vals, st = codec.decode_batch(nr, nc, packs)
    for t, name in enumerate(names):
        assert st[t] == OK and np.array_equal(vals[t], want[t]), name


@pytest.mark.parametrize("shape", SHAPES + [(120, 150)], ids=ids)
def test_device_encoder_writes_the_huffman_container(codec, shape):
    nr, nc = shape
    kinds = KINDS if shape != (120, 150) else ("terrain0",)
    packs, status = codec.encode_batch_dev(6, nr, nc, np.stack([ref(k, nr, nc)[0] for k in kinds]))
    for t, k in enumerate(kinds):
        p0 = ref(k, nr, nc)[2]
        if p0 is None:
            assert status[t] == DECLINED and packs[t] is None, k
        else:
            assert status[t] == OK and packs[t] == p0, (k, len(packs[t] or b""), len(p0))


def test_host_encoder_gives_the_reference_choice(codec):
    nr, nc = 33, 65
    packs, types, status = codec.encode_batch(6, nr, nc, tiles_of(nr, nc))
    seen = set()
    for t, k in enumerate(KINDS):
        v, pr, p0, p1, ctype = ref(k, nr, nc)
        if pr is None:
            assert status[t] == DECLINED and packs[t] is None and types[t] == 0, k
            continue
        assert status[t] == OK and types[t] == ctype and packs[t] == (p0, p1)[ctype], k
        seen.add(ctype)
    assert seen == {0, 1}
    one = codec.encode(6, nr, nc, ref("terrain0", nr, nc)[0])
    assert one == ref("terrain0", nr, nc)[2] and codec.encode(6, nr, nc, ref("uniform", nr, nc)[0]) is None
    assert np.array_equal(codec.decode(nr, nc, one), ref("terrain0", nr, nc)[0])


@pytest.mark.parametrize("shape", [(4, 4), (7, 9), (33, 65), (65, 66), (129, 4), (4, 129)], ids=ids)
def test_decode_both_types_and_header_revisions(codec, shape):
    nr, nc = shape
    packs, want = [], []
    for k in KINDS:
        v, pr, p0, p1, _ = ref(k, nr, nc)
        if pr is None:
            continue
        for p in (p0, p1):
            packs += [p, R.to_legacy_header(p), R.with_checksum_flag(p)]
            want += [v] * 3
    assert len(packs) >= 12
    for vals, st in (codec.decode_batch(nr, nc, packs), codec.decode_batch_dev(nr, nc, packs)):
        for t in range(len(packs)):
            assert st[t] == OK and np.array_equal(vals[t], want[t]), (t, st[t])


def test_mixed_batch_statuses(codec):
    nr, nc = 7, 9
    v, pr, p0, p1, _ = ref("terrain0", nr, nc)
    # encode: good, singular, good
    packs, status = codec.encode_batch_dev(6, nr, nc, np.stack([v, ref("uniform", nr, nc)[0], ref("noise32", nr, nc)[0]]))
    assert status.tolist() == [OK, DECLINED, OK] and packs[0] == p0 and packs[2] == ref("noise32", nr, nc)[2]
    # decode: good packings between damaged ones
    huge = struct.pack("<i", 10 ** 6)
    bad = {"ncoef12": p0[:2] + bytes([12]) + p0[3:], "type2": p0[:1] + bytes([0x42]) + p0[2:], "type3": p1[:1] + bytes([0x43]) + p1[2:],
           "type2_legacy": R.to_legacy_header(p0)[:46] + bytes([2]) + R.to_legacy_header(p0)[47:],
           "count_init": p0[:39] + huge + p0[43:], "count_interior": p1[:43] + huge + p1[47:], "header_only": p0[:47], "short": p1[:20]}
    batch = [p0] + list(bad.values()) + [p1]
    vals, st = codec.decode_batch(nr, nc, batch)
    assert st[0] == OK and st[-1] == OK and np.array_equal(vals[0], v) and np.array_equal(vals[-1], v)
    for t, name in enumerate(bad, start=1):
        with pytest.raises(IOError):
            R.decode(nr, nc, batch[t])
        assert st[t] < 0, name
        if name in ("ncoef12", "type2", "type3", "type2_legacy", "count_init", "count_interior"):
            assert st[t] == ERR_FORMAT, (name, st[t])
    with pytest.raises(IOError):
        codec.decode(nr, nc, bad["ncoef12"])


def test_the_two_lsop_codecs_refuse_each_other(codec):
    import gridfour_amd
    nr, nc = 16, 16
    v = ref("terrain0", nr, nc)[0]
    c12 = gridfour_amd.LsCodecHip(context=codec.ctx)
    p12 = [oracle.lsop12_encode(1, nr, nc, v, False)[0], oracle.lsop12_encode_legacy_huffman(1, nr, nc, v)]
    _, st = codec.decode_batch(nr, nc, p12)
    assert st.tolist() == [ERR_FORMAT, ERR_FORMAT]
    _, st = c12.decode_batch(nr, nc, [ref("terrain0", nr, nc)[2], ref("terrain0", nr, nc)[3]])
    assert st.tolist() == [ERR_FORMAT, ERR_FORMAT]


@pytest.mark.parametrize("n_tiles", [1, 3, GRID_CAP + 5])
def test_tile_counts(codec, n_tiles):
    nr, nc = 4, 5
    base = [ref(k, nr, nc) for k in ("terrain0", "smooth", "noise32", "sparse_big", "uniform")]
    pick = [t % len(base) for t in range(n_tiles)]
    tiles = np.stack([base[i][0] for i in range(len(base))])[pick]
    seeds, coefs, res, status = codec.predict(nr, nc, tiles)
    packs, est = codec.encode_batch_dev(3, nr, nc, tiles)
    for i, (v, pr, p0, p1, _) in enumerate(base):
        rows = np.nonzero(np.array(pick) == i)[0]
        if pr is None:
            assert (status[rows] == DECLINED).all() and (est[rows] == DECLINED).all()
            continue
        assert (status[rows] == OK).all() and (est[rows] == OK).all()
        assert (coefs[rows].view(np.uint32) == pr[1].view(np.uint32)).all() and (res[rows] == np.array(pr[2] + pr[3], np.int32)).all()
        want = R.encode(3, nr, nc, v, force_type=0)[0]
        assert all(packs[t] == want for t in rows)
    good = [t for t in range(n_tiles) if packs[t] is not None]
    for vals, st in (codec.decode_batch_dev(nr, nc, [packs[t] for t in good]),):
        assert (st == OK).all() and np.array_equal(vals, tiles[good])
    got, st = codec.reconstruct(nr, nc, seeds[good], coefs[good], res[good])
    assert (st == OK).all() and np.array_equal(got, tiles[good])


def _cut_class(status):
    return "ok" if status == OK else "refused"


def test_truncation_at_every_length(codec):
    """one 7 x 9 packing of each type cut at every length, in one batch"""
    import gridfour_amd
    nr, nc = 7, 9
    v, pr, p0, p1, _ = ref("terrain0", nr, nc)
    cuts = [(t, n) for t, p in ((0, p0), (1, p1)) for n in range(len(p))]
    batch = [(p0, p1)[t][:n] for t, n in cuts]
    vals, st = codec.decode_batch(nr, nc, batch)
    # what the shared inflate path makes of a zlib trailer that is cut, shown by LSOP12 on the same kind of cut
    v12 = make_tile("noise8", 16, 16)
    p12, t12 = oracle.lsop12_encode(1, 16, 16, v12, True)
    assert t12 == 1
    c12 = gridfour_amd.LsCodecHip(context=codec.ctx)
    vals12, st12 = c12.decode_batch(16, 16, [p12[:len(p12) - k] for k in range(1, 5)])
    trailer = {k: _cut_class(st12[k - 1]) for k in range(1, 5)}
    for k in range(1, 5):
        assert st12[k - 1] != OK or np.array_equal(vals12[k - 1], v12)
    n_ok = 0
    for i, (t, n) in enumerate(cuts):
        missing = len((p0, p1)[t]) - n
        if t == 1 and missing <= 4:
            assert _cut_class(st[i]) == trailer[missing], (t, n, st[i])
            assert st[i] != OK or np.array_equal(vals[i], v)
            continue
        try:
            want = R.decode(nr, nc, batch[i])
        except IOError:
            assert st[i] < 0, (t, n, st[i])
            continue
        assert st[i] == OK and np.array_equal(vals[i], v) and np.array_equal(want, v), (t, n, st[i])
        n_ok += 1
    assert (st[:47] < 0).all()
