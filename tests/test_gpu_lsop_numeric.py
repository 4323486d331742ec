"""LSOP12 on the MI355X at its numeric edges, bit for bit against the CPU oracle (oracle.lsop12_*), whose float32 prediction and
StrictMath.round are pinned by tests/test_oracle_lsop_numeric.py.

Decoder: oracle containers with substituted coefficients (tests/lsop_ref.py) through every reconstruction kernel of
gf_launch_lsop_reconstruct (gvrs_lsop.hip:2305-2351), and gf_lsop12_reconstruct_dev on caller-built and on the library's own buffers.
Encoder: the coefficient paths of k_lsop_predict (gvrs_lsop.hip:446-515) and k_lsop_predict16 (:729-) at their guards -- the MFMA
digit guard, the int32 headroom of its digit sums, the column and LDS limits, the 2^53 exactness guard -- and on degenerate systems.

Line numbers below are gvrs_lsop.hip's unless another file is named."""

import numpy as np
import pytest

import lsop_ref as L
import oracle
from lsop_ref import CASES, COEF_SETS, case_id
from tilegen import make_tile

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def codec():
    import gridfour_amd
    return gridfour_amd.LsCodecHip(deflate_enabled=False)


def _lib():
    from gridfour_amd import _lib, lib
    return lib(), _lib.check


def _stride(nr, nc):
    lib, _ = _lib()
    return (int(lib.gf_lsop12_residual_count(nr, nc)) + 3) // 4 * 4


def _decode_dev(codec, nr, nc, packs):
    """gf_lsop12_decode_batch_i32_dev on packings in HBM: (values, status, coefficient records [nt, 16] uint32, device buffers)."""
    from gridfour_amd import DeviceBuffer
    lib, check = _lib()
    ctx = codec.ctx
    nt = len(packs)
    slot = (max(len(p) for p in packs) + 255) // 256 * 256
    blob = np.zeros(nt * slot, np.uint8)
    for k, pk in enumerate(packs):
        blob[k * slot:k * slot + len(pk)] = np.frombuffer(pk, np.uint8)
    lengths = np.array([len(pk) for pk in packs], np.uint32)
    rs = _stride(nr, nc)
    buf = dict(blob=DeviceBuffer(ctx, blob.nbytes), len=DeviceBuffer(ctx, nt * 4), val=DeviceBuffer(ctx, nt * nr * nc * 4),
               st=DeviceBuffer(ctx, nt * 4), res=DeviceBuffer(ctx, nt * rs * 4), co=DeviceBuffer(ctx, nt * 64),
               sc=DeviceBuffer(ctx, nt * 4))
    buf["blob"].upload(blob)
    buf["len"].upload(lengths)
    check(lib.gf_lsop12_decode_batch_i32_dev(ctx.handle, None, nr, nc, nt, buf["blob"].ptr, blob.nbytes, None, slot, buf["len"].ptr,
                                             buf["val"].ptr, buf["st"].ptr, buf["res"].ptr, rs, buf["co"].ptr, buf["sc"].ptr), "decode")
    ctx.synchronize()
    vals = buf["val"].download(np.int32, nt * nr * nc).reshape(nt, -1)
    return vals, buf["st"].download(np.int32, nt), buf["co"].download(np.uint32, nt * 16).reshape(nt, 16), buf


def _free(buf):
    for b in buf.values():
        b.free()


def _expect_oracle(nr, nc, packs, vals, st):
    for k, pk in enumerate(packs):
        want = oracle.lsop12_decode(nr, nc, pk)
        assert st[k] == 0, (k, int(st[k]))
        assert np.array_equal(vals[k], want), (nr, nc, k, np.nonzero(vals[k] != want)[0][:8])


FMT_WORD = 14          # GF_LSOP_FMT_WORD (gvrs_kernels.h): 1 = the tile's interior residuals lie as a byte plane


# ------------------------------------------------------------------------------------------------------------------------------
# 2. every reconstruction kernel against substituted containers
# ------------------------------------------------------------------------------------------------------------------------------
def _sources(nr, nc, spike=False, container="canon"):
    """One oracle container per offset that CASES uses: {offset: (packing, legacy header?)}."""
    out = {}
    for off in sorted({o for _, o in CASES}):
        v = L.tile_for(nr, nc, off)
        if container == "deflate":                        # a plane with steps: long runs of equal residuals, Deflate wins
            y, x = np.mgrid[0:nr, 0:nc]
            v = (3 * x + 5 * y + 40 * ((x // 16 + y // 16) % 2) + off).astype(np.int32).ravel()
        if spike:
            v = L.with_spike(v, nr, nc, nr // 2, nc // 2, 5000)
        if container == "legacy":
            out[off] = (oracle.lsop12_encode_legacy_huffman(3, nr, nc, v), True)
        else:
            pk, typ = oracle.lsop12_encode(3, nr, nc, v, container == "deflate")
            assert typ == (1 if container == "deflate" else 2), (nr, nc, off, typ)
            out[off] = (pk, False)
    return out


def _substituted(nr, nc, **kw):
    src = _sources(nr, nc, **kw)
    return [L.substitute(src[off][0], COEF_SETS[name], legacy=src[off][1]) for name, off in CASES]


# (shape, residuals, container, the kernel meant): gf_launch_lsop_reconstruct, gvrs_lsop.hip:2314 planes = planes && g.ok; :2317 pipe =
# nRows > 66 && nCols >= 16 (and the LDS of :2316 <= 96 KB); :2318 the plane kernel, whose first nOld workgroups take the non-plane tiles
# when pipe holds (:2320-2330, lsop_reconstruct_pipe_tiles); :2335-2343 k_lsop_reconstruct / k_lsop_reconstruct_pipe; :2345
# k_lsop_reconstruct_global when the LDS of :2316 exceeds 96 KB, i.e. nCols > 11,232
ROUTES = [
    ((40, 64), False, "canon", "plane"),                  # plane geometry ok (lsop_ref.plane_geom_ok), byte residuals, pipe false
    ((66, 64), False, "canon", "plane"),                  # the last row count without pipe
    ((120, 150), False, "canon", "plane"),                # plane with pipe: the plane kernel alone
    ((24, 40), False, "canon", "recon"),                  # no plane geometry (the plane does not fit the slot): k_lsop_reconstruct
    ((12, 16), False, "canon", "recon"),                  # nC < 32: k_lsop_reconstruct
    ((40, 64), True, "canon", "recon"),                   # a plane shape with one wide residual, pipe false: k_lsop_reconstruct
    ((120, 150), True, "canon", "pipe-in-plane"),         # wide residual, pipe true: the plane kernel's first nOld workgroups
    ((120, 150), False, "legacy", "pipe-in-plane"),       # type-0 containers are never planes
    ((120, 150), False, "deflate", "pipe-in-plane"),      # nor type-1
    ((100, 24), False, "canon", "pipe"),                  # nC < 32: no plane geometry, pipe true: k_lsop_reconstruct_pipe itself
    ((1030, 40), False, "canon", "pipe"),                 # nR > 1024: no plane geometry: k_lsop_reconstruct_pipe
    ((6, 11240), False, "canon", "global"),               # nC >= 11,233: k_lsop_reconstruct_global
    ((8, 12000), False, "canon", "global"),
]


@pytest.mark.parametrize("route", ROUTES, ids=lambda r: "%dx%d-%s%s-%s" % (r[0] + ("spike" if r[1] else "bytes", r[2], r[3])))
def test_substituted_coefficients_through_every_reconstruction_kernel(codec, route):
    (nr, nc), spike, container, kernel = route
    assert L.plane_geom_ok(nr, nc) == (kernel in ("plane", "pipe-in-plane") or (kernel == "recon" and spike)), "route misjudged"
    packs = _substituted(nr, nc, spike=spike, container=container)
    # plane tiles: every interior residual a byte (66 x 64 near 2e7 has a wider one and goes the other way)
    want_fmt = [int(kernel == "plane" and L.byte_residuals(nr, nc, L.tile_for(nr, nc, off))) for _, off in CASES]
    assert kernel != "plane" or sum(want_fmt) >= len(CASES) - 1
    vals, st, co, buf = _decode_dev(codec, nr, nc, packs)
    _free(buf)
    _expect_oracle(nr, nc, packs, vals, st)
    # the decoder routed them as meant: plane tiles carry 1 in word GF_LSOP_FMT_WORD, the others 0
    assert [int(x) for x in co[:, FMT_WORD]] == want_fmt
    # and the host-memory form agrees
    vals2, st2 = codec.decode_batch(nr, nc, packs)
    assert np.array_equal(vals2, vals) and np.array_equal(st2, st)


@pytest.mark.parametrize("shape", [(6, 11240), (8, 12000)], ids=lambda s: "%dx%d" % s)
def test_global_kernel_encode_decode_parity(codec, shape):
    """Ordinary tiles of k_lsop_reconstruct_global's widths: encode parity with the oracle, decode back to the tile."""
    nr, nc = shape
    tiles = np.stack([L.smooth(nr, nc, s) for s in range(3)] + [make_tile("noise16", nr, nc), make_tile("sparse_big", nr, nc)])
    packs, types, status = codec.encode_batch(2, nr, nc, tiles)
    good = []
    for t, v in enumerate(tiles):
        ref, typ = oracle.lsop12_encode(2, nr, nc, v, False)
        assert status[t] == 0 and packs[t] == ref, t
        good.append(packs[t])
    vals, st = codec.decode_batch(nr, nc, good)
    assert np.all(st == 0) and np.array_equal(vals, tiles)


@pytest.mark.parametrize("shape", [(40, 64), (120, 150)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("n", [1, 3, 21])
def test_mixed_plane_and_int32_tiles_with_different_coefficients(codec, shape, n):
    """Plane and non-plane tiles with different coefficient sets share the waves of k_lsop_reconstruct_plane (two tiles to a wave):
    plane | other, other | plane, other | other, plane | plane, and an odd count leaves the last wave one tile."""
    nr, nc = shape
    plane = _substituted(nr, nc)
    wide = _substituted(nr, nc, spike=True)
    pattern = "powwoppowpwoowpppwwpo"[:n]
    packs = [(plane if ch == "p" else wide)[(k * 7 + 3) % len(CASES)] for k, ch in enumerate(pattern)]
    vals, st, co, buf = _decode_dev(codec, nr, nc, packs)
    _free(buf)
    _expect_oracle(nr, nc, packs, vals, st)
    assert [int(x) for x in co[:, FMT_WORD]] == [1 if ch == "p" else 0 for ch in pattern]


# LsCodecHip.reconstruct (gf_lsop12_reconstruct_dev): a caller-built record (words 13..15 = 0) and the oracle's residuals: every
# non-plane kernel without a container
@pytest.mark.parametrize("shape", [(12, 16), (24, 40), (40, 64), (120, 150), (100, 24), (6, 11240)], ids=lambda s: "%dx%d" % s)
def test_reconstruct_with_chosen_coefficients(codec, shape):
    nr, nc = shape
    seeds, coefs, res, want = [], [], [], []
    for name, off in CASES:
        v = L.tile_for(nr, nc, off)
        seed, _, init, interior = oracle.lsop12_residuals(nr, nc, v)
        pk, _ = oracle.lsop12_encode(0, nr, nc, v, False)
        seeds.append(seed)
        coefs.append(COEF_SETS[name])
        res.append(np.concatenate([init, interior]))
        want.append(oracle.lsop12_decode(nr, nc, L.substitute(pk, COEF_SETS[name])))
    got, st = codec.reconstruct(nr, nc, seeds, np.stack(coefs), np.stack(res))
    assert np.all(st == 0), st
    for k in range(len(CASES)):
        assert np.array_equal(got[k], want[k]), (CASES[k], np.nonzero(got[k] != want[k])[0][:8])


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the encoder's coefficient paths at their guards
# ------------------------------------------------------------------------------------------------------------------------------
def _encoder_parity(codec, nr, nc, tiles, tag=""):
    """predict and encode_batch against the oracle: seed, the 12 coefficient floats as bytes, residuals, declines, containers.
    Returns the oracle's coefficients of the accepted tiles (for the report of non-finite / saturating ones)."""
    tiles = np.ascontiguousarray(tiles, np.int32).reshape(-1, nr * nc)
    seeds, coefs, res, status = codec.predict(nr, nc, tiles)
    packs, types, est = codec.encode_batch(5, nr, nc, tiles)
    accepted = []
    for t, v in enumerate(tiles):
        ref = oracle.lsop12_residuals(nr, nc, v)
        if ref is None:
            assert status[t] == 1 and est[t] == 1 and packs[t] is None, (tag, t, status[t], est[t])
            continue
        o_seed, o_u, o_init, o_inter = ref
        assert status[t] == 0 and seeds[t] == o_seed, (tag, t, status[t])
        assert coefs[t].tobytes() == o_u.tobytes(), (tag, t, coefs[t], o_u)
        assert np.array_equal(res[t], np.concatenate([o_init, o_inter])), (tag, t)
        want, typ = oracle.lsop12_encode(5, nr, nc, v, False)
        assert est[t] == 0 and types[t] == typ and packs[t] == want, (tag, t)
        accepted.append(o_u)
    return accepted


def _smooth_amp(nr, nc, amp, seed=0):
    return L.smooth(nr, nc, seed, amp=amp)


# k_lsop_predict takes the matrix-pipe Gram (lsop_gram_mfma, :488) when nC <= 256, maxAbs <= LSOP_MFMA_MAX_ABS = 32639 (:272: the high
# digit (z + 128) >> 8 must stay <= 127; 32,640 makes it 128) and nInt < 2^17; k_lsop_predict16 sends a tile back when maxAbs > 32639 (:777)
GUARD_SHAPES = [(64, 64),        # k_lsop_predict16 (256 threads), then k_lsop_predict for what it sends back
                (522, 256)]      # too large for k_lsop_predict16's LDS: k_lsop_predict alone (nInt 131,040 < 2^17)


@pytest.mark.parametrize("shape", GUARD_SHAPES, ids=lambda s: "%dx%d" % s)
def test_mfma_digit_guard(codec, shape):
    nr, nc = shape
    tiles = []
    for k, m in enumerate((32639, 32640, 32767, 32768, -32639, -32640, -32768)):
        v = _smooth_amp(nr, nc, 30000, k).reshape(nr, nc).copy()
        v = np.clip(v, -32000, 32000)
        v[nr // 2, nc // 3] = m                               # the tile's largest magnitude, exactly m
        tiles.append(v.ravel())
    v = _smooth_amp(nr, nc, 300, 9).reshape(nr, nc).copy()
    v[3, 5] = L.I32_MIN                                       # |INT32_MIN| does not fit an int32
    tiles.append(v.ravel())
    _encoder_parity(codec, nr, nc, tiles, "digit guard")


def _minus128(nr, nc, noisy, seed=0):
    """Every value = 256 k - 128 with |value| <= 32,639: every low digit is -128, the int32 digit sums' worst case."""
    rng = np.random.default_rng(seed + nr * 7 + nc)
    if noisy:
        k = rng.integers(-126, 128, nr * nc)
    else:
        y, x = np.mgrid[0:nr, 0:nc]
        k = np.clip(np.round(100 * np.sin(x / 23.0 + seed) * np.cos(y / 19.0) + 20 * np.sin((x + y) / 7.0)), -126, 127).ravel()
    return (256 * k.astype(np.int64) - 128).astype(np.int32)


# the largest interiors the MFMA path takes with nC <= 256: 522 x 256 (nInt 131,040), 1,025 x 132 (130,944); 1,026 x 132 has nInt = 2^17
# exactly and leaves the MFMA path (:488); 256 x 256 is k_lsop_predict16's (1,024 threads), which keeps smooth tiles and sends noisy ones,
# whose residuals exceed a halfword (:944), back to k_lsop_predict's MFMA path
@pytest.mark.parametrize("shape", [(522, 256), (1025, 132), (1026, 132), (256, 256)], ids=lambda s: "%dx%d" % s)
def test_mfma_int32_headroom(codec, shape):
    nr, nc = shape
    tiles = [_minus128(nr, nc, False), _minus128(nr, nc, True), _minus128(nr, nc, False, 1)]
    _encoder_parity(codec, nr, nc, tiles, "headroom")


# gf_lsop_predict16_eligible (:2263) and gf_lsop_predict16_threads (:2258): 2 * ((cells + 64 + 15) & ~15) + sizeof(LsopShared16) against
# 150 KB and 53 KB, with sizeof(LsopShared16) = 4,360 bytes (G[104] doubles, the 27 x 32 int32 digit Gram / histograms, u[12], five
# words): eligible up to 74,544 cells, 256 threads up to 24,880 cells.  nC 256 / 257: the ring and matrix-pipe paths end at
# LSOP_RING_MAXC = 256 (:209)
LIMIT_SHAPES = [(40, 256), (40, 257), (1553, 48), (1554, 48), (311, 80), (312, 80)]


@pytest.mark.parametrize("shape", LIMIT_SHAPES, ids=lambda s: "%dx%d" % s)
def test_column_and_lds_limits(codec, shape):
    nr, nc = shape
    tiles = [L.smooth(nr, nc, 0), L.smooth(nr, nc, 1, amp=20000), make_tile("noise16", nr, nc), _minus128(nr, nc, False)]
    v = L.smooth(nr, nc, 2).copy()
    v[nr * nc // 2] = 40000                                   # maxAbs beyond the digit guard: sent back by k_lsop_predict16
    tiles.append(v)
    _encoder_parity(codec, nr, nc, tiles, "limits")


def _clustered(nr, nc, k, seed):
    """Odd values just below M = sqrt(k 2^53 / nInt): the bound maxAbs^2 nInt is about k 2^53 and so are the ACTUAL Gram sums."""
    n_int = (nr - 2) * (nc - 4)
    m = int((k * 2.0 ** 53 / n_int) ** 0.5)
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:nr, 0:nc]
    v = m - 300 - (120 * np.sin(x / 5.0 + seed) * np.cos(y / 4.0)).astype(np.int64) - rng.integers(0, 150, (nr, nc))
    return (v | 1).astype(np.int32).ravel()


@pytest.mark.parametrize("shape", [(64, 64), (40, 300)], ids=lambda s: "%dx%d" % s)
def test_2p53_guard_with_actual_sums_beyond_it(codec, shape):
    """k_lsop_predict (:483-484) sums in the reference's scan order when maxAbs^2 nInt >= 2^53.  These tiles' real sums lie 1.1 .. 3.9
    times past 2^53 (a bound merely above it proves nothing: the sums stay exact) -- where scan order, row order and exact sums differ --
    and their bound stays below 4 x 2^53."""
    nr, nc = shape
    n_int = (nr - 2) * (nc - 4)
    tiles = []
    for k in (1.1, 2.0, 3.0, 3.9):
        for seed in range(3):
            v = _clustered(nr, nc, k, seed)
            z = v.reshape(nr, nc)[2:, 2:nc - 2].astype(np.int64).ravel()
            c00 = int((z * z).sum())
            bound = float(np.abs(v.astype(np.int64)).max()) ** 2 * n_int
            assert 2 ** 53 < c00 and 2 ** 53 <= bound < 4 * 2 ** 53, (k, seed)
            tiles.append(v)
    _encoder_parity(codec, nr, nc, tiles, "2^53")


def _degenerate(nr, nc):
    y, x = np.mgrid[0:nr, 0:nc]
    out = {
        "constant_rows": 37 * y + 5,
        "constant_columns": 11 * x - 200,
        "plane": 1000 + 3 * x - 7 * y,
        "checkerboard": 500 * ((x + y) % 2),
        "stripes2": 300 * (x % 2) + y,
        "stripes3": 100 * (x % 3) - 40 * (y % 3),
        "separable": (x * x - 3 * x + 1) * (2 * y + 1),
        "mirror_lr": 50 * np.abs(x - (nc - 1) / 2.0).astype(np.int64) + (y * y) % 17,
        "mirror_ud": 70 * np.abs(y - (nr - 1) / 2.0).astype(np.int64) + (x * x) % 13,
        "single": np.where((y == nr // 2) & (x == nc // 2), 1234, 0),
        "two_valued": np.where(np.sin(x * 0.7 + y * 1.3) > 0, 9, -4),
        "two_valued_blocks": np.where(((x // 5) + (y // 3)) % 2 == 0, 32000, -32000),
    }
    return {k: np.asarray(v, np.int64).astype(np.int32).ravel() for k, v in out.items()}


# 24 x 40 and 120 x 150: k_lsop_predict16 (256 threads); 64 x 300: nC > 256, k_lsop_predict's FP64 lsop_gram_wave (:498)
@pytest.mark.parametrize("shape", [(24, 40), (64, 300), (120, 150)], ids=lambda s: "%dx%d" % s)
def test_degenerate_and_tied_systems(codec, shape):
    nr, nc = shape
    d = _degenerate(nr, nc)
    names = list(d)
    accepted = _encoder_parity(codec, nr, nc, [d[k] for k in names], "degenerate")
    # (the coefficients these systems give are whatever JAMA's LU makes of them: the oracle's, bit for bit, checked above; the
    # non-finite or huge ones that reach lsop_round / lsop_round_f32 on the encoder side are listed by -rP)
    for u in accepted:
        if not np.all(np.isfinite(u)) or np.any(np.abs(u) > 1e6):
            print("degenerate %dx%d: extreme coefficients %s" % (nr, nc, u))


@pytest.mark.parametrize("n", [1, 7, 259])
def test_mixed_predict16_and_retry_batches(codec, n):
    """Tiles k_lsop_predict16 keeps next to tiles it marks for k_lsop_predict (retryOnly): maxAbs > 32,639 (:777), residuals beyond a
    halfword (:944), declines; batches of 1, an odd count and more than 256 tiles."""
    nr, nc = 64, 64
    kinds = [lambda s: L.smooth(nr, nc, s),
             lambda s: make_tile("noise16", nr, nc, seed=s),                          # residuals beyond a halfword: sent back
             lambda s: _clustered(nr, nc, 2.0, s),                                     # maxAbs > 32,639: sent back, FP64 scan order
             lambda s: L.smooth(nr, nc, s, amp=20000),
             lambda s: _minus128(nr, nc, True, s),
             lambda s: np.full(nr * nc, 5, np.int32)]                                  # declined
    tiles = [kinds[(k * 5 + 1) % len(kinds) if n > 1 else 1](k) for k in range(n)]
    _encoder_parity(codec, nr, nc, tiles, "mixed")


# ------------------------------------------------------------------------------------------------------------------------------
# 4. gf_lsop12_reconstruct_dev on the library's own buffers
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(64, 64), (256, 256), (522, 256), (40, 300), (120, 150)], ids=lambda s: "%dx%d" % s)
def test_predict_then_reconstruct_on_the_same_buffers(codec, shape):
    """gf_lsop12_predict_dev -> gf_lsop12_reconstruct_dev on the same device buffers gives the tiles back (both predict kernels write 0
    into words 13..15: :530, :797), for tiles of each encoder path."""
    from gridfour_amd import DeviceBuffer
    lib, check = _lib()
    nr, nc = shape
    tiles = np.stack([L.smooth(nr, nc, 0), L.smooth(nr, nc, 1, amp=20000), make_tile("noise16", nr, nc), _minus128(nr, nc, True),
                      _clustered(nr, nc, 2.0, 0), np.full(nr * nc, 3, np.int32), L.with_spike(L.smooth(nr, nc, 2), nr, nc, 3, 5, 9000)])
    nt = len(tiles)
    rs = _stride(nr, nc)
    ctx = codec.ctx
    dv, dr, dc, ds = (DeviceBuffer(ctx, tiles.nbytes), DeviceBuffer(ctx, nt * rs * 4 + 16), DeviceBuffer(ctx, nt * 64),
                      DeviceBuffer(ctx, nt * 4))
    dout, dst = DeviceBuffer(ctx, tiles.nbytes), DeviceBuffer(ctx, nt * 4)
    dv.upload(tiles)
    check(lib.gf_lsop12_predict_dev(ctx.handle, None, nr, nc, nt, dv.ptr, dr.ptr, rs, dc.ptr, ds.ptr), "predict")
    check(lib.gf_lsop12_reconstruct_dev(ctx.handle, None, nr, nc, nt, dr.ptr, rs, dc.ptr, ds.ptr, dout.ptr, dst.ptr), "reconstruct")
    ctx.synchronize()
    status = ds.download(np.int32, nt)
    st2 = dst.download(np.int32, nt)
    got = dout.download(np.int32, nt * nr * nc).reshape(nt, -1)
    co = dc.download(np.uint32, nt * 16).reshape(nt, 16)
    for b in (dv, dr, dc, ds, dout, dst):
        b.free()
    assert status[5] == 1 and st2[5] == 1                   # the constant tile: declined, passed through
    for t in range(nt):
        assert (oracle.lsop12_residuals(nr, nc, tiles[t]) is None) == (status[t] == 1), t
        if status[t] == 0:
            assert np.all(co[t, 13:16] == 0), (t, co[t, 13:16])
            assert st2[t] == 0 and np.array_equal(got[t], tiles[t]), t


@pytest.mark.parametrize("shape", [(40, 64), (120, 150)], ids=lambda s: "%dx%d" % s)
def test_decode_then_reconstruct_on_the_same_buffers(codec, shape):
    """gf_lsop12_decode_batch_i32_dev, then gf_lsop12_reconstruct_dev on the d_residuals / d_coefs it left: the decoded values again.
    The batch holds plane tiles (a byte plane in the residual slot, word 14 = 1) next to int32 ones and a Deflate container."""
    from gridfour_amd import DeviceBuffer
    lib, check = _lib()
    nr, nc = shape
    plane = _substituted(nr, nc)
    wide = _substituted(nr, nc, spike=True)
    defl = _substituted(nr, nc, container="deflate")
    packs = [plane[0], wide[1], plane[5], plane[9], wide[12], defl[2], plane[17], wide[7], plane[20]]
    vals, st, co, buf = _decode_dev(codec, nr, nc, packs)
    nt = len(packs)
    try:
        _expect_oracle(nr, nc, packs, vals, st)
        assert int(co[:, FMT_WORD].sum()) == 5
        dout, dst = DeviceBuffer(codec.ctx, nt * nr * nc * 4), DeviceBuffer(codec.ctx, nt * 4)
        check(lib.gf_lsop12_reconstruct_dev(codec.ctx.handle, None, nr, nc, nt, buf["res"].ptr, _stride(nr, nc), buf["co"].ptr,
                                            buf["sc"].ptr, dout.ptr, dst.ptr), "reconstruct")
        codec.ctx.synchronize()
        again = dout.download(np.int32, nt * nr * nc).reshape(nt, -1)
        st2 = dst.download(np.int32, nt)
        dout.free()
        dst.free()
    finally:
        _free(buf)
    assert np.all(st2 == 0), st2
    for k in range(nt):
        assert np.array_equal(again[k], vals[k]), (k, int(co[k, FMT_WORD]), np.nonzero(again[k] != vals[k])[0][:8])
