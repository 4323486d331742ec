"""The record read chain beyond one round of k_codec_partition (gvrs_records.hip).  The single workgroup sorts the batch's element
instances by codec 1,024 at a time; from instance 1,024 on a place is its segment's start + the members of EARLIER ROUNDS
(run[seg] += sum, the waves' counters cleared) + those in earlier waves + the rank in the wave, and recordsDecodeDev
(gvrs_api_records_dev.hip) hands each decoder the sub-arrays subOffsets + j0, subLengths + j0 and tmp + j0 * cells of its
segment.  Below 1,025 instances none of that carry runs; production batches are 12,960 and 93,312 tiles.

Tiles are 16 x 20 (tests/count_seams.py: a pool of 40 distinct tiles, packed once per integer codec of LIST5 by the oracle's
encoders, and their standard form).  Which tile a record holds follows count_seams.sequence with period 1,024: no record holds the
tile of the record a whole number of rounds before it, so a result one round off cannot pass.  Expected values are the pool's
tiles, statuses and tile indices are known by construction, and the device form must equal the host form on the same bytes."""
import numpy as np
import pytest

import count_seams as S
import damage as D
import oracle
import test_gpu_records_elems as RE
from test_gpu_records_dev import _same_as_host
from test_gpu_records_dev import ctx, master5      # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
R, C = S.POOL_SHAPE
ROUND = 1024
COUNTS = [1023, 1024, 1025, 2049, 3100]
PAST = [1025, 2049, 3100]                         # the counts that have a record number 1,024
CYCLE = (0, 1, 3, 4, None)                        # codec indices of LIST5; None: the standard form
N_POOL = 40


class Pool:
    def __init__(self):
        self.tiles, self.packs = S.partition_pool(N_POOL)
        self.extra = []

    def forms(self, element):
        """the flat list assemble() draws from: entry CYCLE.index(slot) * 40 + k is tile k in the form `slot`"""
        flat = []
        for slot in CYCLE:
            flat += S.standard_form(self.tiles, element) if slot is None else self.packs[slot]
        return flat

    def want(self, seq, element):
        return self.tiles[seq].astype(np.int16 if element == "short" else np.int32)


@pytest.fixture(scope="module")
def pool():
    return Pool()


def _indices(n):
    return (np.arange(n, dtype=np.int64) * 7 + 1000).astype(np.int32)


def _which(slots, seq):
    return np.array([CYCLE.index(s) for s in slots]) * N_POOL + seq


def _run(master, pool, slots, element="int", seed=1, verify=(True,)):
    """a batch whose record t holds tile seq[t] in the form slots[t]: every record decodes to its tile, device form = host form"""
    n = len(slots)
    seq = S.sequence(seed, n, ROUND, N_POOL)
    blob, offsets = S.assemble(pool.forms(element), _which(slots, seq), _indices(n))
    for v in verify:
        idx, vals, st = _same_as_host(master, R, C, blob, offsets, element, v, (n, element))
        assert (st == 0).all(), np.flatnonzero(st)[:8]
        assert np.array_equal(idx, _indices(n))
        wrong = np.flatnonzero((vals != pool.want(seq, element)).any(axis=1))
        assert wrong.size == 0, (n, element, wrong[:8], [slots[t] for t in wrong[:8]])


def _alternating(n, shift=0):
    return [CYCLE[(t + shift) % 5] for t in range(n)]


@pytest.mark.parametrize("element", ["int", "short"])
@pytest.mark.parametrize("n", COUNTS)
def test_codecs_alternating_from_record_to_record(master5, pool, n, element):
    _run(master5, pool, _alternating(n), element, seed=n, verify=(True, False) if n == 2049 else (True,))


@pytest.mark.parametrize("n", PAST)
@pytest.mark.parametrize("layout", ["huffman round first", "huffman round last", "one deflate record at 1024"])
def test_segments_that_exist_in_one_round_only(master5, pool, layout, n):
    """a segment whose members all lie in round 0 and four that begin in round 1; the mirror image; a segment whose only member is
    the first record of round 1 (run[] of the others carried, its own counted from zero)"""
    if layout == "one deflate record at 1024":
        others = (0, 3, 4, None)
        slots = [others[t % 4] for t in range(n)]
        slots[ROUND] = 1
    else:
        rest = (1, 3, 4, None)
        slots = [0] * ROUND + [rest[t % 4] for t in range(n - ROUND)]
        if layout == "huffman round last":
            slots = slots[::-1]
    _run(master5, pool, slots, seed=n + len(layout))


@pytest.mark.parametrize("n", PAST)
def test_a_segment_that_straddles_the_seam_inside_one_wave(master5, pool, n):
    """records 1,000 .. 1,050 are all canonical (the last wave of round 0 and the first of round 1), the codec changes with every
    record around them"""
    slots = _alternating(n)
    for t in range(1000, min(1051, n)):
        slots[t] = 3
    _run(master5, pool, slots, seed=n + 50)


@pytest.mark.parametrize("n", [2049, 3100])
def test_failed_records_at_the_seam(master5, pool, n):
    """bad framing at 1,023 (type byte 3, the checksum made good), a flipped checksum bit at 1,024, a damaged Huffman packing at
    1,025: failed records take no place in the partition, every other record decodes, the three get the host form's verdicts"""
    cases = D.damage_set(pool.packs[0][7], D.HUFFMAN, R, C, seed=17)
    bad = None
    for label, p in cases:
        if len(p) and p[0] == 0 and len(p) != 4 * R * C and D.deviation(p, D.HUFFMAN, R * C) is None:
            try:
                oracle.codec_huffman_decode(R, C, p)
            except IOError:
                bad = bytes(p)
                break
    assert bad is not None
    slots = _alternating(n)
    seq = S.sequence(n + 9, n, ROUND, N_POOL)
    forms = pool.forms("int") + [bad]
    which = _which(slots, seq)
    which[ROUND + 1] = len(forms) - 1
    blob, offsets = S.assemble(forms, which, _indices(n))
    o = offsets.astype(np.int64)
    blob[o[ROUND - 1] + 4] = 3
    rec = blob[o[ROUND - 1]:o[ROUND]]
    rec[-4:] = np.array([S.crc32c_rows(rec[None, :-4])[0]], "<u4").view(np.uint8)
    blob[o[ROUND + 1] - 2] ^= 0x10
    three = [ROUND - 1, ROUND, ROUND + 1]
    for verify in (True, False):
        idx, vals, st = _same_as_host(master5, R, C, blob, offsets, "int", verify, (n, verify))
        assert st[ROUND - 1] == -1 and st[ROUND] == (-1 if verify else 0) and st[ROUND + 1] in (-1, -2), st[three]
        others = np.delete(np.arange(n), three if verify else three[::2])
        assert (st[others] == 0).all() and np.array_equal(idx[others], _indices(n)[others])
        assert np.array_equal(vals[others], pool.tiles[seq][others])
        assert idx[ROUND - 1] == -1


def _float_values(tiles):
    return (tiles.astype(np.float64) / 7.0).astype(np.float32)


@pytest.mark.parametrize("n_tiles,set_name", [(400, "three"), (1025, "three"), (65, "sixteen")])
def test_several_elements(master5, pool, n_tiles, set_name):
    """instances lie element-major (i = e * nTiles + t): the round seam falls inside an element.  Element e of record t holds pool
    tile (seq[t] + e) mod 40 in a form that changes with t + e; the sequence keeps apart every two tiles whose instances, of any
    two elements, lie a whole number of rounds apart.  The "three" set is SHORT, int-coded float and FLOAT (the float element in
    standard form and as a CodecFloat packing under the list's entry 2); sixteen INT elements otherwise."""
    elems = RE.ELEMS3 if set_name == "three" else ["int"] * 16
    ne = len(elems)
    assert n_tiles * ne > ROUND
    shifts = S.instance_shifts(n_tiles, ne, ROUND)
    seq = S.sequence(n_tiles + ne, n_tiles, shifts, N_POOL)
    fl = _float_values(pool.tiles)
    fpacks = [oracle.codec_float_encode(2, R, C, v.view(np.uint32), level=6) for v in fl]
    forms = {"short": pool.forms("short"), "int": pool.forms("int")}

    def element(e, k, f):
        kind = elems[e] if isinstance(elems[e], str) else "icf"
        k = (k + e) % N_POOL
        if kind == "float":
            return fpacks[k] if (f + e) % 2 and len(fpacks[k]) < 4 * R * C else fl[k].astype("<f4").tobytes()
        return forms["short" if kind == "short" else "int"][((f + e) % 5) * N_POOL + k]
    entries = [[element(e, k, f) for e in range(ne)] for f in range(5) for k in range(N_POOL)]
    which = (np.arange(n_tiles) % 5) * N_POOL + seq
    blob, offsets = S.assemble(entries, which, _indices(n_tiles))
    want = []
    for e, el in enumerate(elems):
        t = pool.tiles[(seq + e) % N_POOL]
        want.append(t.astype(np.int16) if el == "short" else fl[(seq + e) % N_POOL] if el == "float" else
                    RE._icf_expect(t, el) if not isinstance(el, str) else t)
    dev = master5.record_blob_elems_dev(R, C, blob, offsets, elems, verify_checksums=True)
    host = master5.record_blob_elems(R, C, blob, offsets, elems, verify_checksums=True)
    for what, (idx, vals, st) in (("device", dev), ("host", host)):
        assert st.shape == (ne, n_tiles) and (st == 0).all(), (what, np.argwhere(st)[:8])
        assert np.array_equal(idx, _indices(n_tiles)), what
        for e in range(ne):
            a, b = np.ascontiguousarray(vals[e]), np.ascontiguousarray(want[e])
            wrong = np.flatnonzero((a.view(np.uint8) != b.view(np.uint8)).reshape(n_tiles, -1).any(axis=1))
            assert wrong.size == 0, (what, "element", e, "tiles", wrong[:8])


@pytest.mark.parametrize("n", [1025, 2049])
def test_packings_without_framing(master5, pool, n):
    slots = [(0, 1, 3, 4)[t % 4] for t in range(n)]
    seq = S.sequence(n + 3, n, ROUND, N_POOL)
    packs = [pool.packs[s][k] for s, k in zip(slots, seq)]
    hv, hs = master5.decode_batch(R, C, packs)
    dv, ds = master5.decode_batch_dev(R, C, packs)
    assert (hs == 0).all() and np.array_equal(ds, hs) and np.array_equal(dv, hv)
    assert np.array_equal(dv, pool.tiles[seq])


@pytest.mark.parametrize("element", ["int", "short"])
@pytest.mark.parametrize("n", [1025, 2049])
def test_one_codec_only(master5, pool, n, element):
    """counts[k] == n: for INT cells the partition is the identity and the decoder writes straight to the caller's arrays; for
    SHORT cells the shortcut must not be taken (the decoded ints are narrowed on their way)"""
    _run(master5, pool, [3] * n, element, seed=n + 77, verify=(True, False))
