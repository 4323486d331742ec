"""The conditions tests/test_gpu_encode_bounds.py relies on, proved with the oracle alone: every family of tests/slot_edges.py
reaches the lengths around its stride, keeps the batch order the write-bound checks need, has the content that selects its packer,
and is deterministic."""
import numpy as np
import pytest

import oracle
import slot_edges as se
import value_edges as ve

M32 = [(se.m32, (0,)), (se.m32, (1,))]
ALL = se.SMALL_FAMILIES + M32 + [(se.huffman_general, ())]


@pytest.fixture(scope="module", params=ALL, ids=se.family_id)
def family(request):
    fn, args = request.param
    return fn(*args)


def test_stride_is_legal_and_lengths_reach_its_edges(family):
    f = family
    S = f.stride
    assert S % 16 == 0 and S >= (64 if f.codec in ("lsop", "lsop08") else 16)
    have = set(f.all_lengths)
    if f.relaxed:                         # huffman general: one packing within 16 bytes under S, one within 16 bytes over
        assert any(S - 16 <= L <= S for L in f.lengths if L) and any(S < L <= S + 16 for L in f.lengths)
        return
    m = f.margin()
    # S - 1, S, S + 1 (m32: S - 9, S - 8, S - 7) and every way of filling the last word: S - 3 .. S
    assert all(S - m + o in have for o in (-3, -2, -1, 0, 1)), sorted(L for L in have if abs(L - S + m) < 8)
    assert {L % 4 for L in have if S - m - 3 <= L <= S - m} == {0, 1, 2, 3}
    batch = {L for x in f.lengths for L in (x if isinstance(x, tuple) else (x,))}
    assert all(S - m + o in batch for o in (-3, -2, -1, 0, 1)), "the batch lost an edge length"
    if f.codec != "m32":                  # a few tiles far below S and a few far above (m32: the ladder's two ends, wherever they lie)
        assert min(batch - {0}) < S - se.NEAR and max(batch) > S + se.NEAR


def test_oracle_packings_and_statuses(family):
    """the recorded packing, predictor and length of every tile are the oracle's for the family's arguments, and all three
    statuses occur (m32: GF_OK and GF_OVERFLOW; its tiles always have a candidate)"""
    f = family
    for t in range(f.n):
        if f.codec == "m32":
            streams, models, seed = se.m32_candidates(f.nr, f.nc, f.tiles[t])
            assert streams == f.packs[t] and models == f.preds[t] and seed == f.seeds[t]
            continue
        pk, pred = se.encode_one(f.codec, f.nr, f.nc, f.tiles[t], f.mask, f.lsop_flags)
        assert pk == f.packs[t] and pred == f.preds[t] and f.lengths[t] == (len(pk) if pk else 0), t
    st = [f.expected_status(t) for t in range(f.n)]
    assert se.OK in st and se.OVERFLOW in st and (f.codec == "m32" or se.DECLINED in st)
    assert f.guard() >= se.GUARD and f.guard() % 16 == 0 and f.guard() >= max(max(x) if isinstance(x, tuple) else x for x in f.lengths)


@pytest.mark.parametrize("entry", [e for e in ALL if e[0] is not se.m32], ids=se.family_id)
def test_batch_order(entry):
    """every tile with S - 3 <= L <= S is followed by a tile that writes nothing (all-null, or L > S), the first tile has L == S,
    the last one is an edge tile too"""
    f = entry[0](*entry[1])
    S = f.stride
    silent = [f.expected_status(t) != se.OK for t in range(f.n)]
    lo = 16 if f.relaxed else 3
    edge = [t for t in range(f.n) if f.packs[t] is not None and S - lo <= f.lengths[t] <= S]
    assert edge[0] == 0 and edge[-1] == f.n - 1 and (f.relaxed or f.lengths[0] == S)
    assert all(silent[t + 1] for t in edge[:-1]), [t for t in edge[:-1] if not silent[t + 1]]


def test_m32_neighbours():
    """m32 (the neighbour of a stream is the tile's next sub-slot).  Differencing at the edge: every stream of S - 11 .. S - 8 bytes
    lies in front of a sub-slot that stays untouched.  Linear at the edge: tiles with a candidate that does not fit between two that
    do.  Both: tiles with nulls leave sub-slots 1 and 2 without a candidate."""
    f = se.m32(0)
    S = f.stride
    for L in range(S - 11, S - 7):
        assert any(x[0] == L and x[1] + 8 > S for x in f.lengths), L
    g = se.m32(1)
    S = g.stride
    assert any(x[0] + 8 <= S < x[1] + 8 and x[2] + 8 <= S for x in g.lengths)
    for L in range(S - 11, S - 7):
        assert any(x[1] == L for x in g.lengths), L
    for h in (f, g):
        assert any(p[1] is None for p in h.packs) and any(p[1] is not None for p in h.packs)
        st = [h.expected_status(t) for t in range(h.n)]
        assert se.OK in st and se.OVERFLOW in st


def _fitting(f):
    """the tiles that are packed (the others' content selects nothing)"""
    return [t for t in range(f.n) if f.expected_status(t) == se.OK]


def test_content_selects_the_packer():
    nr, nc = se.SMALL
    for m in (1, 2, 3):
        f = se.huffman_plane(m)
        ok = _fitting(f)
        assert nc >= 8 and all(f.preds[t] == m and se.is_plain(m, nr, nc, f.tiles[t]) and se.keeps_plane(nr, nc, f.tiles[t]) for t in ok)
        f = se.huffman_flatplain(m)
        ok = _fitting(f)
        assert f.nc < 8 and all(f.preds[t] == m and se.is_plain(m, f.nr, f.nc, f.tiles[t]) for t in ok)
        f = se.huffman_wide(m)
        ok = _fitting(f)
        assert all(f.preds[t] == m and not se.is_plain(m, nr, nc, f.tiles[t]) for t in ok)
        wide = [int((np.abs(se.residuals(m, nr, nc, f.tiles[t])) > 126).sum()) for t in ok]
        assert 1 <= min(wide) and max(wide) <= nr * nc // 20, wide       # "a few": under 5 % of the stream
        f = se.canon_plain(m)
        ok = [t for t in _fitting(f) if len(f.packs[t]) > 6]
        assert all(f.preds[t] == m and max(ve.canon_kind(x) for x in se.residuals(m, nr, nc, f.tiles[t])) == 0 for t in ok)
        assert any(f.packs[t] is not None and len(f.packs[t]) == 6 for t in range(f.n)), "no uniform tile"
    for f in (se.huffman_nulls(), se.canon_nulls()):
        assert all(f.preds[t] == ve.NULLS for t in _fitting(f) if len(f.packs[t]) > 6)
    f = se.canon_escape()
    for t in range(f.n):
        if f.packs[t] is not None:
            kinds = {ve.canon_kind(x) for x in se.residuals(f.preds[t], nr, nc, f.tiles[t])}
            assert kinds >= {0, 1, 2, 3, 4, 5, 6}, (t, kinds)
            assert np.array_equal(oracle.codec_canon_decode(nr, nc, f.packs[t]), f.tiles[t])
    f = se.huffman_rare()
    assert all(se.rare_bits(f.nr, f.nc, f.tiles[t], 1) >= se.RARE_BITS for t in range(f.n) if f.packs[t] is not None)
    for g in [se.huffman_plane(1), se.huffman_wide(2), se.huffman_nulls()]:        # ... and the other families stay with k_huffman_pack
        assert all(se.rare_bits(g.nr, g.nc, g.tiles[t], g.preds[t]) < se.RARE_BITS for t in range(g.n) if g.packs[t] is not None)
    assert se.lsop16_eligible(*se.SMALL) and not se.lsop16_eligible(*se.LSOP_WIDE)
    assert se.lsop16_eligible(se.LSOP_WIDE[0], se.LSOP_WIDE[1] - 1), "a smaller shape is refused too"
    for wide in (False, True):
        a, b = se.lsop(wide, False), se.lsop(wide, True)
        assert min(x for x in b.all_lengths) - min(x for x in a.all_lengths) == 4          # the checksum: header 55 -> 59 bytes
        assert all(p is None or (p[1] & 0x80) for p in b.packs) and all(p is None or not (p[1] & 0x80) for p in a.packs)


def test_lsop08_families():
    """the LSOP08 families: tiles of a batch start at every alignment a cell count that is no multiple of 4 gives, every packing is
    the Huffman container (type 0, what the device encoder writes) and decodes to its tile by the restatement, and no slot is
    larger than gf_lsop08_max_packing needs it (the stride lies below it: a slot that is too small is a caller's choice)"""
    import gridfour_amd
    import lsop08_ref as R
    for wide in (False, True):
        f = se.lsop08(wide)
        assert f.cells % 4 != 0 and (f.nr, f.nc) == (se.LSOP_WIDE if wide else se.LSOP08_ODD)
        assert 64 <= f.stride < gridfour_amd.lib().gf_lsop08_max_packing(f.nr, f.nc)
        for t in range(f.n):
            if f.packs[t] is not None:
                assert f.packs[t][:3] == bytes([0, 0x40, 8])
        for t in (0, f.n - 1):
            assert np.array_equal(R.decode(f.nr, f.nc, f.packs[t]), f.tiles[t])


def test_uniform_family_at_the_smallest_stride():
    """S = 16: all three statuses; the uniform tiles (6 bytes, predictor 0, the oracle decodes them) are the only ones that fit;
    the varied tiles cover every predictor and the escapes; each uniform tile but the last is followed by a tile that writes
    nothing, the first and the last tile are uniform"""
    f = se.canon_uniform()
    assert f.stride == 16
    st = [f.expected_status(t) for t in range(f.n)]
    assert st.count(se.OK) >= 4 and st.count(se.OVERFLOW) >= 6 and st.count(se.DECLINED) >= 2
    fit = [t for t in range(f.n) if st[t] == se.OK]
    assert fit[0] == 0 and fit[-1] == f.n - 1 and all(st[t + 1] != se.OK for t in fit[:-1])
    for t in fit:
        assert f.lengths[t] == 6 and f.preds[t] == 0 and len(set(f.tiles[t].tolist())) == 1
        assert np.array_equal(oracle.codec_canon_decode(f.nr, f.nc, f.packs[t]), f.tiles[t])
    over = [t for t in range(f.n) if st[t] == se.OVERFLOW]
    assert {f.preds[t] for t in over} >= {1, 2, 3, 4} and min(f.lengths[t] for t in over) > 16, sorted({f.preds[t] for t in over})
    assert f.guard() >= max(f.lengths)


def test_lsop_eligibility_restated_from_the_source():
    """slot_edges.lsop16_eligible restates gf_lsop_predict16_eligible, and no GPU report says which form of k_canon_pack2 ran:
    the rule's terms are looked up in gvrs_lsop.hip, so that a change of the rule fails here and the restatement is looked at"""
    import os
    src = open(os.path.join(os.path.dirname(os.path.abspath(se.__file__)), "..", "gridfour_amd", "csrc", "gvrs_lsop.hip")).read()
    body = src[src.index("bool gf_lsop_predict16_eligible(int nRows, int nCols)"):]
    body = " ".join(body[:body.index("}")].split())
    assert "nRows >= 6 && nCols >= 6 && (size_t)nCols <= LSOP_RING_MAXC && nInt < (1u << 17) &&" in body
    assert "2 * ((nCells + 64 + 15) & ~(size_t)15) + sizeof(LsopShared16) <= 150 * 1024" in body
    assert "LSOP_RING_MAXC = %d" % se.LSOP_RING_MAXC in " ".join(src.split())


def test_general_family_shape():
    import route_plan as rp
    f = se.huffman_general()
    assert f.nr >= 2 and 6 * f.cells >= 1 << 23 and f.n == 5
    p = rp.plan(rp.KIND_HUFFMAN, f.nr, f.nc, f.n)
    assert p.encBits & rp.ENC_GENERAL and not p.encBits & rp.ENC_SPLIT


def test_families_are_deterministic():
    for fn, args in ALL[:3] + [(se.canon_escape, ()), (se.lsop, (False, True)), (se.m32, (0,))]:
        a = fn(*args)
        fn.cache_clear()
        b = fn(*args)
        assert a is not b and a.stride == b.stride and a.lengths == b.lengths and a.packs == b.packs
        assert np.array_equal(a.values(), b.values())


def test_compact_order_covers_every_alignment():
    order = se.compact_order()
    assert sorted(order) == sorted(L for L in se.COMPACT_LENGTHS for _ in range(4))
    off, seen = 0, set()
    for L in order:
        if L:
            seen.add((L < 8, off % 4))
        off += L
    assert seen == {(s, m) for s in (True, False) for m in range(4)}
    slots, cat = se.compact_slots(order)
    assert len(cat) == sum(order) and se.SENTINEL not in cat
