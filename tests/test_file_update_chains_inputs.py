"""The inputs of tests/file_update_chains.py, checked without a GPU: every directed case makes the list event it names at the node
index and list length it names, on a list of n nodes at open; the chains meet their coverage condition; the fill's files sum to
their totals on the model's FINAL list; the judge's inputs are refused by the host assembler; the batches have their empty
records on the blob's 256-word seams.  On every case and every round the host assembler (gf_file_update_assemble) equals the
model (tests/gvrs_file_update_ref.py) byte for byte, and the result keeps the file's invariants."""
import numpy as np
import pytest

import file_update_cases as U
import file_update_chains as K
from gridfour_amd import GvrsFileHip, _lib


def both(image, records, tiles, status=None):
    """the assembler equals the model -> (image, opened list, final list, log of the tile writes)"""
    want, opened, final, writes, _ = U.model(image, records, tiles, status, n_tile_cols=U.BIG_TILE_COLS)
    f = GvrsFileHip(image)
    u = f.update_begin()
    assert u.free_list == opened
    got = f.update_assemble(u, records, tiles, U.TIME, status)
    u.end()
    assert got == want
    U.check_invariants(got, final, U.BIG_TILE_COLS)
    return got, opened, final, writes


def test_the_log_states_index_and_length():
    """the appended fields on the short list of tests/file_update_cases.py, where they can be read off the layout"""
    image, records, tiles, *_ = U.scenario("replace frees first")            # tile 1 lies between node 0 and node 1 of four
    _, opened, _, writes, _ = U.model(image, records, tiles)
    assert len(opened) == 4 and len(writes) == 2
    assert writes[0] == ("free", "both", opened[0][0] + 64, 48, 1, 4)         # node 1 is erased, of four
    assert writes[1] == ("alloc", "split", opened[0][0], 160, 48, 0, 3)       # the merged node of 64 + 48 + 96 bytes, of three
    image, records, tiles, *_ = U.scenario("trailing node too small")
    _, opened, _, writes, _ = U.model(image, records, tiles)
    assert writes == [("alloc", "overwrite-last", opened[-1][0], 2000, 4)]     # the search passed all four
    image, records, tiles, *_ = U.scenario("free without a merge")             # tile 3 lies behind node 1, with records on both sides
    _, opened, _, writes, _ = U.model(image, records, tiles)
    assert writes == [("free", "insert", opened[1][0] + 96 + 56, 72, 2, 4)]


@pytest.mark.parametrize("n", K.N_NODES)
def test_directed_cases(n):
    cases = K.directed(n)
    kinds = {w[:2] for _, _, _, w in cases.values()}
    assert {("alloc", "exact"), ("free", "both"), ("free", "insert"), ("alloc", "overwrite-last"), ("alloc", "append")} <= kinds
    if n > 66:
        assert {("free", "prior"), ("free", "next"), ("alloc", "split")} <= kinds and len(cases) >= 18
    for name, (image, records, tiles, wanted) in cases.items():
        _, opened, final, writes = both(image, records, tiles)
        assert len(opened) == n, name
        assert len({z for _, z in opened}) == n, name                          # distinct sizes: an exact fit names one node
        assert U.holds(writes, [wanted]) and None not in wanted[4:], name
        assert len(writes) == 1, name                                         # one event: nothing else moved the list
    # what the names promise of the shifts: an erase with 63, 64 and 65 nodes behind it and an insert that moves as many
    behind = {w[6] - 1 - w[5] for _, _, _, w in cases.values() if w[:2] == ("alloc", "exact")}
    moved = {w[5] - w[4] for _, _, _, w in cases.values() if w[:2] == ("free", "insert")}
    assert behind & {K.TURN - 1, K.TURN, K.TURN + 1, 2 * K.TURN, 2 * K.TURN + 1} and moved & {63, 64, 65, 128, 129}


def test_directed_cases_reach_every_seam():
    seen = set()
    for n in K.N_NODES:
        for _, _, _, w in K.directed(n).values():
            if w[:2] == ("alloc", "exact"):
                seen.add(("erase behind", w[6] - 1 - w[5]))
            elif w[:2] == ("free", "both"):
                seen.add(("both", w[4], w[5] - 1 - w[4] >= K.TURN))
            elif w[:2] == ("free", "insert"):
                seen.add(("insert moves", w[5] - w[4]))
            elif w[0] == "free" or w[1] == "split":
                seen.add((w[1], w[5] if w[0] == "alloc" else w[4]))
    assert {("erase behind", k) for k in (63, 64, 65, 127, 128, 129)} <= seen
    assert {("insert moves", k) for k in (63, 64, 65, 128, 129)} <= seen
    assert {("both", 1, True), ("both", 64, True), ("both", 65, True)} <= seen
    assert {(kind, k) for kind in ("prior", "next", "split") for k in (64, 65)} <= seen


@pytest.mark.parametrize("seed,n_rounds,checksums", K.CHAINS, ids=[f"seed{c[0]}" for c in K.CHAINS])
def test_chain_coverage(seed, n_rounds, checksums):
    """Over a seed's rounds every list event happens at a node index of 64 or more, at least three rounds open on 65 or more
    nodes, and an erase has 65 or more nodes behind it.  (A generator that misses this gets other parameters, not another
    condition.)"""
    assert n_rounds >= 5
    image = K.chain_start(seed, checksums)
    log, opened_on = [], []
    for rnd in range(1, n_rounds + 1):
        records, tiles, status = K.chain_round(seed, rnd, image, checksums)
        assert 40 <= len(records) <= 120 and any(s < 0 for s in status) and any(s == 1 for s in status) and len(set(tiles)) == len(tiles)
        image, opened, final, writes = both(image, records, tiles, status)
        log += writes
        opened_on.append(len(opened))
    assert opened_on[0] == 130 and sum(n >= K.TURN + 1 for n in opened_on) >= 3
    far = {w[:2] for w in log if (w[4] if w[0] == "free" else w[5] if w[1] in ("split", "exact") else w[4]) >= K.TURN}
    assert {("free", "insert"), ("free", "prior"), ("free", "next"), ("free", "both"), ("alloc", "exact"), ("alloc", "split")} <= far
    assert far & {("alloc", "overwrite-last"), ("alloc", "append")}
    erases = [w[6] - 1 - w[5] for w in log if w[:2] == ("alloc", "exact")] + [w[5] - 1 - w[4] for w in log if w[:2] == ("free", "both")]
    assert max(erases) >= K.TURN + 1


def test_chains_are_fixed():
    assert len(K.CHAINS) >= 3 and any(c[2] for c in K.CHAINS) and not all(c[2] for c in K.CHAINS)
    a, b = K.chain_start(11), K.chain_start(11)
    assert a == b and K.chain_round(11, 1, a) == K.chain_round(11, 1, b) and K.chain_round(11, 1, a) != K.chain_round(11, 2, a)


@pytest.mark.parametrize("several", [False, True], ids=["one node", "several nodes"])
@pytest.mark.parametrize("name", sorted(K.FILLS))
def test_fill_totals(name, several):
    total = K.FILLS[name]
    assert K.FILL_TURN == 1 << 21
    assert {"one turn": total == K.FILL_TURN, "one word into the second turn": total == K.FILL_TURN + 8,
            "into the third turn": total > 2 * K.FILL_TURN + 8}[name]
    image, records, tiles = K.fill_case(total, several)
    got, _, final, _ = both(image, records, tiles)
    assert sum(z for _, z in final) == total                                 # (the model's final list)
    f = GvrsFileHip(image)
    u = f.update_begin()
    assert u.plan()[0] // 8 // K.GROUP + 1 >= K.FILL_GROUPS                    # the room the GPU test gives: the launch has all its workgroups
    u.end()
    assert got[104 + 24] == 1                                                # checksums: a node's last word is written
    sizes = [z for _, z in final]
    if several:
        ends = np.cumsum(sizes)
        assert sum(z > total // 4 for z in sizes) == 3
        if total > 2 * K.FILL_TURN:
            assert any(K.FILL_TURN < e < 2 * K.FILL_TURN for e in ends[:-1])  # a node ends, and the next begins, inside the second turn
    else:
        assert max(sizes) > total - (1 << 16)


def test_judge_inputs_are_refused_by_the_assembler():
    image, blob, cases = K.judge_cases()
    assert len(cases) == 1 + 6 * len(K.JUDGE_AT) + 2
    rc, buf, need = K.assemble_raw(image, blob, *cases["valid"])
    want = U.model(image, [bytes(blob[int(a):int(b)]) for a, b in zip(cases["valid"][0], cases["valid"][0][1:])], cases["valid"][1].tolist(),
                   n_tile_cols=U.BIG_TILE_COLS)[0]
    assert rc == _lib.OK and need == len(want) and buf[:need] == want        # all 131 are valid without the planted one
    for name, (offsets, tiles) in cases.items():
        if name == "valid":
            continue
        assert offsets.size == 132 and tiles.size == 131
        rc, buf, need = K.assemble_raw(image, blob, offsets, tiles)
        assert rc == _lib.ERR_ARG and need == 0, name
        assert buf[:len(image)] == image and set(buf[len(image):]) <= {0xA5}, name


@pytest.mark.parametrize("n", K.BATCHES)
def test_batches(n):
    image, records, tiles = K.batch(n)
    assert len(records) == n > K.GROUP and len(set(tiles)) == n
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in records])])
    empty = [r for r in range(n) if not records[r]]
    assert 0.27 <= len(empty) / n <= 0.42
    assert all(24 <= len(r) <= 96 for r in records if r)
    seams = list(range(K.SEAM, int(offsets[-1]), K.SEAM))
    assert len(seams) >= 4
    for m in seams:                                                          # an empty record stands on every seam of 256 words
        assert any(offsets[r] == m == offsets[r + 1] for r in empty), m
        assert m in offsets[[r for r in range(n) if records[r]]], m          # and a record starts there: the first word of a workgroup
    old = GvrsFileHip(image)
    had = [old.tile_position(t) != 0 for t in tiles]
    assert any(had[r] for r in empty) and any(not had[r] for r in empty)       # frees, and declined without an old record
    _, _, _, writes = both(image, records, tiles)
    assert len(writes) > n // 2
