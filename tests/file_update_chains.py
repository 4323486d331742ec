"""Test-only: the inputs that take the in-place update (gridfour_amd/csrc/gvrs_file_update.hip) past the seams of its launches,
built on tests/file_update_cases.py and shared by tests/test_file_update_chains_inputs.py (no GPU: the inputs do what they claim,
and the host assembler equals the model on them) and tests/test_gpu_file_update_chains.py.
  directed(n)        files whose list has n nodes AT OPEN, and one update each that makes one list event at a stated node index
  chain_start/round  seeded chains of updates: a round's input image is the previous round's output
  fill_case          files whose FINAL list sums to a stated number of bytes: k_update_fill's grid-stride loop past its first turn
  judge_cases        131 records with one refusal planted at a stated index: k_update_alloc's judging loop past its first turn
  batch              257 .. 399 records with empty ones on the 256-word seams of the blob: k_update_patch and k_update_copy
The launch numbers these rest on: 64 nodes (and 64 records) a turn of the one wave, workgroups of 256 lanes, at most 1024
workgroups in the fill."""
import ctypes as C
import functools
import struct

import numpy as np

import file_update_cases as U
import gvrs_file_update_ref as R

TURN = 64                                 # nodes (wl_*) and records (the judging loop) a turn of k_update_alloc
GROUP = 256                               # lanes of a workgroup of k_update_patch / _copy / _fill: a lane a record, a lane a word
FILL_GROUPS = 1024                        # k_update_fill's cap
FILL_TURN = FILL_GROUPS * GROUP * 8       # the bytes of free space one turn of its grid-stride loop covers: 2^21
N_NODES = (64, 65, 66, 128, 129, 130)
NEW_TILE = 399                            # no layout here gives it a record


# ---- directed long-list cases ----
def node_size(j):
    """Node j of a long file.  Ascending, so that no earlier node holds a record made for node k; a step of 24, so that a record
    32 bytes smaller than node k is no earlier node's size."""
    return 40 + 24 * j


def long_file(n, gaps=None, checksums=True):
    """A file whose list has n nodes after opening: n - 1 nodes of node_size(j) in the free-space directory and, behind the last
    record, the two directories, which opening frees into one trailing node (the largest).  In front of node j stand gaps[j] tile
    records of 24 bytes (default 2) -> (image, {(j, slot): tile index})"""
    gaps = gaps or {}
    layout, tile_of, t = [], {}, 0
    for j in range(n):
        for slot in range(gaps.get(j, 2)):
            layout.append(("t", t, 24))
            tile_of[(j, slot)] = t
            t += 1
        if j < n - 1:
            layout.append(("f", node_size(j)))
    assert t <= NEW_TILE
    return U.make_file(layout, checksums, grid=U.BIG_GRID), tile_of


@functools.lru_cache(maxsize=None)
def directed(n):
    """{name: (image, records, tiles, wanted)}: one update each, `wanted` its one list event as the model's log states it, with the
    node index and the list's length before it.  An index the list of n nodes does not have makes no case."""
    cases = {}

    def put(name, gaps, writes, wanted):
        image, tile_of = long_file(n, gaps)
        records, tiles = U.writes_of([(tile_of[t] if isinstance(t, tuple) else t, z) for t, z in writes])
        cases[name] = (image, records, tiles, wanted)

    # an exact fit erases node k: n - 1 - k nodes move down, 64 a turn
    for k in sorted({0, 1, n - 65, n - 66}):
        if 0 <= k <= n - 2:
            put(f"exact fit of node {k}: {n - 1 - k} behind", None, [(NEW_TILE, node_size(k))], ("alloc", "exact", None, node_size(k), 0, k, n))
    for k in (1, 64, 65):
        if k <= n - 1:
            # the one record between node k - 1 and node k: both merge, node k is erased
            put(f"free merges both at {k}", {k: 1}, [((k, 0), 0)], ("free", "both", None, 24, k, n))
    for k in (64, 65):
        if k <= n - 1:
            put(f"free merges prior at {k}", None, [((k, 0), 0)], ("free", "prior", None, 24, k, n))
            put(f"free merges next at {k}", None, [((k, 1), 0)], ("free", "next", None, 24, k, n))
        if k <= n - 2:
            z = node_size(k) - 32
            put(f"split of node {k}", None, [(NEW_TILE, z)], ("alloc", "split", None, z, 32, k, n))
    for move in (63, 64, 65, 128, 129):
        k = n - move
        if k >= 0:
            # the middle one of three records: no node touches it
            put(f"insert moves {move}", {k: 3}, [((k, 1), 0)], ("free", "insert", None, 24, k, n))
    image, _ = long_file(n)
    trailing = R.RefUpdate(image, U.BIG_TILE_COLS, True).free[-1][1]
    assert trailing > node_size(n - 2) + 32
    put("overwrite-last", None, [(NEW_TILE, trailing + 8)], ("alloc", "overwrite-last", None, trailing + 8, n))
    put("append", None, [(NEW_TILE, trailing - 8)], ("alloc", "append", None, trailing - 8, n))    # (8 too large for a split)
    return cases


# ---- seeded chains ----
CHAINS = ((11, 5, True), (12, 5, True), (13, 6, False))           # (seed, rounds, checksums)
CHAIN_GRID = (1280, 1280, 64, 64)         # 20 x 20 tiles as U.BIG_GRID has, of 64 x 64 cells: the inspector passes a tile record of up
MAX_RECORD = (4 + 4 + 4 * 64 * 64 + 12 + 7) & ~7                   # to the standard form's size, and the chains' last images are inspected


def chain_start(seed, checksums=True):
    """300 records of 24 .. 96 bytes on the 400 tiles and 129 nodes scattered between them.  The nodes' sizes rise along the file
    (24 + 8 j and up to 16 more), so that a record made for a node far down the list fits no node in front of it: the first-fit
    search, and the erase or the split it ends in, reach the list's later turns."""
    rng = np.random.default_rng([seed, 0])
    tiles = rng.permutation(400)[:300]
    node_at = set(rng.choice(np.arange(1, 300), 129, replace=False).tolist())
    layout, j = [], 0
    for k, t in enumerate(tiles):
        if k in node_at:
            layout.append(("f", 24 + 8 * (j + int(rng.integers(0, 3)))))
            j += 1
        layout.append(("t", int(t), 24 + 8 * int(rng.integers(0, 10))))
    return U.make_file(layout, checksums, grid=CHAIN_GRID)


def chain_round(seed, rnd, image, checksums=True):
    """Round rnd (from 1) on `image`: 40 .. 120 writes on distinct tiles -> (records, tiles, status).  A tile with a record is
    freed, replaced by a record up to 40 bytes smaller or larger, or keeps it under a negative status; a tile without one gets a
    record of a node's size (an exact fit), 32 smaller (a split that leaves the smallest surplus) or 32 larger -- one time in
    ten than the LARGEST node, which no node holds: the file's end --, a record under a negative status, or is declined."""
    rng = np.random.default_rng([seed, rnd])
    m = R.RefUpdate(image, U.BIG_TILE_COLS, True)
    free_sizes = [z for _, z in m.free]
    old = {row * U.BIG_TILE_COLS + col: struct.unpack_from("<i", image, p - 8)[0] for (row, col), p in m.offsets.items() if p}
    writes, status = [], []
    for t in rng.permutation(400)[:int(rng.integers(40, 121))].tolist():
        z, u = old.get(t, 0), rng.random()
        if z and u < 0.30:
            w, st = 0, R.DECLINED
        elif z and u < 0.86:
            w, st = max(24, z + 8 * int(rng.integers(-5, 6))), 0
        elif z:
            w, st = z + 8, -int(rng.integers(1, 9))
        elif u < 0.80:
            if rng.random() < 0.1:
                w, st = max(free_sizes) + 32, 0
            else:
                w, st = free_sizes[int(rng.integers(len(free_sizes)))] + 32 * int(rng.integers(-1, 2)), 0
                w = w if w >= 24 else w + 32
        elif u < 0.90:
            w, st = 40, -int(rng.integers(1, 9))
        else:
            w, st = 0, R.DECLINED
        writes.append((t, min(w, MAX_RECORD)))
        status.append(st)
    records, tiles = U.writes_of(writes, checksums, seed=rnd)
    return records, tiles, status


# ---- the fill ----
MEDIUM = 1 << 16
FILLS = {"one turn": FILL_TURN, "one word into the second turn": FILL_TURN + 8, "into the third turn": 2 * FILL_TURN + (1 << 19) + 16}


@functools.lru_cache(maxsize=None)
def fill_case(total, several):
    """A file of adjacent records of 64 KiB and the update that frees them all, after which the model's FINAL list sums to
    exactly `total` bytes (the first of the records is sized for that) -> (image, records, tiles).  The freed records merge into
    one node, or with `several` into three of about a third each, kept apart by a small record."""
    n_medium = total // MEDIUM
    regions = [n_medium // 3, n_medium // 3, n_medium - 2 * (n_medium // 3)] if several else [n_medium]

    def build(first):
        layout, writes, t = [("t", 390, 24)], [], 0
        for k, count in enumerate(regions):
            for _ in range(count):
                layout.append(("t", t, first if t == 0 else MEDIUM))
                writes.append((t, 0))
                t += 1
            layout.append(("t", 391 + k, 24))
        return U.make_file(layout, grid=U.BIG_GRID), writes

    image, writes = build(MEDIUM)
    records, tiles = U.writes_of(writes)
    _, _, final, _, _ = U.model(image, records, tiles, n_tile_cols=U.BIG_TILE_COLS)
    image, writes = build(MEDIUM + total - sum(z for _, z in final))
    return image, records, tiles


# ---- the judging loop ----
JUDGE_AT = (63, 64, 65, 130)


@functools.lru_cache(maxsize=None)
def judge_cases():
    """-> (image, blob, {name: (offsets, tiles)}): 131 records of 24 .. 96 bytes on 131 tiles, some with an old record, some
    without, all valid ("valid"), and one thing the update refuses planted at record 63, 64, 65 or 130"""
    image, _ = long_file(66)
    rng = np.random.default_rng(131)
    tiles = np.arange(100, 231, dtype=np.int32)
    records, _ = U.writes_of([(int(t), 24 + 8 * int(rng.integers(0, 10))) for t in tiles])
    blob = np.frombuffer(b"".join(records) + b"\0" * 16, np.uint8)
    offsets = np.zeros(132, np.uint64)
    offsets[1:] = np.cumsum([len(r) for r in records])
    cases = {"valid": (offsets, tiles)}

    def put(name, at, value, of_tiles=False):
        o, t = offsets.copy(), tiles.copy()
        (t if of_tiles else o)[at] = value
        cases[name] = (o, t)

    for i in JUDGE_AT:
        put(f"o1 < o0 at {i}", i + 1, offsets[i] - np.uint64(8))
        put(f"an offset no multiple of 8 at {i}", i, offsets[i] + np.uint64(4))
        o = offsets.copy()
        o[i + 1:] -= o[i + 1] - o[i] - np.uint64(16)
        cases[f"a length of 16 at {i}"] = (o, tiles)
        put(f"tile -1 at {i}", i, -1, True)
        put(f"tile nTilesGrid at {i}", i, 400, True)
        put(f"a duplicate tile at {i}", i, tiles[i - 1], True)
    put("a duplicate pair at (3, 64)", 64, tiles[3], True)
    put("a duplicate pair at (63, 128)", 128, tiles[63], True)
    return image, blob, cases


def assemble_raw(image, blob, offsets, tiles):
    """gf_file_update_assemble with the caller's own offsets -> (status, the buffer, the size): as update_assemble calls it"""
    from gridfour_amd import GvrsFileHip
    from gridfour_amd._lib import lib
    f = GvrsFileHip(image)
    u = f.update_begin()
    cap = u.plan()[0]
    buf = np.full(cap, 0xA5, np.uint8)
    buf[:len(image)] = np.frombuffer(image, np.uint8)
    need = C.c_uint64()
    rc = lib().gf_file_update_assemble(u.handle, C.c_void_p(buf.ctypes.data), cap, C.c_void_p(blob.ctypes.data), C.c_void_p(offsets.ctypes.data),
                                       C.c_void_p(tiles.ctypes.data), None, tiles.size, U.TIME, 0, C.byref(need))
    u.end()
    return rc, buf.tobytes(), need.value


# ---- patch and copy ----
SEAM = GROUP * 8                          # the bytes of the blob one workgroup of k_update_copy takes
BATCHES = (257, 300, 399)


@functools.lru_cache(maxsize=None)
def batch(n):
    """n records in one update of a chain's first file: sizes 24 .. 96, about a third empty (a free where the tile has a record,
    declined where it has none), and the sizes steered so that every multiple of 256 words inside the blob is the end of one
    record and the start of another with an empty record (or two) between them -> (image, records, tiles)"""
    image = chain_start(n)
    rng = np.random.default_rng([n, 1])
    sizes, at, on_seam = [], 0, False
    while len(sizes) < n:
        if at and at % SEAM == 0 and not on_seam:
            sizes += [0] * int(rng.integers(1, 3))
            on_seam = True
            continue
        if rng.random() < 0.28:
            sizes.append(0)
            continue
        z, d = 24 + 8 * int(rng.integers(0, 10)), SEAM - at % SEAM
        if 24 <= d <= 96:
            z = d
        elif d - z < 24:
            z = d - 24
        assert 24 <= z <= 96
        sizes.append(z)
        at += z
        on_seam = False
    records, tiles = U.writes_of(list(zip(rng.permutation(400)[:n].tolist(), sizes[:n])), seed=n)
    return image, records, tiles
