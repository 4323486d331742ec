"""Test-only: file images with free space and the update scenarios run on them, shared by tests/test_file_update_ref.py (the
model alone), tests/test_file_update_assemble.py (the library's host path against the model) and tests/test_gpu_file_update.py.
No file the reference made has free space, so the images are built here: a LAYOUT is the file's content in file order,
("t", tile, size) a tile record of `size` bytes, ("f", size) a free node; the tile directory and, where there are nodes, the
free-space directory follow.  After opening, the two directories at the file's end are one trailing free node.
tests/file_update_chains.py builds on make_file / writes_of / model: lists that are long AT OPEN, chains, and the launch seams."""
import struct

import gvrs_file_build as B
import gvrs_file_update_ref as R
import gvrs_walk

GRID = (20, 20, 2, 2)                     # 10 x 10 tiles of 2 x 2 cells
N_TILE_COLS = 10
ELEMENTS = [B.element("z", "int")]
TIME = 1_700_000_000_123


def rec(tile, size, checksums=True, seed=0):
    """a tile record of exactly `size` bytes (a multiple of 8, at least 24) for one element"""
    assert size % 8 == 0 and size >= 24
    payload = bytes((tile * 7 + seed + k) & 0xff for k in range(size - 20))
    r = B.frame_record(tile, [payload], checksums)
    assert len(r) == size
    return r


def free_node(size, checksums=True):
    head = struct.pack("<ii", size, 0)
    return head + b"\0" * (size - 12) + struct.pack("<I", R.crc32c(head) if checksums else 0)


def make_file(layout, checksums=True, compression=True, dir_rect=None, extended=False, free_dir_slack=0, grid=GRID):
    """-> the image.  free_dir_slack: the free-space directory record 12 bytes roomier per unit, as the reference may leave it."""
    records, order, gaps, pending = {}, [], {}, b""
    for item in layout:
        if item[0] == "f":
            pending += free_node(item[1], checksums)
        else:
            records[item[1]] = rec(item[1], item[2], checksums)
            gaps[len(order)] = pending
            order.append(item[1])
            pending = b""
    assert not pending, "a layout ends with a tile record (the directories follow)"
    image, _ = B.build_image(grid, ELEMENTS, records, ("GvrsHuffman",) if compression else (), checksums, order=order,
                             between=lambda k: gaps[k], dir_rect=dir_rect, extended=extended)
    nodes = [(pos, size) for pos, size, rtype, _ in gvrs_walk.walk_records(image) if rtype == 0]
    if not nodes:
        return image
    content = struct.pack("<i", len(nodes)) + b"".join(struct.pack("<qi", p, z) for p, z in nodes)
    size = (8 + len(content) + 12 * free_dir_slack + 4 + 7) // 8 * 8
    d = bytearray(struct.pack("<i", size) + bytes([3, 0, 0, 0]) + content)
    d += b"\0" * (size - len(d))
    if checksums:
        struct.pack_into("<I", d, size - 4, R.crc32c(d[:size - 4]))
    b = bytearray(image)
    struct.pack_into("<q", b, 56, len(b) + 8)
    b += d
    return B.refresh_header_crc(bytes(b)) if checksums else bytes(b)


def writes_of(writes, checksums=True, seed=1):
    """[(tile, size or 0)] -> (records, tile indices)"""
    return [rec(t, z, checksums, seed) if z else b"" for t, z in writes], [t for t, _ in writes]


BASE = [("t", 0, 40), ("f", 64), ("t", 1, 48), ("f", 96), ("t", 2, 56), ("t", 3, 72), ("t", 4, 40), ("f", 200), ("t", 5, 88)]

# name -> (layout, writes [(tile, record size; 0: no valid data)], what the model's log of the tile writes must hold, options)
SCENARIOS = {
    "exact fit": (BASE, [(50, 64)], [("alloc", "exact", None, 64)], {}),
    "hole larger by 8 is skipped": (BASE, [(50, 56)], [("alloc", "split", None, 56, 40)], {}),
    "hole larger by 16 is skipped": (BASE, [(50, 48)], [("alloc", "split", None, 48, 48)], {}),
    "hole larger by 24 is skipped": (BASE, [(50, 40)], [("alloc", "split", None, 40, 56)], {}),
    "hole larger by 32 is split": (BASE, [(50, 32)], [("alloc", "split", None, 32, 32)], {}),
    "a larger split": (BASE, [(50, 120)], [("alloc", "split", None, 120, 80)], {}),
    "free without a merge": (BASE, [(3, 0)], [("free", "insert")], {}),
    "free merges with the prior": (BASE, [(5, 0)], [("free", "both")], {}),          # (the last record: the opened directory follows)
    "free merges with the prior only": ([("t", 0, 40), ("f", 64), ("t", 1, 48), ("t", 2, 56)], [(1, 0)], [("free", "prior")], {}),
    "free merges with the next": (BASE, [(4, 0)], [("free", "next")], {}),
    "free merges with both": (BASE, [(1, 0)], [("free", "both")], {}),
    "free the first record": (BASE, [(0, 0)], [("free", "next")], {}),
    "trailing node too small": (BASE, [(50, 2000)], [("alloc", "overwrite-last")], {}),
    "trailing node large enough": (BASE, [(50, 320)], [("alloc", "split")], {}),
    "no node fits": (BASE, [(50, 472)], [("alloc", "append")], {}),                  # (the trailing node is 8 .. 24 larger: see the test)
    "declined without an old record": (BASE, [(50, 0)], [], {}),
    "replace frees first": (BASE, [(1, 160)], [("free", "both"), ("alloc", "split")], {}),
    "negative status": (BASE, [(1, 64), (2, 0), (50, 64)], [("alloc", "exact")], {"status": [-1, -2, 0]}),
    "grow up": ([("t", 44, 40), ("f", 64), ("t", 55, 40)], [(4, 64)], [("alloc", "exact")], {"dir_rect": (4, 4, 2, 2)}),
    "grow down": ([("t", 44, 40), ("f", 64), ("t", 55, 40)], [(94, 64)], [("alloc", "exact")], {"dir_rect": (4, 4, 2, 2)}),
    "grow left": ([("t", 44, 40), ("f", 64), ("t", 55, 40)], [(40, 64)], [("alloc", "exact")], {"dir_rect": (4, 4, 2, 2)}),
    "grow right": ([("t", 44, 40), ("f", 64), ("t", 55, 40)], [(49, 64)], [("alloc", "exact")], {"dir_rect": (4, 4, 2, 2)}),
    "the rectangle never shrinks": ([("t", 44, 40), ("f", 64), ("t", 55, 40)], [(44, 0), (55, 0)], [("free", "next")], {"dir_rect": (4, 4, 2, 2)}),
    "forced extended": (BASE, [(50, 64)], [("alloc", "exact")], {"flags": 1}),
    "extended stays": (BASE, [(50, 64)], [("alloc", "exact")], {"extended": True}),
    "row-major": (BASE, [(10, 64), (11, 96), (12, 40), (1, 200)], [], {}),
    "reversed": (BASE, [(1, 200), (12, 40), (11, 96), (10, 64)], [], {}),
    "permuted": (BASE, [(12, 40), (1, 200), (10, 64), (11, 96)], [], {}),
    "without compression": (BASE, [(1, 48), (50, 64), (3, 72)], [("alloc", "exact")], {"compression": False}),
    "the deviation": (BASE, [(3, 72)], [("free", "insert"), ("alloc", "exact")], {}),
}


def holds(log, wanted):
    """every wanted event, in order, matches an event of the log: None and missing fields match anything"""
    at = 0
    for w in wanted:
        while at < len(log) and not all(x is None or x == y for x, y in zip(w, log[at])):
            at += 1
        if at == len(log):
            return False
        at += 1
    return True


def scenario(name, checksums=True):
    """-> (image, records, tiles, status, flags, compression, wanted log)"""
    layout, writes, wanted, opt = SCENARIOS[name]
    compression = opt.get("compression", True)
    image = make_file(layout, checksums, compression, opt.get("dir_rect"), opt.get("extended", False))
    records, tiles = writes_of(writes, checksums)
    return image, records, tiles, opt.get("status"), opt.get("flags", 0), compression, wanted


def model(image, records, tiles, status=None, flags=0, compression=True, time_modified=TIME, n_tile_cols=N_TILE_COLS):
    return R.ref_update(image, n_tile_cols, compression, records, tiles, time_modified, status, bool(flags & 1))


def check_invariants(image, final_list, n_tile_cols=N_TILE_COLS):
    """the records tile the file exactly; no two nodes touch or overlap; every entry names a tile record with its own index;
    every free record is a node of the list, and the free-space directory states that list"""
    (size,) = struct.unpack_from("<i", image, 16)
    at, free = 16 + size, []
    for pos, z, rtype, _ in gvrs_walk.walk_records(image):
        assert pos == at and z % 8 == 0 and z >= 16
        at += z
        if rtype == 0:
            free.append((pos, z))
    assert at == len(image)
    assert free == list(final_list)
    for (p, z), (q, _) in zip(free, free[1:]):
        assert p + z < q
    fs, md = struct.unpack_from("<qq", image, 56)
    (td,) = struct.unpack_from("<q", image, 80)
    assert struct.unpack_from("<q", image, 48)[0] == 0
    if fs:
        (n,) = struct.unpack_from("<i", image, fs)
        assert image[fs - 4] == 3 and [struct.unpack_from("<qi", image, fs + 4 + 12 * k) for k in range(n)] == free
    else:
        assert not free
    assert image[td - 4] == 5
    extended = image[td + 1] != 0
    r0, c0, nr, nc = struct.unpack_from("<iiii", image, td + 8)
    for k in range(nr * nc):
        p = struct.unpack_from("<q", image, td + 24 + 8 * k)[0] if extended else struct.unpack_from("<I", image, td + 24 + 4 * k)[0] * 8
        if p:
            assert image[p - 4] == 2 and struct.unpack_from("<i", image, p)[0] == (r0 + k // nc) * n_tile_cols + c0 + k % nc


BIG_GRID = (40, 40, 2, 2)                 # 20 x 20 tiles: room for the long lists
BIG_TILE_COLS = 20


def long_list(n_nodes, reverse=False):
    """A file of small records and the update that frees every other one, so that n_nodes nodes of 24 bytes stand in front of the
    one node of 64 bytes that the record written last fits: the first-fit search passes n_nodes nodes, and every free inserts a
    node (behind all others, or with reverse in front of them: the longest shift) -> (image, records, tiles)"""
    layout = []
    for k in range(n_nodes):
        layout += [("t", 2 * k, 24), ("t", 2 * k + 1, 24)]
    layout += [("t", 2 * n_nodes, 64), ("t", 2 * n_nodes + 1, 24)]
    frees = [(2 * k, 0) for k in range(n_nodes)]
    writes = (frees[::-1] if reverse else frees) + [(2 * n_nodes, 0), (399, 64)]
    records, tiles = writes_of(writes)
    return make_file(layout, grid=BIG_GRID), records, tiles
