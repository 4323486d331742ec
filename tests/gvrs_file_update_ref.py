"""Test-only model of a GVRS 1.04 file updated in place: a plain sequential restatement, on a bytearray, of what the reference
does between GvrsFile(file, "rw") and close().  Written from the reference's lines (core/src/main/java/org/gridfour/gvrs/) and
sharing no code with the library; it writes into the file as the reference does, step by step, where the library plans first.
  GvrsFile.java:443-483           open for writing: the free-space, metadata and tile directory records are freed, in that order
  RecordManager.java:161-204      fileSpaceInitRecord, fileSpaceFinishRecord
  RecordManager.java:218-312      fileSpaceAlloc: first fit, exact or at least 32 larger; split; the file's end
  RecordManager.java:314-384      fileSpaceDealloc: merge with the prior (then the next), else the next, else insert
  RecordManager.java:386-490      writeTile's placement
  TileDirectory.java:121-191      setFilePosition: the rectangle only grows
  GvrsFile.java:584-616           close; RecordManager.java:864-883, 905-989, 991-1017 the three directories
One deliberate deviation, the library's: in a file with compression every record is freed first and then allocated, also where
the reference would write the standard form into the block it has just freed (RecordManager.java:476-480)."""
import struct

FREE, TILE, FREE_DIR, META_DIR, TILE_DIR = 0, 2, 3, 4, 5
MIN_FREE_BLOCK_SIZE = 32
MAX_NON_EXTENDED_FILE_POS = 1 << 35
DECLINED = 1

_TABLE = []
for _i in range(256):
    _c = _i
    for _ in range(8):
        _c = (_c >> 1) ^ (0x82F63B78 if _c & 1 else 0)
    _TABLE.append(_c)


def crc32c(data):
    c = 0xffffffff
    for x in bytes(data):
        c = _TABLE[(c ^ x) & 0xff] ^ (c >> 8)
    return c ^ 0xffffffff


def multiple_of_8(v):
    return (v + 7) & ~7


class RefUpdate:
    """A file opened for writing.  n_cols_of_tiles and compression (the specification has codecs) are the caller's knowledge.
    .log: an event per dealloc and alloc, each ending with the node index k it found and the list's length n BEFORE the event:
    ("free", "insert" | "prior" | "next" | "both", pos, size, k, n), ("alloc", "split" | "exact", pos, size, surplus, k, n) and
    ("alloc", "overwrite-last" | "append", pos, size, n), where the search passed all n nodes."""

    def __init__(self, image, n_cols_of_tiles, compression):
        b = self.b = bytearray(image)
        self.n_cols_of_tiles, self.compression = n_cols_of_tiles, compression
        self.content_pos = 16 + struct.unpack_from("<i", b, 16)[0]
        self.checksums = b[104 + 24] != 0
        fs, md = struct.unpack_from("<qq", b, 56)
        (td,) = struct.unpack_from("<q", b, 80)
        struct.pack_into("<q", b, 48, 1)                       # opened for writing: never seen in a finished image
        self.free = []                                         # [position, size], in list order
        self.log = []                                          # which case each alloc / dealloc took, for tests to ask
        self.metadata = None
        if fs > 0:
            (n,) = struct.unpack_from("<i", b, fs)
            for k in range(n):
                p, z = struct.unpack_from("<qi", b, fs + 4 + 12 * k)
                self.free.append([p, z])
            struct.pack_into("<q", b, 56, 0)
            self.dealloc(fs)
        if md > 0:
            (n,) = struct.unpack_from("<i", b, md)
            at = md + 4
            for _ in range(n):
                (ln,) = struct.unpack_from("<H", b, at + 8)
                at += 8 + 2 + ln + 4 + 1
            self.metadata = bytes(b[md:at])                    # sizeMetadata bytes: no reference changes here
            struct.pack_into("<q", b, 64, 0)
            self.dealloc(md)
        self.extended = b[td + 1] != 0
        self.row0, self.col0, self.n_rows, self.n_cols = struct.unpack_from("<iiii", b, td + 8)
        self.offsets = {}
        w = 8 if self.extended else 4
        for i in range(self.n_rows if self.n_cols else 0):
            for j in range(self.n_cols):
                (raw,) = struct.unpack_from("<q" if self.extended else "<I", b, td + 24 + (i * self.n_cols + j) * w)
                self.offsets[(self.row0 + i, self.col0 + j)] = raw if self.extended else raw * 8
        struct.pack_into("<q", b, 80, 0)
        self.dealloc(td)

    # ---- RecordManager ----
    def init_record(self, pos, size, rtype):
        if len(self.b) < pos + size:
            self.b += b"\0" * (pos + size - len(self.b))
        self.b[pos:pos + size] = struct.pack("<i", size) + bytes([rtype, 0, 0, 0]) + b"\0" * (size - 8)

    def finish_record(self, content_pos, content_size):
        pos = content_pos - 8
        (size,) = struct.unpack_from("<i", self.b, pos)
        n_pad = size - (content_size + 8)
        assert n_pad >= 0
        self.b[pos + 8 + content_size:pos + size] = b"\0" * n_pad
        if self.checksums:
            struct.pack_into("<I", self.b, pos + size - 4, crc32c(self.b[pos:pos + size - 4]))

    def alloc(self, size_of_content, rtype):
        size_to_store = multiple_of_8(size_of_content + 12)
        min_size_for_split = size_to_store + MIN_FREE_BLOCK_SIZE
        k = 0
        while k < len(self.free):
            if self.free[k][1] == size_to_store or self.free[k][1] >= min_size_for_split:
                break
            k += 1
        if k == len(self.free):
            file_size = len(self.b)
            if self.free and self.free[-1][0] + self.free[-1][1] == file_size and self.free[-1][1] < size_to_store:
                pos = self.free.pop()[0]
                self.log.append(("alloc", "overwrite-last", pos, size_to_store, k))
                self.init_record(pos, size_to_store, rtype)
                return pos + 8
            self.log.append(("alloc", "append", file_size, size_to_store, k))
            self.init_record(file_size, size_to_store, rtype)
            return file_size + 8
        n_before = len(self.free)
        pos, _ = self.free.pop(k)
        (found,) = struct.unpack_from("<i", self.b, pos)
        surplus = found - size_to_store
        self.log.append(("alloc", "split" if surplus > 0 else "exact", pos, size_to_store, surplus, k, n_before))
        if surplus > 0:
            surplus_pos = pos + size_to_store
            self.init_record(surplus_pos, surplus, FREE)
            j = 0
            while j < len(self.free) and self.free[j][0] <= surplus_pos:
                j += 1
            self.free.insert(j, [surplus_pos, surplus])
        self.init_record(pos, size_to_store, rtype)
        return pos + 8

    def dealloc(self, content_pos):
        release_pos = content_pos - 8
        (release_size,) = struct.unpack_from("<i", self.b, release_pos)
        self.b[release_pos + 4:release_pos + 8] = bytes([FREE, 0, 0, 0])
        k = 0
        while k < len(self.free) and self.free[k][0] <= release_pos:
            k += 1
        n_before = len(self.free)
        prior = self.free[k - 1] if k > 0 else None
        nxt = self.free[k] if k < len(self.free) else None
        if prior is not None and prior[0] + prior[1] == release_pos:
            prior[1] += release_size
            if nxt is not None and prior[0] + prior[1] == nxt[0]:
                prior[1] += nxt[1]
                del self.free[k]
                self.log.append(("free", "both", release_pos, release_size, k, n_before))
            else:
                self.log.append(("free", "prior", release_pos, release_size, k, n_before))
            struct.pack_into("<ii", self.b, prior[0], prior[1], FREE)
            return
        if nxt is not None and release_pos + release_size == nxt[0]:
            nxt[0] = release_pos
            nxt[1] += release_size
            struct.pack_into("<ii", self.b, nxt[0], nxt[1], FREE)
            self.log.append(("free", "next", release_pos, release_size, k, n_before))
            return
        self.free.insert(k, [release_pos, release_size])
        self.log.append(("free", "insert", release_pos, release_size, k, n_before))

    # ---- TileDirectory ----
    def get_position(self, tile):
        return self.offsets.get(divmod(tile, self.n_cols_of_tiles), 0)

    def set_position(self, tile, pos):
        row, col = divmod(tile, self.n_cols_of_tiles)
        if self.n_cols == 0:
            self.row0, self.col0, self.n_rows, self.n_cols = row, col, 1, 1
        else:
            r1, c1 = self.row0 + self.n_rows - 1, self.col0 + self.n_cols - 1
            self.row0, self.col0 = min(self.row0, row), min(self.col0, col)
            self.n_rows, self.n_cols = max(r1, row) - self.row0 + 1, max(c1, col) - self.col0 + 1
        self.offsets[(row, col)] = pos

    # ---- writeTile's placement: record = the framed record as the library takes it, b"" for a tile without valid data ----
    def write_tile(self, tile, record):
        initial = self.get_position(tile)
        if not record:
            if initial > 0:
                self.dealloc(initial)
                self.set_position(tile, 0)
            return
        assert len(record) % 8 == 0 and len(record) >= 24
        content = record[8:len(record) - 4]
        if self.compression or initial == 0:
            if initial > 0:
                self.dealloc(initial)
                self.set_position(tile, 0)
            pos = self.alloc(len(content), TILE)
            if pos > MAX_NON_EXTENDED_FILE_POS:
                self.extended = True
            self.set_position(tile, pos)
        else:
            pos = initial                                        # rewritten where it lies
        self.b[pos:pos + len(content)] = content
        self.finish_record(pos, len(content))

    def update(self, records, tiles, status=None):
        """records in the caller's order; a negative status leaves the tile as it is"""
        for k, (rec, t) in enumerate(zip(records, tiles)):
            st = (0 if rec else DECLINED) if status is None else status[k]
            if st >= 0:
                self.write_tile(t, rec)

    # ---- close ----
    def close(self, time_modified, force_extended=False):
        b = self.b
        self.extended = self.extended or force_extended
        struct.pack_into("<qq", b, 40, time_modified, 0)
        md = 0
        if self.metadata is not None:
            md = self.alloc(len(self.metadata), META_DIR)
            b[md:md + len(self.metadata)] = self.metadata
            self.finish_record(md, len(self.metadata))
        struct.pack_into("<q", b, 64, md)
        n_cells = self.n_rows * self.n_cols
        size = 16 + (8 if self.extended else 4) * n_cells + 8
        td = self.alloc(size, TILE_DIR)
        body = bytes([0, 1 if self.extended else 0]) + b"\0" * 6 + struct.pack("<iiii", self.row0, self.col0, self.n_rows, self.n_cols)
        for i in range(self.n_rows if self.n_cols else 0):
            for j in range(self.n_cols):
                p = self.offsets.get((self.row0 + i, self.col0 + j), 0)
                body += struct.pack("<q", p) if self.extended else struct.pack("<I", (p // 8) & 0xffffffff)
        assert len(body) == size
        b[td:td + size] = body
        self.finish_record(td, size)
        struct.pack_into("<q", b, 80, td)
        struct.pack_into("<q", b, 56, self.write_free_space_directory())
        if self.checksums:
            struct.pack_into("<I", b, self.content_pos - 4, crc32c(b[16:self.content_pos - 4]))
        return bytes(b)

    def write_free_space_directory(self):
        b = self.b
        n = len(self.free)
        if n == 0:
            return 0
        pos = self.alloc(4 + 12 * n, FREE_DIR)
        n = len(self.free)                                       # counted again: the allocation may have consumed a node
        body = struct.pack("<i", n) + b"".join(struct.pack("<qi", p, z) for p, z in self.free)
        b[pos:pos + len(body)] = body
        self.finish_record(pos, len(body))
        for p, z in self.free:
            if self.checksums:
                crc = crc32c(b[p:p + 8])
                b[p + 8:p + z] = b"\0" * (z - 12) + struct.pack("<I", crc)
            else:
                b[p + 8:p + z] = b"\0" * (z - 8)
        return pos


def ref_update(image, n_cols_of_tiles, compression, records, tiles, time_modified, status=None, force_extended=False):
    """-> (the finished image, the free list after opening, the final free list, the log of the tile writes, the log of close)"""
    m = RefUpdate(image, n_cols_of_tiles, compression)
    opened = [tuple(x) for x in m.free]
    del m.log[:]
    m.update(records, tiles, status)
    writes = list(m.log)
    del m.log[:]
    out = m.close(time_modified, force_extended)
    return out, opened, [tuple(x) for x in m.free], writes, list(m.log)
