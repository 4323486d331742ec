"""Test-only: GvrsInspector's walk (core/src/main/java/org/gridfour/gvrs/GvrsInspector.java:213-337) restated sequentially in plain
Python, with the deviations include/gvrs_hip_codec.h states where the reference is undefined.  Where a deviation changes the
answer, "reference" holds what the reference itself would have said, so that the deviation is visible and pinned:
  the termination position after a bad type code stays 16 there (IOException before it is set);
  a record that ends behind the file of a file WITHOUT checksums is walked past and the inspection reported complete;
  a size word that is negative, below 16 or no multiple of 8 has no defined answer there ("undefined")."""
import struct

from gvrs_file_build import crc32c

END, BAD_TILE_INDEX, TILE_TOO_LARGE, TWO_CHECKSUM_FAILURES, BAD_RECORD_TYPE, BAD_RECORD_SIZE, TRUNCATED = range(7)


def facts_of(f):
    """What the walk needs of an opened file (a GvrsFileHip): positions, the checksum flag, the tile count, the size limit"""
    g = f.grid
    cells = g[2] * g[3]
    standard = sum((cells * 2 + 3) & ~3 if (e if isinstance(e, str) else e[0]) == "short" else cells * 4 for e in f.elems)
    return dict(content_pos=f.info["content_pos"], tile_dir_pos=f.info["tile_dir_pos"], checksums=bool(f.info["checksum_enabled"]),
                n_tiles=-(-g[0] // g[2]) * -(-g[1] // g[3]), max_tile_record_size=(4 + 4 * f.n_elems + standard + 12 + 7) & ~7)


def _i32(image, at):
    return struct.unpack_from("<i", image, at)[0]


def _u32(image, at):
    return struct.unpack_from("<I", image, at)[0]


def dir_record_passes(image, P, content_pos):
    """testRecordChecksum of the record whose content lies at P (false, not an exception, for a size word that is undefined there)"""
    n = len(image)
    if P < content_pos + 8 or P % 8 or P > n:
        return False
    size, rtype = _i32(image, P - 8), image[P - 4]
    if rtype > 6 or size < 16 or size % 8 or P - 8 + size > n:
        return False
    return crc32c(image[P - 8:P - 8 + size - 4]) == _u32(image, P - 8 + size - 4)


def inspect(image, facts):
    image = bytes(image)
    n, pos = len(image), facts["content_pos"]
    out = dict(failed=0, complete=0, stop=END, bad_tile_index=0, invalid_record_size=0, tile_dir_located=1,
               tile_dir_passed=int(dir_record_passes(image, facts["tile_dir_pos"], facts["content_pos"])), n_by_type=[0] * 7,
               n_checksum_failures=0)
    bad, records, reference = [], [], {}
    previous_passed = True

    def stop_at(code, rec):
        out["stop"], out["failed"] = code, 1
        records.append(rec)
        if 0 <= rec[2] <= 6:
            out["n_by_type"][rec[2]] += 1

    while pos < n - 12:
        size = _i32(image, pos)
        if size == 0:
            break
        rtype, tile = image[pos + 4], -1
        if rtype > 6:
            stop_at(BAD_RECORD_TYPE, (pos, size & 0xffffffff, rtype, -1, -1))
            reference["termination_pos"] = 16
            break
        if size < 16 or size % 8:
            stop_at(BAD_RECORD_SIZE, (pos, size & 0xffffffff, rtype, -1, -1))
            reference["undefined"] = True
            break
        if rtype == 2:
            tile = _i32(image, pos + 8)
            if tile < 0 or tile >= facts["n_tiles"]:
                out["bad_tile_index"] = 1
                stop_at(BAD_TILE_INDEX, (pos, size, rtype, tile, -1))
                break
            if size > facts["max_tile_record_size"]:
                bad.append(tile)
                out["invalid_record_size"] = 1
                stop_at(TILE_TOO_LARGE, (pos, size, rtype, tile, -1))
                break
        if pos + size > n:
            stop_at(TRUNCATED, (pos, size, rtype, tile, -1))
            if not facts["checksums"]:
                reference["complete"], reference["termination_pos"] = 1, pos + size
            break
        checksum = -1
        if facts["checksums"]:
            crc = crc32c(image[pos:pos + 8]) if rtype == 0 else crc32c(image[pos:pos + size - 4])
            checksum = int(crc == _u32(image, pos + size - 4))
            if not checksum:
                out["n_checksum_failures"] += 1
                out["failed"] = 1
                if rtype == 2:
                    bad.append(tile)
                if not previous_passed:
                    stop_at(TWO_CHECKSUM_FAILURES, (pos, size, rtype, tile, 0))
                    break
                previous_passed = False
            else:
                previous_passed = True
                if rtype == 5:
                    out["tile_dir_passed"] = 1
        records.append((pos, size, rtype, tile, checksum))
        out["n_by_type"][rtype] += 1
        pos += size
    if out["stop"] == END:
        out["complete"] = 1
    out.update(status=0, termination_pos=pos, n_records=len(records), n_bad_tiles=len(bad), bad_tiles=bad, records=records, reference=reference)
    return out


REPORT_FIELDS = ("status", "failed", "complete", "stop", "bad_tile_index", "invalid_record_size", "tile_dir_located", "tile_dir_passed",
                 "termination_pos", "n_records", "n_by_type", "n_checksum_failures", "n_bad_tiles")


def same(result, want):
    """A GvrsInspection against the restatement's answer, field for field: the list of what differs"""
    diffs = [(k, getattr(result, k), want[k]) for k in REPORT_FIELDS if getattr(result, k) != want[k]]
    if result.bad_tiles != want["bad_tiles"]:
        diffs.append(("bad_tiles", result.bad_tiles, want["bad_tiles"]))
    if result.records != want["records"]:
        diffs.append(("records", None if result.records is None else [r for r, w in zip(result.records, want["records"]) if r != w][:3], len(want["records"])))
    return diffs
