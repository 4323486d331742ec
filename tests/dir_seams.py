"""Test-only: the directory sizes at the seams of the tile directory checksum's chunks, shared by the tests of the write
(tests/test_gpu_file_write.py), of the update (tests/test_gpu_file_update.py) and of the host assemblers."""

# name -> the number of directory entries, from the chunk size c and an entry's width w (4 compact, 8 extended)
SEAMS = [("one", lambda c, w: 1), ("C-1", lambda c, w: c // w - 1), ("C", lambda c, w: c // w), ("C+1", lambda c, w: c // w + 1),
         ("3C+5", lambda c, w: 3 * c // w + 5),
         # more than 64 chunks: the lanes of the fold (one wave) each take a second chunk
         ("65C+1", lambda c, w: 65 * c // w + 1)]


def read_chunk(tmp_path_factory):
    """GF_FILE_CRC_CHUNK, read through the stand-alone program of tests/csrc/file_emit_test.cpp: no copy of it is kept here"""
    from test_file_assemble import build_emit_test, crc_chunk
    exe, err = build_emit_test(tmp_path_factory, False)
    assert exe, err[-2000:]
    return crc_chunk(exe)
