"""Shared by the image tests: the stand-alone harness of gridfour_amd/csrc/gvrs_image_common.h (built and run as a program of its
own), and the inputs of the CPU and GPU tests -- words, plane values at the edges, images whose windows sit on the rounding
boundary of the reduce."""
import os
import struct
import subprocess

import numpy as np

import image_ref as M

HERE = os.path.dirname(os.path.abspath(__file__))

# gvrs_image.hip: IMG_MAX_GROUPS workgroups of IMG_THREADS lanes, four pixels a lane; past it the stride loop takes a second trip
SPLIT_ONE_TRIP = 2048 * 256 * 4
COUNTS = (0, 1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, SPLIT_ONE_TRIP + 7)
EDGE_INTS = (M.INT_MIN, M.INT_MAX, -1, 256, 0, 255, -256, 0x7fff, -0x8000, 0x10000, M.INT_MIN + 1)
REDUCE_FACTORS = (1, 2, 3, 4, 7, 8, 9, 16, 60)


def build_harness(flags=("-O2",), name="image_harness"):
    src, exe = os.path.join(HERE, "csrc", "image_harness.cpp"), os.path.join(HERE, "csrc", name)
    subprocess.check_call(["g++", *flags, "-std=c++17", "-o", exe, src])
    return exe


def _run(exe, mode, payload, tmp):
    src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(src, "wb") as f:
        f.write(payload)
    subprocess.run([exe, mode, src, dst], check=True)
    return open(dst, "rb").read()


def harness_split(exe, tmp, model, argb):
    w = M.words(argb).reshape(-1)
    out = np.frombuffer(_run(exe, "split", struct.pack("<iq", model, w.size) + w.tobytes(), tmp), np.int32)
    return list(out.reshape(3, w.size))


def harness_join(exe, tmp, model, planes):
    p = np.stack([np.asarray(x).astype(np.int32).reshape(-1) for x in planes])
    return np.frombuffer(_run(exe, "join", struct.pack("<iq", model, p.shape[1]) + p.tobytes(), tmp), np.int32)


def harness_reduce(exe, tmp, argb, f):
    w = M.words(argb)
    out = np.frombuffer(_run(exe, "reduce", struct.pack("<iqq", f, w.shape[1], w.shape[0]) + np.ascontiguousarray(w).tobytes(), tmp), np.int32)
    return out.reshape(w.shape[0] // f, w.shape[1] // f)


def random_words(rng, n):
    """words with random alpha"""
    return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def join_planes(rng, n, fill, elem_type=M.INT):
    """three planes of n items for a join: plane values of real pictures, any ints, and the fill and the edge values in every
    plane, alone and together"""
    if elem_type == M.SHORT:
        planes = [rng.integers(-32768, 32768, n).astype(np.int16) for _ in range(3)]
        edges = [v for v in EDGE_INTS + (fill,) if -32768 <= v <= 32767]
    else:
        planes = [rng.integers(M.INT_MIN, M.INT_MAX + 1, n).astype(np.int32) for _ in range(3)]
        edges = list(EDGE_INTS + (fill,))
    real = M.split(M.YCOCG, random_words(rng, n))
    for k in range(3):
        planes[k][::3] = real[k][::3]
    at = 0
    for v in edges:                                     # (short arrays take what fits of the list)
        for k in range(4):
            if at < n:
                for p in range(3):
                    if k == p or k == 3:
                        planes[p][at] = v
                at += 1
    return planes


def boundary_image(f, n_rows, n_cols, rng):
    """n_rows x n_cols windows of f x f pixels whose channel sums mod n sit at n / 2 - 1, n / 2, n / 2 + 1 (and elsewhere), with
    random alpha, plus a partial row and column that no window covers"""
    n = f * f
    h, w = n_rows * f + (f > 1) * (f // 2), n_cols * f + (f > 1) * (f - 1)
    img = np.zeros((h, w), np.uint32)
    img[:, :] = random_words(rng, h * w).reshape(h, w)
    for i in range(n_rows):
        for j in range(n_cols):
            win = np.zeros((3, n), np.int64)
            for c in range(3):
                q = int(rng.integers(0, 255))
                target = q * n + (n // 2 - 1 + (i + j + c) % 3) % n if (i + j) % 4 else int(rng.integers(0, 255 * n + 1))
                target = min(max(target, 0), 255 * n)
                base, extra = divmod(target, n)
                win[c, :] = base
                win[c, :extra] += 1
                rng.shuffle(win[c])
            px = (win[0] << 16 | win[1] << 8 | win[2]).astype(np.uint32).reshape(f, f)
            alpha = img[i * f:(i + 1) * f, j * f:(j + 1) * f] & np.uint32(0xff000000)
            img[i * f:(i + 1) * f, j * f:(j + 1) * f] = px | alpha
    return img
