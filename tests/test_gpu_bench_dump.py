"""bench.py --dump-outputs: what the last timed step computed, written as .npy files in float32 / float64 under 64 MB, the
same from run to run whatever the step count, and equal to what the oracle makes of the same seeded tiles."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, steps, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--cpu-sample-tiles", "0", "--dump-outputs", str(out_dir)] + list(extra)
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["ms_per_step"] > 0
    files = sorted(os.listdir(out_dir))
    arrays = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in files}
    assert all(f.endswith(".npy") for f in files)
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(os.path.getsize(os.path.join(out_dir, f)) for f in files) <= 64 * 10 ** 6
    return d, arrays


def test_dump_huffman_is_reproducible_and_matches_the_oracle(tmp_path):
    n_rows, n_cols, n_tiles, tiles_per_row = 200, 200, 1024, 32          # bench.py's dem1024
    d, a = _bench(tmp_path / "a", 2, "--workload", "dem1024")
    assert d["bit_exact"] is True
    assert set(a) == {"tiles", "lengths", "predictors", "enc_status", "dec_status", "packings", "decoded"}
    assert a["lengths"].shape == a["predictors"].shape == a["enc_status"].shape == (n_tiles,)
    assert (a["enc_status"] == 0).all() and (a["dec_status"] == 0).all()
    tiles = a["tiles"].astype(np.int64)
    assert 0 < len(tiles) <= n_tiles and (np.diff(tiles) > 0).all()
    assert a["decoded"].shape == (len(tiles), n_rows, n_cols)
    lens = a["lengths"][tiles].astype(np.int64)
    assert a["packings"].shape == (int(lens.sum()),)
    # the same seeded inputs: the generator of bench.py's dem1024 batch, on the host
    vals = {int(t): oracle.dem_tiles(oracle.DEM_SEED + 1, n_rows, n_cols, tiles_per_row, int(t), 1)[0] for t in tiles}
    assert np.array_equal(a["decoded"].reshape(len(tiles), -1), np.stack([vals[int(t)] for t in tiles]).astype(np.float64))
    starts = np.concatenate([[0], np.cumsum(lens)])
    for i in (0, len(tiles) // 2, len(tiles) - 1):
        t = int(tiles[i])
        ref, used = oracle.codec_huffman_encode(0, n_rows, n_cols, vals[t])
        assert bytes(a["packings"][starts[i]:starts[i + 1]].astype(np.uint8)) == ref and a["predictors"][t] == used
    # another run with another step count writes the same arrays
    _, b = _bench(tmp_path / "b", 3, "--workload", "dem1024")
    assert set(b) == set(a) and all(np.array_equal(a[k], b[k]) for k in a)


def test_dump_float_planes(tmp_path):
    n_rows, n_cols = 256, 256
    d, a = _bench(tmp_path / "f", 1, "--workload", "float256", "--codec", "float")
    assert d["bit_exact"] is True and d["steps"] == 1
    assert set(a) == {"tiles", "planes", "decoded"}
    tiles = a["tiles"].astype(np.int64)
    assert 0 < len(tiles) < 4096 and a["decoded"].dtype == np.float32
    assert a["decoded"].shape == (len(tiles), n_rows, n_cols) and a["planes"].shape[0] == len(tiles)
    # the floats of bench.py's float256 batch: the synthetic DEM of seed DEM_SEED + 5, 64 tiles per row, times 0.1f
    vals = np.concatenate([oracle.dem_tiles(oracle.DEM_SEED + 5, n_rows, n_cols, 64, int(t), 1) for t in tiles])
    f = (vals.astype(np.float32) * np.float32(0.1)).reshape(len(tiles), n_rows, n_cols)
    assert np.array_equal(a["decoded"].view(np.uint32), f.view(np.uint32))
    for i in (0, len(tiles) - 1):
        want = np.frombuffer(bytes(oracle.float_planes_encode(n_rows, n_cols, f[i].ravel().view(np.uint32))), np.uint8)
        assert np.array_equal(a["planes"][i].astype(np.uint8), want), int(tiles[i])
