"""CPU-only: gridfour_amd/csrc/gvrs_render_common.h, the restatement of the reference's colour palette lookup and shaded relief that
the kernels inline, compiled with g++ -O2 -ffp-contract=off into a program of its own (tests/csrc/render_harness.cpp) and compared
BIT FOR BIT with the numpy model of tests/render_ref.py: some thousand random z per palette, z at, just below and just above every
key and every range1, the special values, every shade kind, both range behaviours, cells of every element type, and random lattices
over a block with both demos' gain signs.  The same program built with -fsanitize=address,undefined runs the same inputs once."""
import numpy as np
import pytest

import interp_cases as K
import interp_ref as R
import render_cases as RC
import render_ref as M


@pytest.fixture(scope="module")
def rh():
    return RC.build_harness()


def _lookups(exe, tmp, name, n_random, seed):
    pal = RC.model(name)
    rng = np.random.default_rng(seed)
    z = RC.lookup_z(pal, rng, n_random)
    sh = RC.shades_for(rng, z.size)
    for unlimited in (False, True):
        assert np.array_equal(RC.harness_lookup(exe, tmp, pal, z, None, unlimited), pal.argb(z, None, unlimited)), (name, unlimited)
        assert np.array_equal(RC.harness_lookup(exe, tmp, pal, z, sh, unlimited), pal.argb(z, sh, unlimited)), (name, unlimited, "shade")
    return pal, z


@pytest.mark.parametrize("name", sorted(RC.PALETTES))
def test_lookups_equal_the_model(rh, tmp_path, name):
    pal, z = _lookups(rh, str(tmp_path), name, 3000, 10)
    got = pal.argb(z)
    assert (got == pal.argb_for_null).any() and (got != pal.argb_for_null).any()


def _cells(exe, tmp, seed):
    rng = np.random.default_rng(seed)
    pal = RC.model("etopo1")
    for elem_type, fill in ((R.INT, 12345), (R.SHORT, -32768), (R.FLOAT, 0), (R.ICF, 0)):
        cells = K.random_block(rng, elem_type, (1, 2000), fill)
        if elem_type in (R.FLOAT, R.ICF):
            cells = K.float_specials(cells * np.float32(200.0))
        elif elem_type == R.INT:
            cells = (cells >> 17).astype(np.int32)
            cells[5::23] = fill
        sh = RC.shades_for(rng, cells.size)
        want = M.render_cells(pal, cells, elem_type, fill, sh)
        assert (want == pal.argb_for_null).any() and (want != pal.argb_for_null).any()
        assert np.array_equal(RC.harness_lookup(exe, tmp, pal, cells, sh, False, elem_type, fill), want), elem_type


def test_cells_of_every_element_type(rh, tmp_path):
    _cells(rh, str(tmp_path), 20)


def _lattices(exe, tmp, seed, shapes):
    rng = np.random.default_rng(seed)
    pal = M.Palette(RC._ramp(9, -70.0, 70.0, gaps=True), 0xff00ff00)     # the samples of K.random_block lie in -64 .. 64
    seen = set()
    for (grid, rect), wrap, light_name, (n_rows, n_cols) in shapes:
        light = RC.LIGHTS[light_name] if light_name else None
        spec = R.Spec(grid[0], grid[1], rect, R.FLOAT, wrap=wrap, row_spacing=0.37109375 + 2.0 ** -40, col_spacing=1.9 / 3.0)
        block = K.random_block(rng, R.FLOAT, spec.block[2:])
        lattice = (-0.9, -2.6, (grid[0] + 1.5) / n_rows, (grid[1] + 5.0) / n_cols, n_rows, n_cols)
        rows, cols = R.lattice_coords(*lattice)
        cs_rows = rng.uniform(0.25, 3.0, n_rows)
        cs_rows[3] = 0.0
        for cs in (None, cs_rows):
            want = M.render_points(spec, block, rows, cols, pal, light, None if cs is None else np.repeat(cs, n_cols))
            got = RC.harness_lattice(exe, tmp, spec, block, lattice, pal, light, cs)
            assert np.array_equal(got["status"], want["status"]) and np.array_equal(got["argb"], want["argb"]), (grid, wrap, light_name)
            if light is not None:
                assert R.same_bits(got["shade"], want["shade"]) and not np.isnan(want["shade"]).any()
                assert (want["shade"][want["status"] != R.OK] == light.ambient).all()
            assert (want["argb"][want["status"] != R.OK] == pal.argb_for_null).all()
            seen |= set(want["status"].tolist())
    return seen


GRIDS = [((9, 11), None), ((12, 14), (2, 3, 7, 9))]


def test_lattices_equal_the_model(rh, tmp_path):
    shapes = [(GRIDS[0], 0, "extract", (40, 50)), (GRIDS[1], 0, "cog", (40, 50)), (GRIDS[0], 1, "cog", (33, 47)), (GRIDS[0], 2, None, (40, 50)),
              (GRIDS[1], 1, "extract", (21, 60))]
    assert _lattices(rh, str(tmp_path), 30, shapes) >= {R.OK, R.DECLINED, R.ERR_BOUNDS, R.ERR_ARG}


def test_under_the_sanitizers(tmp_path):
    """the same stand-alone program with -fsanitize=address,undefined, run directly on smaller draws of the same inputs: a report
    ends the program with a non-zero status"""
    exe = RC.build_harness(("-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"), "render_harness_san")
    for name in ("etopo1", "hsv", "hinge", "point_records", "gaps_256"):
        _lookups(exe, str(tmp_path), name, 300, 40)
    _cells(exe, str(tmp_path), 50)
    _lattices(exe, str(tmp_path), 60, [(GRIDS[1], 1, "extract", (17, 23)), (GRIDS[0], 2, None, (9, 31))])
