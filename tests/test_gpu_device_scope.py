"""The binding's device-call scope and its element table (gridfour_amd/codec.py): a scope frees every buffer made through it when
its body raises, an "lsop" DeviceTileBatch frees its work buffers too, and the element helpers return, per kind, the literal
gf_elem_spec fields and dtypes written out below."""
import numpy as np
import pytest

from gridfour_amd import INT4_NULL_CODE, CodecMasterHip, DeviceTileBatch
from gridfour_amd.codec import _DeviceScope
from test_gpu_records_dev import ctx      # noqa: F401  (ctx: fixture)

ICF = ("icf", 0.25, -3.5, -77, -9999.0)
# elems entry -> (type, scale, offset, fill_i, fill_f as _elem_specs leaves them; delivered dtype; dtype _elem_values hands on;
# the gf_elem_spec field and value of the default fill, None: _fill_specs takes no fill for the kind)
EXPECTED = {
    "int": ((0, 1.0, 0.0, 0, 0.0), np.int32, np.int32, ("fill_i", INT4_NULL_CODE)),
    "short": ((1, 1.0, 0.0, 0, 0.0), np.int16, np.int16, ("fill_i", -32768)),
    "float": ((2, 1.0, 0.0, 0, 0.0), np.float32, np.float32, ("fill_f", np.nan)),
    ICF: ((3, 0.25, -3.5, -77, -9999.0), np.float32, np.int32, None),
}
FIELDS = ("type", "scale", "offset", "fill_i", "fill_f")


def _fields(spec):
    return tuple(spec[k].item() for k in FIELDS)


def _same(got, want):
    return len(got) == len(want) and all(g == w or (g != g and w != w) for g, w in zip(got, want))


@pytest.mark.gpu
def test_scope_frees_on_error(ctx):      # noqa: F811
    made = []
    with pytest.raises(ValueError, match="from the body"):
        with _DeviceScope(ctx) as s:
            made.append(s.upload(np.arange(40, dtype=np.int32), slack=16))
            made.append(s.alloc(100, fill=0xA5))
            made.append(s.alloc(7))
            assert [b.nbytes for b in made] == [176, 100, 7] and all(b.ptr for b in made)
            assert np.array_equal(made[0].download(np.int32, 40), np.arange(40)) and (made[1].download(np.uint8, 100) == 0xA5).all()
            raise ValueError("from the body")
    assert len(made) == 3
    for b in made:
        assert not b.ptr
        b.free()
        assert not b.ptr


@pytest.mark.gpu
def test_lsop_batch_frees_everything(ctx):      # noqa: F811
    batch = DeviceTileBatch(ctx, 8, 8, 2, codec="lsop")
    buffers = {k: getattr(batch, k) for k in ("values", "decoded", "slots", "lengths", "predictors", "enc_status", "dec_status", "residuals",
                                              "coefs", "scratch_status")}
    assert all(b.ptr for b in buffers.values())
    batch.free()
    assert [k for k, b in buffers.items() if b.ptr] == []
    batch.free()


@pytest.mark.parametrize("el", list(EXPECTED), ids=lambda el: el if isinstance(el, str) else el[0])
def test_element_table(el):
    fields, delivered, written, fill = EXPECTED[el]
    specs, dtypes = CodecMasterHip._elem_specs([el])
    assert specs.shape == (1,) and _same(_fields(specs[0]), fields) and dtypes == [delivered]

    nr, nc, nt = 3, 5, 2
    values = np.arange(nt * nr * nc).reshape(nt, nr, nc) - 7
    specs, vals = CodecMasterHip._elem_values(nr, nc, [values], [el], None)
    want = list(fields)
    if el == "short":
        want[3] = -32768                     # a writer's "short" element carries its fill; the default
    assert _same(_fields(specs[0]), want)
    assert len(vals) == 1 and vals[0].dtype == written and vals[0].shape == (nt, nr * nc) and np.array_equal(vals[0], values.reshape(nt, -1))
    specs, _ = CodecMasterHip._elem_values(nr, nc, [values], [el], [-5])
    assert specs[0]["fill_i"] == (-5 if el == "short" else fields[3])

    specs = CodecMasterHip._fill_specs(CodecMasterHip._elem_specs([el])[0], [el], None)
    want = list(fields)
    if fill is not None:
        want[FIELDS.index(fill[0])] = fill[1]
    assert _same(_fields(specs[0]), want)
    if fill is None:
        with pytest.raises(AssertionError):
            CodecMasterHip._fill_specs(CodecMasterHip._elem_specs([el])[0], [el], [1.0])
    else:
        specs = CodecMasterHip._fill_specs(CodecMasterHip._elem_specs([el])[0], [el], [-12])
        assert specs[0][fill[0]] == -12 and _same(_fields(CodecMasterHip._fill_specs(CodecMasterHip._elem_specs([el])[0], [el], [None])[0]), want)
