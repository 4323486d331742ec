// gvrs_api_interp.hip -- B-spline interpolation over a grid block: what GvrsInterpolatorBSpline.zInterpGrid / zNormalGrid and
// InterpolatorBSpline.interpolate deliver for a batch of grid coordinates, from a block that already lies in device memory
// (gf_block_interp_points_dev, gf_block_interp_lattice_dev) or in host memory (gf_block_interp_points, staged through the context).
// The device forms check their arguments, fill in the kernels' arguments and launch (gf_launch_interp, gvrs_interp.hip: k_interp_lattice
// for a lattice with one column spacing, k_interp_points for everything else): they allocate nothing and never synchronise.
// Reference: gvrs/GvrsInterpolatorBSpline.java:107-146, :283-334, :374-484; interpolation/InterpolatorBSpline.java:159-379.

#include "gvrs_api_internal.h"

// what the host can check of a spec; fills g (the render calls of gvrs_api_render.hip check theirs with it too)
gf_status interpSpecArgs(const gf_context *c, const gf_interp_spec *spec, const void *block, bool perPointSpacing, GfInterpGeom &g)
{
    if (!c || !spec || !block) return GF_ERR_ARG;
    if (spec->n_rows_grid < 4 || spec->n_cols_grid < 4) return GF_ERR_ARG;                         // (GvrsInterpolatorBSpline.java:113-116)
    const gf_rect &b = spec->block;
    if (b.row0 < 0 || b.col0 < 0 || b.n_rows < 4 || b.n_cols < 4) return GF_ERR_ARG;
    if ((int64_t)b.row0 + b.n_rows > spec->n_rows_grid || (int64_t)b.col0 + b.n_cols > spec->n_cols_grid) return GF_ERR_ARG;
    if (spec->elem_type < GF_ELEM_INT || spec->elem_type > GF_ELEM_ICF) return GF_ERR_ARG;
    if (spec->wrap < 0 || spec->wrap > 2 || spec->target < GF_INTERP_VALUE || spec->target > GF_INTERP_SECOND) return GF_ERR_ARG;
    if (spec->elem_type == GF_ELEM_SHORT && (spec->fill_i < -32768 || spec->fill_i > 32767)) return GF_ERR_ARG;
    if (spec->target >= GF_INTERP_FIRST && (spec->row_spacing == 0 || (spec->col_spacing == 0 && !perPointSpacing))) return GF_ERR_ARG;
    g.nRowsGrid = spec->n_rows_grid, g.nColsGrid = spec->n_cols_grid;
    g.bRow0 = b.row0, g.bCol0 = b.col0, g.bRows = b.n_rows, g.bCols = b.n_cols;
    g.elemType = spec->elem_type, g.fillI = spec->fill_i, g.wrap = spec->wrap, g.target = spec->target;
    g.rowSpacing = spec->row_spacing, g.colSpacing = spec->col_spacing;
    g.rowFringe0 = spec->row_fringe0, g.rowFringe1 = spec->row_fringe1, g.colFringe0 = spec->col_fringe0, g.colFringe1 = spec->col_fringe1;
    return GF_OK;
}

namespace {

// ... and of the outputs
gf_status interpArgs(const gf_context *c, const gf_interp_spec *spec, const void *block, bool perPointSpacing, const gf_interp_out *out, GfInterpGeom &g)
{
    if (!c || !spec || !block || !out || !out->z) return GF_ERR_ARG;
    const gf_status s = interpSpecArgs(c, spec, block, perPointSpacing, g);
    if (s != GF_OK) return s;
    if (spec->target == GF_INTERP_VALUE && out->normal) return GF_ERR_ARG;
    return GF_OK;
}

void setOut(GfInterpArgs &a, const gf_interp_out *out)
{
    a.z = out->z, a.zx = out->zx, a.zy = out->zy, a.zxx = out->zxx, a.zxy = out->zxy, a.zyy = out->zyy;
    a.normal = out->normal, a.status = out->status;
}

}  // namespace

extern "C" {

gf_status gf_block_interp_points_dev(gf_context *c, void *stream, const gf_interp_spec *spec, const void *dBlock, size_t nPoints,
                                     const double *dRows, const double *dCols, const double *dColSpacing, const gf_interp_out *out)
{
    GfInterpArgs a{};
    const gf_status s = interpArgs(c, spec, dBlock, dColSpacing != nullptr, out, a.g);
    if (s != GF_OK) return s;
    if (nPoints && (!dRows || !dCols)) return GF_ERR_ARG;
    if (nPoints == 0) return GF_OK;
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    a.block = dBlock;
    a.nPoints = nPoints;
    a.rows = dRows, a.cols = dCols, a.colSpacing = dColSpacing;
    setOut(a, out);
    GF_HIP(gf_launch_interp(a, streamOf(c, stream)));
    return GF_OK;
}

gf_status gf_block_interp_lattice_dev(gf_context *c, void *stream, const gf_interp_spec *spec, const void *dBlock, const gf_interp_lattice *lat,
                                      const double *dColSpacingRows, const gf_interp_out *out)
{
    GfInterpArgs a{};
    const gf_status s = interpArgs(c, spec, dBlock, dColSpacingRows != nullptr, out, a.g);
    if (s != GF_OK) return s;
    if (!lat || lat->n_rows < 1 || lat->n_cols < 1) return GF_ERR_ARG;
    if ((uint64_t)lat->n_rows > (((uint64_t)1 << 63) - 1) / (uint64_t)lat->n_cols) return GF_ERR_UNSUPPORTED;   // 2^63 or more points
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    a.block = dBlock;
    a.nPoints = (size_t)lat->n_rows * (size_t)lat->n_cols;
    a.colSpacing = dColSpacingRows;
    a.latRow0 = lat->row0, a.latCol0 = lat->col0, a.latRowStep = lat->row_step, a.latColStep = lat->col_step;
    a.latRows = (uint64_t)lat->n_rows, a.latCols = (uint64_t)lat->n_cols;
    setOut(a, out);
    GF_HIP(gf_launch_interp(a, streamOf(c, stream)));
    return GF_OK;
}

gf_status gf_block_interp_points(gf_context *c, const gf_interp_spec *spec, const void *block, size_t nPoints, const double *rows,
                                 const double *cols, const double *colSpacing, const gf_interp_out *out)
{
    GfInterpArgs a{};
    gf_status s = interpArgs(c, spec, block, colSpacing != nullptr, out, a.g);
    if (s != GF_OK) return s;
    if (nPoints && (!rows || !cols)) return GF_ERR_ARG;
    if (nPoints > ((size_t)1 << 56)) return GF_ERR_UNSUPPORTED;                                    // (the staging sizes below stay in 64 bits)
    if (nPoints == 0) return GF_OK;
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    // staging: block | rows | cols | spacings | z zx zy zxx zxy zyy | normal | status, the parts that the call has
    HostStage sg(c);
    const int blockP = sg.in(block, (size_t)a.g.bRows * (size_t)a.g.bCols * (a.g.elemType == GF_ELEM_SHORT ? 2 : 4));
    const int rowsP = sg.in(rows, nPoints * 8), colsP = sg.in(cols, nPoints * 8), csP = sg.in(colSpacing, nPoints * 8);
    double *const host[6] = {out->z, out->zx, out->zy, out->zxx, out->zxy, out->zyy};
    int devP[6];
    for (int k = 0; k < 6; k++) devP[k] = sg.out(host[k], nPoints * 8);
    const int normalP = sg.out(out->normal, nPoints * 24), statusP = sg.out(out->status, nPoints * 4);
    if ((s = sg.begin()) != GF_OK) return s;
    a.block = sg.ptr<void>(blockP);
    a.nPoints = nPoints;
    a.rows = sg.ptr<double>(rowsP), a.cols = sg.ptr<double>(colsP), a.colSpacing = sg.ptr<double>(csP);
    a.z = sg.ptr<double>(devP[0]), a.zx = sg.ptr<double>(devP[1]), a.zy = sg.ptr<double>(devP[2]);
    a.zxx = sg.ptr<double>(devP[3]), a.zxy = sg.ptr<double>(devP[4]), a.zyy = sg.ptr<double>(devP[5]);
    a.normal = sg.ptr<double>(normalP), a.status = sg.ptr<int32_t>(statusP);
    GF_HIP(gf_launch_interp(a, c->stream));
    return sg.end();
}

}  // extern "C"
