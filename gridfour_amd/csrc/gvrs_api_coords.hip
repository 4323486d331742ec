// gvrs_api_coords.hip -- a GVRS file's coordinate rules at the C ABI: gf_file_interp_spec (the gf_interp_spec the reference's
// interpolator would work with: wrap, fringes, du and dv derived from the file) and gf_file_map_points[_dev] (the mappings between
// geographic / model and grid coordinates over a batch, with the GridPoint's integers and zNormal's column spacing).  The host
// forms are arithmetic (gvrs_coords.h; no device, no context); the device form checks its arguments and launches k_coords_map
// (gvrs_coords.hip): it allocates nothing and never synchronises.  The fused interpolation at coordinates is in
// gvrs_api_file_points.hip, beside the forms it extends.
// Reference: gvrs/GvrsFileSpecification.java:435-440, :695-707, :2101-2234; gvrs/GvrsInterpolatorBSpline.java:120-131, :226-232.

#include "gvrs_api_internal.h"

GfCoords coordsOf(const gf_file_info &i)
{
    GfCoords c{};
    c.nRowsGrid = i.grid.n_rows_grid, c.nColsGrid = i.grid.n_cols_grid;
    c.geographic = i.coordinate_system == 2;
    c.x0 = i.x0, c.y0 = i.y0, c.x1 = i.x1, c.y1 = i.y1, c.cellSizeX = i.cell_size_x, c.cellSizeY = i.cell_size_y;
    for (int k = 0; k < 6; k++) c.m2r[k] = i.m2r[k], c.r2m[k] = i.r2m[k];
    gf_coords_derive(c);
    return c;
}

gf_status noContext() { return gf_device_count() > 0 ? GF_ERR_ARG : GF_ERR_NO_DEVICE; }

namespace {

// what both forms of the mapping check, and the file's rules
gf_status mapArgs(const gf_file *f, int kind, size_t n, const double *a, const double *b, const double *outA, const double *outB, const int32_t *iRow,
                  const int32_t *iCol, const double *colSpacing, const int32_t *status, GfCoords &c)
{
    if (!f || kind < GF_MAP_GEO_TO_GRID || kind > GF_MAP_GRID_TO_MODEL) return GF_ERR_ARG;
    if (n && (!a || !b || !outA || !outB)) return GF_ERR_ARG;
    if (kind >= GF_MAP_GRID_TO_GEO && (iRow || iCol || colSpacing || status)) return GF_ERR_ARG;
    gf_file_info i;
    const gf_status s = gf_file_get_info(f, &i);
    if (s != GF_OK) return s;
    c = coordsOf(i);
    return GF_OK;
}

}  // namespace

extern "C" {

gf_status gf_file_interp_spec(const gf_file *f, int elem, int target, gf_interp_spec *spec)
{
    if (!f || !spec || elem < 0 || target < GF_INTERP_VALUE || target > GF_INTERP_SECOND) return GF_ERR_ARG;
    gf_file_info i;
    const gf_status s = gf_file_get_info(f, &i);
    if (s != GF_OK) return s;
    if (elem >= i.n_elems || i.grid.n_rows_grid < 4 || i.grid.n_cols_grid < 4) return GF_ERR_ARG;   // (GvrsInterpolatorBSpline.java:113-116)
    const GfCoords c = coordsOf(i);
    *spec = gf_interp_spec{};
    spec->n_rows_grid = i.grid.n_rows_grid, spec->n_cols_grid = i.grid.n_cols_grid;
    spec->block = gf_rect{0, 0, i.grid.n_rows_grid, i.grid.n_cols_grid};
    spec->elem_type = i.elems[elem].type, spec->fill_i = i.elems[elem].fill_i;
    spec->wrap = c.wrap, spec->target = target;
    spec->row_spacing = c.dv, spec->col_spacing = c.du;
    spec->row_fringe0 = c.rowFringe0, spec->row_fringe1 = c.rowFringe1, spec->col_fringe0 = c.colFringe0, spec->col_fringe1 = c.colFringe1;
    return GF_OK;
}

gf_status gf_file_map_points(const gf_file *f, int kind, size_t n, const double *a, const double *b, double *outA, double *outB, int32_t *iRow,
                             int32_t *iCol, double *colSpacing, int32_t *status)
{
    GfCoords c;
    const gf_status s = mapArgs(f, kind, n, a, b, outA, outB, iRow, iCol, colSpacing, status, c);
    if (s != GF_OK) return s;
    for (size_t t = 0; t < n; t++) {
        GfCoordsMapped m;
        gf_coords_map(c, kind, a[t], b[t], m);
        outA[t] = m.outA, outB[t] = m.outB;
        if (kind >= GF_MAP_GRID_TO_GEO) continue;
        if (iRow) iRow[t] = m.iRow;
        if (iCol) iCol[t] = m.iCol;
        if (colSpacing) colSpacing[t] = m.spacing;
        if (status) status[t] = m.status;
    }
    return GF_OK;
}

gf_status gf_file_map_points_dev(gf_context *ctx, const gf_file *f, int kind, size_t n, const double *dA, const double *dB, double *dOutA,
                                 double *dOutB, int32_t *dIRow, int32_t *dICol, double *dColSpacing, int32_t *dStatus)
{
    GfCoordsMapArgs a{};
    const gf_status s = mapArgs(f, kind, n, dA, dB, dOutA, dOutB, dIRow, dICol, dColSpacing, dStatus, a.c);
    if (s != GF_OK) return s;
    if (!ctx) return noContext();
    if (n == 0) return GF_OK;
    GF_CTX_LOCK(ctx);
    GF_HIP(hipSetDevice(ctx->device));
    a.kind = kind, a.nPoints = n, a.a = dA, a.b = dB, a.outA = dOutA, a.outB = dOutB;
    a.iRow = dIRow, a.iCol = dICol, a.colSpacing = dColSpacing, a.status = dStatus;
    GF_HIP(gf_launch_coords_map(a, ctx->stream));
    return GF_OK;
}

}  // extern "C"
