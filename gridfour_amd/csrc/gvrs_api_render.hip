// gvrs_api_render.hip -- a grid block rendered to ARGB words: the colour palette object (gf_palette_create: what the constructor of
// imaging/palette/ColorPaletteTable.java:162-253 does, on the host, and one packed table uploaded) and the entry points that turn
// the cells of a block (gf_block_render_cells_dev) or the B-spline surface over it, lit as the reference's demos light it
// (gf_block_render_lattice_dev, gf_block_render_points_dev; gf_block_render_lattice staged through the context), into one int32
// per pixel.  The device forms check their arguments, fill in the kernels' arguments and launch (gvrs_render.hip): they allocate
// nothing and never synchronise.

#include "gvrs_api_internal.h"

struct gf_palette {
    int device = -1;                    // -1: the table lies on the host alone (gf_internal_palette_create_host)
    void *dTable = nullptr;             // GfPalHead | keys[n] | recs[n]
    std::vector<uint8_t> packed;        // the same bytes
    const GfPalHead &head() const { return *reinterpret_cast<const GfPalHead *>(packed.data()); }
};

namespace {

// Double.compare
int javaDoubleCompare(double a, double b)
{
    if (a < b) return -1;
    if (a > b) return 1;
    const int64_t x = gf_render_double_bits(a), y = gf_render_double_bits(b);
    return x == y ? 0 : (x < y ? -1 : 1);
}

// the constructor's work (ColorPaletteTable.java:199-252; the records' own: ColorPaletteRecordRGB.java:76-84,
// ColorPaletteRecordHSV.java:98-125) and the checks the host can make
gf_status palettePack(const gf_palette_spec *spec, std::vector<uint8_t> &packed)
{
    if (!spec || !spec->records || spec->n_records < 1) return GF_ERR_ARG;
    const int32_t n = spec->n_records;
    for (int32_t i = 0; i < n; i++) {
        const gf_palette_record &r = spec->records[i];
        if (!(r.range0 <= r.range1)) return GF_ERR_ARG;
        if (r.model != GF_PALETTE_RGB && r.model != GF_PALETTE_HSV) return GF_ERR_ARG;
        if (r.model == GF_PALETTE_RGB)
            for (int k = 0; k < 3; k++)
                if (r.rgb0[k] < 0 || r.rgb0[k] > 255 || r.rgb1[k] < 0 || r.rgb1[k] > 255) return GF_ERR_ARG;
    }
    // (the sort and the hinge are looked at before the count's limit: ARG before UNSUPPORTED)
    std::vector<const gf_palette_record *> order((size_t)n);
    for (int32_t i = 0; i < n; i++) order[(size_t)i] = spec->records + i;
    std::stable_sort(order.begin(), order.end(), [](const gf_palette_record *a, const gf_palette_record *b) {
        const int t = javaDoubleCompare(a->range0, b->range0);
        return (t != 0 ? t : javaDoubleCompare(a->range1, b->range1)) < 0;
    });
    int32_t hingeIndex = -1;
    if (spec->hinge) {
        for (int32_t i = 0; i < n && hingeIndex < 0; i++)
            if (order[(size_t)i]->range0 == spec->hinge_value) hingeIndex = i;
        if (hingeIndex < 0) return GF_ERR_ARG;
        if (spec->normalized && hingeIndex == 0) return GF_ERR_ARG;            // (the reference would index records[-1])
    }
    if (n > GF_PALETTE_MAX_RECORDS) return GF_ERR_UNSUPPORTED;

    packed.assign(sizeof(GfPalHead) + (size_t)n * (sizeof(double) + sizeof(GfPalRec)), 0);
    GfPalHead h{};
    h.n = n, h.argbForNull = spec->argb_for_null;
    h.normalized = spec->normalized != 0, h.hinge = spec->hinge != 0, h.hingeIndex = hingeIndex;
    h.rangeMin = order[0]->range0, h.rangeMax = order[(size_t)n - 1]->range1;
    h.normMin = spec->range_min, h.normMax = spec->range_max, h.hingeValue = spec->hinge_value;
    memcpy(packed.data(), &h, sizeof(h));
    double *keys = reinterpret_cast<double *>(packed.data() + sizeof(GfPalHead));
    GfPalRec *recs = reinterpret_cast<GfPalRec *>(keys + n);
    for (int32_t i = 0; i < n; i++) {
        const gf_palette_record &r = *order[(size_t)i];
        GfPalRec o{};
        keys[i] = o.range0 = r.range0, o.range1 = r.range1;
        o.model = r.model;
        if (r.model == GF_PALETTE_RGB) {
            for (int k = 0; k < 3; k++) o.c0[k] = r.rgb0[k], o.d[k] = r.rgb1[k] - r.rgb0[k];
        } else {
            for (int k = 0; k < 3; k++) o.c0[k] = r.hsv0[k];
            o.d[1] = r.hsv1[1] - r.hsv0[1];
            o.d[2] = r.hsv1[2] - r.hsv0[2];
            double dH = r.hsv1[0] - r.hsv0[0];
            if (fabs(dH) < 1.0e-6) {
                o.d[0] = 0;
            } else {
                if (dH <= -180) dH += 360;
                else if (dH > 180) dH -= 360;
                if (dH == 0) dH = 360;
                o.d[0] = dH;
            }
            o.wrapAround = r.hsv0[0] + o.d[0] > 360.0 || r.hsv0[0] + o.d[0] < 0;
        }
        recs[i] = o;
    }
    return GF_OK;
}

void palOf(const gf_palette *p, int flags, GfRenderPal &pal)
{
    pal.head = p->head();
    pal.table = reinterpret_cast<const double *>((const uint8_t *)p->dTable + sizeof(GfPalHead));
    pal.unlimited = (flags & GF_RENDER_UNLIMITED) != 0;
}

// what the host can check of an interpolating render call; fills a.ip.g, the light and the outputs
gf_status renderArgs(const gf_context *c, const gf_interp_spec *spec, const void *block, bool perPointSpacing, const gf_palette *palette,
                     const gf_render_light *light, int flags, const gf_render_out *out, GfRenderArgs &a)
{
    if (!c || !spec || !block || !palette || !out) return GF_ERR_ARG;
    if (!out->argb && !out->shade) return GF_ERR_ARG;
    if (out->shade && !light) return GF_ERR_ARG;
    if (flags & ~GF_RENDER_UNLIMITED) return GF_ERR_ARG;
    gf_interp_spec s = *spec;
    s.target = light ? GF_INTERP_FIRST : GF_INTERP_VALUE;                       // (what is evaluated; the caller's is checked too)
    if (spec->target < GF_INTERP_VALUE || spec->target > GF_INTERP_SECOND) return GF_ERR_ARG;
    const gf_status st = interpSpecArgs(c, &s, block, perPointSpacing, a.ip.g);
    if (st != GF_OK) return st;
    a.lit = light != nullptr;
    if (light) {
        a.light.xGain = light->x_gain, a.light.yGain = light->y_gain, a.light.ambient = light->ambient;
        for (int k = 0; k < 3; k++) a.light.sun[k] = light->sun[k];
    }
    a.argb = reinterpret_cast<uint32_t *>(out->argb), a.shade = out->shade, a.status = out->status;
    return GF_OK;
}

gf_status latticeArgs(const gf_interp_lattice *lat, GfInterpArgs &ip)
{
    if (!lat || lat->n_rows < 1 || lat->n_cols < 1) return GF_ERR_ARG;
    if ((uint64_t)lat->n_rows > (((uint64_t)1 << 63) - 1) / (uint64_t)lat->n_cols) return GF_ERR_UNSUPPORTED;   // 2^63 or more points
    ip.nPoints = (size_t)lat->n_rows * (size_t)lat->n_cols;
    ip.latRow0 = lat->row0, ip.latCol0 = lat->col0, ip.latRowStep = lat->row_step, ip.latColStep = lat->col_step;
    ip.latRows = (uint64_t)lat->n_rows, ip.latCols = (uint64_t)lat->n_cols;
    return GF_OK;
}

}  // namespace

extern "C" {

gf_status gf_palette_create(gf_context *c, const gf_palette_spec *spec, gf_palette **out)
{
    if (!out) return GF_ERR_ARG;
    *out = nullptr;
    std::unique_ptr<gf_palette> p(new (std::nothrow) gf_palette());
    if (!p) return GF_ERR_ARG;
    const gf_status s = palettePack(spec, p->packed);
    if (s != GF_OK) return s;
    if (!c) return GF_ERR_ARG;
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    GF_HIP(hipMalloc(&p->dTable, p->packed.size()));
    const hipError_t e = hipMemcpy(p->dTable, p->packed.data(), p->packed.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(p->dTable);
        return hipFail(e, "hipMemcpy");
    }
    p->device = c->device;
    *out = p.release();
    return GF_OK;
}

void gf_palette_destroy(gf_palette *p)
{
    if (!p) return;
    if (p->dTable) {
        (void)hipSetDevice(p->device);
        (void)hipFree(p->dTable);
    }
    delete p;
}

// Not part of the public ABI (tests load them by name): a palette checked, sorted and packed without a device, and a palette's
// packed table (GfPalHead | keys[n] | recs[n], gvrs_render_common.h)
gf_status gf_internal_palette_create_host(const gf_palette_spec *spec, gf_palette **out)
{
    if (!out) return GF_ERR_ARG;
    *out = nullptr;
    std::unique_ptr<gf_palette> p(new (std::nothrow) gf_palette());
    if (!p) return GF_ERR_ARG;
    const gf_status s = palettePack(spec, p->packed);
    if (s != GF_OK) return s;
    *out = p.release();
    return GF_OK;
}

gf_status gf_internal_palette_table(const gf_palette *p, void *out, size_t cap, size_t *bytes)
{
    if (!p || !bytes) return GF_ERR_ARG;
    *bytes = p->packed.size();
    if (!out || cap < p->packed.size()) return GF_ERR_CAPACITY;
    memcpy(out, p->packed.data(), p->packed.size());
    return GF_OK;
}

gf_status gf_block_render_cells_dev(gf_context *c, void *stream, const gf_palette *palette, int flags, int elemType, int32_t fillI,
                                    const void *dCells, size_t nCells, const double *dShade, int32_t *dArgb)
{
    if (!c || !palette) return GF_ERR_ARG;
    if (flags & ~GF_RENDER_UNLIMITED) return GF_ERR_ARG;
    if (elemType < GF_ELEM_INT || elemType > GF_RENDER_Z) return GF_ERR_ARG;
    if (elemType == GF_ELEM_SHORT && (fillI < -32768 || fillI > 32767)) return GF_ERR_ARG;
    if (nCells && (!dCells || !dArgb)) return GF_ERR_ARG;
    if (((uintptr_t)dCells & (elemType == GF_ELEM_SHORT ? 1u : elemType == GF_RENDER_Z ? 7u : 3u)) || ((uintptr_t)dArgb & 3u) || ((uintptr_t)dShade & 7u)) return GF_ERR_ARG;
    if (nCells > ((size_t)1 << 48)) return GF_ERR_UNSUPPORTED;
    if (nCells == 0) return GF_OK;
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    if (palette->device != c->device) return GF_ERR_ARG;
    GfRenderCellsArgs a{};
    palOf(palette, flags, a.pal);
    a.elemType = elemType, a.fillI = fillI;
    a.cells = dCells, a.shade = dShade, a.argb = reinterpret_cast<uint32_t *>(dArgb), a.nCells = nCells;
    GF_HIP(gf_launch_render_cells(a, streamOf(c, stream)));
    return GF_OK;
}

gf_status gf_block_render_lattice_dev(gf_context *c, void *stream, const gf_interp_spec *spec, const void *dBlock, const gf_interp_lattice *lat,
                                      const gf_palette *palette, const gf_render_light *light, int flags, const gf_render_out *out)
{
    GfRenderArgs a{};
    gf_status s = renderArgs(c, spec, dBlock, false, palette, light, flags, out, a);
    if (s != GF_OK) return s;
    if ((s = latticeArgs(lat, a.ip)) != GF_OK) return s;
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    if (palette->device != c->device) return GF_ERR_ARG;
    palOf(palette, flags, a.pal);
    a.ip.block = dBlock;
    GF_HIP(gf_launch_render(a, streamOf(c, stream)));
    return GF_OK;
}

gf_status gf_block_render_points_dev(gf_context *c, void *stream, const gf_interp_spec *spec, const void *dBlock, const gf_interp_lattice *lat,
                                     size_t nPoints, const double *dRows, const double *dCols, const double *dColSpacing,
                                     const gf_palette *palette, const gf_render_light *light, int flags, const gf_render_out *out)
{
    GfRenderArgs a{};
    gf_status s = renderArgs(c, spec, dBlock, dColSpacing != nullptr, palette, light, flags, out, a);
    if (s != GF_OK) return s;
    if (lat) {
        if (dRows || dCols) return GF_ERR_ARG;                                  // one or the other
        if ((s = latticeArgs(lat, a.ip)) != GF_OK) return s;
    } else {
        if (nPoints && (!dRows || !dCols)) return GF_ERR_ARG;
        if (nPoints == 0) return GF_OK;
        a.ip.nPoints = nPoints;
        a.ip.rows = dRows, a.ip.cols = dCols;
    }
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    if (palette->device != c->device) return GF_ERR_ARG;
    palOf(palette, flags, a.pal);
    a.ip.block = dBlock;
    a.ip.colSpacing = dColSpacing;
    GF_HIP(gf_launch_render(a, streamOf(c, stream)));
    return GF_OK;
}

gf_status gf_block_render_lattice(gf_context *c, const gf_interp_spec *spec, const void *block, const gf_interp_lattice *lat,
                                  const gf_palette *palette, const gf_render_light *light, int flags, const gf_render_out *out)
{
    GfRenderArgs a{};
    gf_status s = renderArgs(c, spec, block, false, palette, light, flags, out, a);
    if (s != GF_OK) return s;
    if ((s = latticeArgs(lat, a.ip)) != GF_OK) return s;
    if (a.ip.nPoints > ((size_t)1 << 56)) return GF_ERR_UNSUPPORTED;           // (the staging sizes below stay in 64 bits)
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    if (palette->device != c->device) return GF_ERR_ARG;
    // staging: block | argb | shade | status, the parts that the call has
    const size_t n = a.ip.nPoints;
    HostStage sg(c);
    const int blockP = sg.in(block, (size_t)a.ip.g.bRows * (size_t)a.ip.g.bCols * (a.ip.g.elemType == GF_ELEM_SHORT ? 2 : 4));
    const int argbP = sg.out(out->argb, n * 4), shadeP = sg.out(out->shade, n * 8), statusP = sg.out(out->status, n * 4);
    if ((s = sg.begin()) != GF_OK) return s;
    palOf(palette, flags, a.pal);
    a.ip.block = sg.ptr<void>(blockP);
    a.argb = sg.ptr<uint32_t>(argbP), a.shade = sg.ptr<double>(shadeP), a.status = sg.ptr<int32_t>(statusP);
    GF_HIP(gf_launch_render(a, c->stream));
    return sg.end();
}

}  // extern "C"
