// CPU harness for gridfour_amd/csrc/gvrs_render_common.h (and gvrs_interp_common.h beneath it), the host/device-shared restatement
// of the reference's colour palette lookup and shaded relief: the same functions the kernels of gvrs_render.hip inline, compiled
// with g++ and called value by value.  A program of its own, built and run by tests/test_render_shared_header.py (g++ -O2
// -ffp-contract=off, and once more with -fsanitize=address,undefined):
//     render_harness lookup  IN OUT     values or cells through a palette
//     render_harness lattice IN OUT     a lattice over a block: interpolation, shade, palette
// IN and OUT are binary files (tests/render_cases.py writes and reads them); a blob is an int64 length and its bytes.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../gridfour_amd/csrc/gvrs_render_common.h"

namespace {

struct Reader {
    std::vector<uint8_t> data;
    size_t at = 0;
    bool ok = true;
    bool take(void *dst, size_t n)
    {
        if (!ok || n > data.size() - at) return ok = false;
        if (n) memcpy(dst, data.data() + at, n);
        at += n;
        return true;
    }
    template <class T> T get()
    {
        T v{};
        take(&v, sizeof(T));
        return v;
    }
    template <class T> std::vector<T> array(size_t n)
    {
        std::vector<T> v;
        if (!ok || n > (data.size() - at) / sizeof(T)) { ok = false; return v; }
        v.resize(n);
        take(v.data(), n * sizeof(T));
        return v;
    }
    std::vector<uint8_t> blob()
    {
        const int64_t n = get<int64_t>();
        if (n < 0) { ok = false; return {}; }
        return array<uint8_t>((size_t)n);
    }
};

struct Table {
    GfPalHead head{};
    std::vector<double> keys;
    std::vector<GfPalRec> recs;
    bool load(Reader &in)
    {
        const std::vector<uint8_t> b = in.blob();
        if (!in.ok || b.size() < sizeof(GfPalHead)) return false;
        memcpy(&head, b.data(), sizeof(head));
        if (head.n < 1 || head.n > GF_PAL_MAX_RECORDS || b.size() != sizeof(GfPalHead) + (size_t)head.n * (sizeof(double) + sizeof(GfPalRec))) return false;
        keys.resize((size_t)head.n), recs.resize((size_t)head.n);
        memcpy(keys.data(), b.data() + sizeof(GfPalHead), keys.size() * sizeof(double));
        memcpy(recs.data(), b.data() + sizeof(GfPalHead) + keys.size() * sizeof(double), recs.size() * sizeof(GfPalRec));
        return true;
    }
};

bool writeAll(const char *path, const std::vector<uint8_t> &out)
{
    FILE *f = fopen(path, "wb");
    if (!f) return false;
    const bool ok = out.empty() || fwrite(out.data(), 1, out.size(), f) == out.size();
    return fclose(f) == 0 && ok;
}

template <class T> void append(std::vector<uint8_t> &out, const std::vector<T> &v)
{
    const uint8_t *p = reinterpret_cast<const uint8_t *>(v.data());
    out.insert(out.end(), p, p + v.size() * sizeof(T));
}

int lookup(Reader &in, std::vector<uint8_t> &out)
{
    Table t;
    if (!t.load(in)) return 2;
    const int64_t n = in.get<int64_t>();
    const int32_t elemType = in.get<int32_t>(), fill = in.get<int32_t>(), withShade = in.get<int32_t>(), unlimited = in.get<int32_t>();
    const std::vector<uint8_t> values = in.blob();
    if (!in.ok || n < 0 || elemType < -1 || elemType > 3) return 2;
    const size_t item = elemType == -1 ? 8 : elemType == 1 ? 2 : 4;
    if (values.size() != (size_t)n * item) return 2;
    const std::vector<double> shades = in.array<double>(withShade ? (size_t)n : 0);
    if (!in.ok) return 2;
    std::vector<uint32_t> argb((size_t)n);
    for (size_t i = 0; i < (size_t)n; i++) {
        double z;
        if (elemType == -1) {
            memcpy(&z, values.data() + 8 * i, 8);
        } else if (elemType == 1) {
            int16_t c;
            memcpy(&c, values.data() + 2 * i, 2);
            z = gf_render_cell_i32(c, fill);
        } else {
            uint32_t c;
            memcpy(&c, values.data() + 4 * i, 4);
            z = elemType >= 2 ? gf_render_cell_f32(c) : gf_render_cell_i32((int32_t)c, fill);
        }
        argb[i] = gf_render_palette(t.head, t.keys.data(), t.recs.data(), z, withShade ? shades[i] : 0.0, withShade != 0, unlimited != 0);
    }
    append(out, argb);
    return 0;
}

int lattice(Reader &in, std::vector<uint8_t> &out)
{
    Table t;
    if (!t.load(in)) return 2;
    const std::vector<uint8_t> geom = in.blob(), block = in.blob();
    if (!in.ok || geom.size() != sizeof(GfInterpGeom)) return 2;
    GfInterpGeom g;
    memcpy(&g, geom.data(), sizeof(g));
    const double row0 = in.get<double>(), col0 = in.get<double>(), rowStep = in.get<double>(), colStep = in.get<double>();
    const int64_t nRows = in.get<int64_t>(), nCols = in.get<int64_t>();
    const int32_t hasCs = in.get<int32_t>(), lit = in.get<int32_t>(), unlimited = in.get<int32_t>();
    if (!in.ok || nRows < 1 || nCols < 1 || nRows > 100000 || nCols > 100000) return 2;
    if (g.bRows < 4 || g.bCols < 4 || block.size() != (size_t)g.bRows * (size_t)g.bCols * (g.elemType == 1 ? 2 : 4)) return 2;
    const std::vector<double> cs = in.array<double>(hasCs ? (size_t)nRows : 0);
    GfRenderLight light{};
    if (lit) {
        light.xGain = in.get<double>(), light.yGain = in.get<double>();
        for (int k = 0; k < 3; k++) light.sun[k] = in.get<double>();
        light.ambient = in.get<double>();
    }
    if (!in.ok) return 2;
    // the block behind 16 spare bytes: gf_interp_samples reads whole windows that lie inside it, nothing else
    std::vector<uint32_t> cells((block.size() + 3) / 4 + 4);
    memcpy(cells.data(), block.data(), block.size());
    const size_t n = (size_t)nRows * (size_t)nCols;
    std::vector<uint32_t> argb(n);
    std::vector<double> shade(n);
    std::vector<int32_t> status(n);
    for (int64_t i = 0; i < nRows; i++)
        for (int64_t j = 0; j < nCols; j++) {
            const size_t p = (size_t)i * (size_t)nCols + (size_t)j;
            GfInterpResult r;
            status[p] = gf_interp_point(g, cells.data(), row0 + (double)i * rowStep, col0 + (double)j * colStep, hasCs ? cs[(size_t)i] : g.colSpacing, false, r);
            shade[p] = lit ? gf_render_shade(r.zx, r.zy, light) : 0.0;
            argb[p] = gf_render_palette(t.head, t.keys.data(), t.recs.data(), r.z, shade[p], lit != 0, unlimited != 0);
        }
    append(out, argb);
    if (out.size() % 8) out.insert(out.end(), 4, 0);
    append(out, shade);
    append(out, status);
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 4) {
        fprintf(stderr, "usage: render_harness lookup|lattice IN OUT\n");
        return 2;
    }
    Reader in;
    FILE *f = fopen(argv[2], "rb");
    if (!f) return 2;
    uint8_t buf[65536];
    for (size_t k; (k = fread(buf, 1, sizeof(buf), f)) > 0;) in.data.insert(in.data.end(), buf, buf + k);
    fclose(f);
    std::vector<uint8_t> out;
    const std::string mode = argv[1];
    const int rc = mode == "lookup" ? lookup(in, out) : mode == "lattice" ? lattice(in, out) : 2;
    if (rc != 0) return rc;
    return writeAll(argv[3], out) ? 0 : 2;
}
