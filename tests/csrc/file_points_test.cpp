// file_points_test.cpp -- a stand-alone program around gvrs_file_points.h (with gvrs_interp_common.h behind it), for the CPU: the
// cases of a text file, one a line, answered one line each; tests/test_file_points_program.py compares the lines with those of the
// numpy restatement and builds the program plain and under the address and undefined-behaviour sanitizers.
//   cells   nRowsGrid nColsGrid nRowsTile nColsTile n  row col ...                                  (int32 cells)
//   windows nRowsGrid nColsGrid nRowsTile nColsTile wrap rowFringe0 rowFringe1 colFringe0 colFringe1 n  row col ...   (doubles, as
//           strtod reads them: hexadecimal floats, nan, inf)
// The answer: per point its tile:indexInTile (cells) or its window's tiles t,t,... (windows), x for a refused point; then the touched
// tiles in ascending order; then "slots ok" when every touched tile's slot by the bitmap rule is its place in that list.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../gridfour_amd/csrc/gvrs_file_points.h"

static bool finish(const GfPointsGrid &g, const std::vector<uint32_t> &bits)
{
    std::vector<uint32_t> prefix(bits.size());
    uint32_t sum = 0;
    for (size_t w = 0; w < bits.size(); w++) {
        prefix[w] = sum;
        sum += gf_points_popcount(bits[w]);
    }
    printf("; tiles");
    uint32_t place = 0;
    bool ok = true;
    for (int32_t t = 0; t < g.nTilesGrid; t++) {
        if (!(bits[(uint32_t)t >> 5] >> ((uint32_t)t & 31u) & 1u)) continue;
        printf(" %d", t);
        ok = ok && gf_points_slot(bits.data(), prefix.data(), t) == place;
        place++;
    }
    printf("; slots %s\n", ok && place == sum ? "ok" : "WRONG");
    return ok;
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    if (!in) return 2;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream s(line);
        std::string kind;
        int32_t nRG, nCG, nRT, nCT;
        s >> kind >> nRG >> nCG >> nRT >> nCT;
        const GfPointsGrid g = gf_points_grid(nRG, nCG, nRT, nCT);
        std::vector<uint32_t> bits(gf_points_words(g.nTilesGrid), 0u);
        if (kind == "cells") {
            size_t n;
            s >> n;
            printf("cells:");
            for (size_t k = 0; k < n; k++) {
                int32_t row, col, tile = 0, at = 0;
                s >> row >> col;
                if (!gf_points_cell(g, row, col, tile, at)) {
                    printf(" x");
                    continue;
                }
                printf(" %d:%d", tile, at);
                bits[(uint32_t)tile >> 5] |= 1u << ((uint32_t)tile & 31u);
            }
        } else if (kind == "windows") {
            GfInterpGeom ig = GfInterpGeom();
            gf_points_whole_grid(ig, g);
            std::string f[4];
            size_t n;
            s >> ig.wrap >> f[0] >> f[1] >> f[2] >> f[3] >> n;
            ig.rowFringe0 = strtod(f[0].c_str(), nullptr), ig.rowFringe1 = strtod(f[1].c_str(), nullptr);
            ig.colFringe0 = strtod(f[2].c_str(), nullptr), ig.colFringe1 = strtod(f[3].c_str(), nullptr);
            printf("windows:");
            for (size_t k = 0; k < n; k++) {
                std::string a, b;
                s >> a >> b;
                GfInterpWindow w;
                if (gf_interp_window(ig, strtod(a.c_str(), nullptr), strtod(b.c_str(), nullptr), w) != GF_IP_OK) {
                    printf(" x");
                    continue;
                }
                if (!gf_interp_window_in_block(ig, w.row0, w.col0, w.n1)) return 3;      // (the whole grid is the block)
                const GfWindowTiles wt = gf_points_window_tiles(g, w.row0, w.col0, w.n1);
                int32_t last = -1;
                for (int32_t j = 0; j < wt.count(); j++) {
                    const int32_t t = wt.at(j);
                    if (t <= last || t >= g.nTilesGrid) return 4;                        // (ascending, distinct, inside the grid)
                    last = t;
                    printf("%s%d", j ? "," : " ", t);
                    bits[(uint32_t)t >> 5] |= 1u << ((uint32_t)t & 31u);
                }
            }
        } else
            return 2;
        if (!s) return 2;
        if (!finish(g, bits)) return 5;
    }
    printf("done\n");
    return 0;
}
