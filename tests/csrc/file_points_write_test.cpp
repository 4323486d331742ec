// file_points_write_test.cpp -- a stand-alone CPU program around gvrs_file_points_store.h, the cell rule that the block write and the
// writes at scattered points share (TileElement*.setValue, hasValidData).  Built plain and under the address and
// undefined-behaviour sanitizers by tests/test_file_points_write_program.py and compared, value for value, with the table that the
// numpy model (tests/block_write_ref.py) prints.
//   usage: file_points_write_test CASES
// A line of CASES: kind fill fillF lo hi scale offset n v0 v1 ... -- kind 0 INT, 1 SHORT, 2 FLOAT, 3 ICF; everything else the 32
// bits of a word in hex (scale and offset: float bits; a SHORT's value: its low 16 bits).  Per line it prints, per value,
// " <stored 0|1>:<the tile's cell in hex>:<the cell is data 0|1>", and "done" at the end.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../gridfour_amd/csrc/gvrs_file_points_store.h"

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    int kind;
    while (fscanf(f, "%d", &kind) == 1) {
        uint32_t w[6];
        size_t n;
        for (int k = 0; k < 6; k++)
            if (fscanf(f, "%" SCNx32, &w[k]) != 1) return 3;
        if (fscanf(f, "%zu", &n) != 1 || kind < 0 || kind > 3) return 3;
        std::vector<uint32_t> v(n);
        for (size_t k = 0; k < n; k++)
            if (fscanf(f, "%" SCNx32, &v[k]) != 1) return 3;
        const GfStoreElem e = gf_store_elem(kind, w[0], w[1], w[2], w[3], gf_store_float(w[4]), gf_store_float(w[5]));
        for (size_t k = 0; k < n; k++) {
            uint32_t o = 0;
            const bool ok = gf_store_value_of(kind, v[k], e, o);
            // what the tile holds afterwards: the stored cell, or (a refused value) a cell that was fill
            const uint32_t cell = ok ? o : e.fill;
            printf(" %d:%" PRIx32 ":%d", ok ? 1 : 0, ok ? o : 0u, gf_store_valid_of(kind, cell, e) ? 1 : 0);
        }
        printf("\n");
    }
    fclose(f);
    printf("done\n");
    return 0;
}
