// carve_test.cpp -- gridfour_amd/csrc/gvrs_carve.h on its own (no HIP, no library): built with the address and undefined-behaviour
// sanitizers and run by tests/test_carve_header.py.  Exit status 0 and "ok" when every property holds.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../gridfour_amd/csrc/gvrs_carve.h"

static int failures = 0;
#define CHECK(x)                                                    \
    do {                                                            \
        if (!(x)) {                                                 \
            printf("line %d: %s\n", __LINE__, #x);                  \
            failures++;                                             \
        }                                                           \
    } while (0)

static size_t up16(size_t v) { return (v + 15) / 16 * 16; }

// parts of these sizes: offsets are multiples of 16, parts do not overlap, the total is the sum of the rounded parts, and every
// part written full stays inside an allocation of exactly `total` bytes
static void parts(const std::vector<size_t> &sizes)
{
    Carve k;
    std::vector<size_t> at;
    size_t sum = 0;
    for (size_t b : sizes) {
        at.push_back(k.add(b));
        sum += up16(b);
        CHECK(k.total == sum);
    }
    for (size_t i = 0; i < sizes.size(); i++) {
        CHECK(at[i] % 16 == 0);
        CHECK(at[i] + sizes[i] <= k.total);
        if (i + 1 < sizes.size()) CHECK(at[i] + sizes[i] <= at[i + 1]);
    }
    uint8_t *buf = (uint8_t *)malloc(k.total ? k.total : 1);
    for (size_t i = 0; i < sizes.size(); i++) memset(buf + at[i], (int)(i + 1), sizes[i]);
    for (size_t i = 0; i < sizes.size(); i++)                       // (no part wrote into another)
        for (size_t j = 0; j < sizes[i]; j++)
            if (buf[at[i] + j] != (uint8_t)(i + 1)) {
                CHECK(!"a part was overwritten");
                break;
            }
    free(buf);
}

int main()
{
    parts({});
    parts({0});
    parts({1});
    parts({16, 17, 15, 0, 0, 1, 4096, 33});
    parts({0, 0, 5, 0, 31, 32, 0});
    parts({6, 2, 4, 8, 24, 3, 1000003});
    std::vector<size_t> many;
    for (size_t i = 0; i < 200; i++) many.push_back((i * 7919) % 97);
    parts(many);

    // a zero-byte part shares its offset with the next one
    {
        Carve k;
        const size_t a = k.add(40), z = k.add(0), b = k.add(8);
        CHECK(a == 0 && z == 48 && b == 48 && k.total == 64);
    }
    // a coarser alignment: a multiple of 16, parts rounded to it
    {
        Carve k;
        const size_t a = k.add(9 * 8, 64), b = k.add(8 * 4, 64), c = k.add(0, 64), d = k.add(8, 64);
        CHECK(a == 0 && b == 128 && c == 192 && d == 192 && k.total == 256);
    }
    // the per-element form with mixed 2- and 4-byte items is the loop it replaces, with and without spare bytes
    for (size_t count : {(size_t)0, (size_t)1, (size_t)7, (size_t)255, (size_t)120 * 150 * 33})
        for (size_t extra : {(size_t)0, (size_t)4}) {
            const size_t item[8] = {4, 2, 2, 4, 4, 2, 4, 2};
            for (int n = 0; n <= 8; n++) {
                size_t bytes = 0, want[8];
                for (int e = 0; e < n; e++) {
                    want[e] = bytes;
                    bytes += up16(count * item[e] + extra);
                }
                Carve k;
                const size_t before = k.add(24);
                size_t at[8];
                k.each(n, count, item, at, extra);
                CHECK(before == 0 && k.total == 32 + bytes);
                for (int e = 0; e < n; e++) CHECK(at[e] == 32 + want[e]);
            }
        }
    // ... and written full inside an allocation of exactly the total
    {
        const size_t item[3] = {2, 4, 2}, count = 333;
        Carve k;
        size_t at[3];
        k.each(3, count, item, at, 4);
        uint8_t *buf = (uint8_t *)malloc(k.total);
        for (int e = 0; e < 3; e++) memset(buf + at[e], 0xA0 + e, count * item[e] + 4);
        for (int e = 0; e < 3; e++) CHECK(buf[at[e]] == 0xA0 + e && buf[at[e] + count * item[e] + 3] == 0xA0 + e);
        free(buf);
    }
    if (failures) return 1;
    printf("ok\n");
    return 0;
}
