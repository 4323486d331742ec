// stage_test.cpp -- gridfour_amd/csrc/gvrs_stage.h on its own (no HIP, no library): built with the address and undefined-behaviour
// sanitizers and run by tests/test_stage_header.py.  The "device" is a malloc of exactly the laid-out total, filled with 0xA5, and
// the copier is memcpy: a copy that leaves a part, or a part that leaves the buffer, is the sanitizer's to find.  Exit status 0 and
// "ok" when every property holds.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../gridfour_amd/csrc/gvrs_stage.h"

static int failures = 0;
#define CHECK(x)                                                    \
    do {                                                            \
        if (!(x)) {                                                 \
            printf("line %d: %s\n", __LINE__, #x);                  \
            failures++;                                             \
        }                                                           \
    } while (0)

struct Buf {
    unsigned char *p = nullptr;
    size_t bytes = 0;
    bool busy = false;
    int syncs = 0, copiesIn = 0, copiesOut = 0, fills = 0, moves = 0;
    int failCopyIn = -1;                                            // the copy in of this number fails
    std::string why;
    ~Buf() { free(p); }
};

struct MemDev {
    typedef int Status;
    Buf *b;
    bool &busy() { return b->busy; }
    int reserve(size_t bytes, unsigned char *&base)
    {
        if (bytes != b->bytes || !b->p) {                           // exactly the total, and dirty
            free(b->p);
            b->p = (unsigned char *)malloc(bytes ? bytes : 1);
            b->bytes = bytes;
            b->moves++;
        }
        memset(b->p, 0xA5, bytes);
        base = b->p;
        return 0;
    }
    int toDevice(void *d, const void *h, size_t n)
    {
        if (b->copiesIn++ == b->failCopyIn) return -6;
        memcpy(d, h, n);
        return 0;
    }
    int toHost(void *h, const void *d, size_t n)
    {
        b->copiesOut++;
        memcpy(h, d, n);
        return 0;
    }
    int zero(void *d, size_t n)
    {
        b->fills++;
        memset(d, 0, n);
        return 0;
    }
    int sync()
    {
        b->syncs++;
        return 0;
    }
    int refuse(const char *why)
    {
        b->why = why;
        return -99;
    }
};
typedef Stage<MemDev> TestStage;

static std::vector<uint8_t> pattern(size_t n, int seed)
{
    std::vector<uint8_t> v(n);
    for (size_t i = 0; i < n; i++) v[i] = (uint8_t)(seed + 31 * i + (i >> 8));
    return v;
}

static bool all(const uint8_t *p, size_t n, uint8_t v)
{
    for (size_t i = 0; i < n; i++)
        if (p[i] != v) return false;
    return true;
}

// parts of every kind: laid out at multiples of 16 without overlap inside the total, inputs intact with their slack readable,
// outputs and in-out parts home after end(), one synchronisation
static void everyKind(const std::vector<size_t> &sizes)
{
    Buf buf;
    TestStage sg(MemDev{&buf});
    struct Decl { int part; size_t bytes, slack; unsigned flags; std::vector<uint8_t> host, want; };
    std::vector<Decl> d;
    const unsigned kinds[5] = {STAGE_IN, STAGE_OUT, STAGE_IN | STAGE_OUT, STAGE_LOCAL, STAGE_LOCAL | STAGE_ZERO};
    for (size_t i = 0; i < sizes.size(); i++) {
        Decl x;
        x.bytes = sizes[i], x.flags = kinds[i % 5], x.slack = (x.flags == STAGE_IN && i % 2 == 0) ? 32 : 0;
        x.host = pattern(x.bytes + 1, (int)i);                      // (one more: never null)
        d.push_back(x);
    }
    for (Decl &x : d) x.part = sg.add(x.flags & STAGE_LOCAL ? nullptr : x.host.data(), x.bytes, x.flags, x.slack);
    CHECK(sg.begin() == 0 && buf.busy && buf.bytes == sg.total());
    for (size_t i = 0; i < d.size(); i++) {
        const uint8_t *p = sg.ptr<uint8_t>(d[i].part);
        CHECK(p != nullptr && (size_t)(p - buf.p) % 16 == 0);
        CHECK((size_t)(p - buf.p) + d[i].bytes + d[i].slack <= buf.bytes);
        if (i + 1 < d.size()) CHECK(p + d[i].bytes + d[i].slack <= sg.ptr<uint8_t>(d[i + 1].part));
        if (d[i].flags & STAGE_IN) CHECK(memcmp(p, d[i].host.data(), d[i].bytes) == 0);
        if (d[i].flags & STAGE_ZERO) CHECK(all(p, d[i].bytes, 0));
        if (d[i].flags == STAGE_LOCAL || d[i].flags == STAGE_OUT) CHECK(all(p, d[i].bytes, 0xA5));
        unsigned sum = 0;
        for (size_t j = 0; j < d[i].bytes + d[i].slack; j++) sum += p[j];      // (the slack is inside the buffer)
        CHECK(sum != 0xffffffffu);
    }
    // the "kernel": every part that goes home gets what it held, inverted, or a pattern of its own
    for (Decl &x : d) {
        uint8_t *p = sg.ptr<uint8_t>(x.part);
        x.want.assign(x.bytes + 1, 0);
        for (size_t j = 0; j < x.bytes; j++) {
            if (x.flags == (STAGE_IN | STAGE_OUT)) p[j] = (uint8_t)~p[j];
            else if (x.flags == STAGE_OUT) p[j] = (uint8_t)(j * 7 + x.part);
            x.want[j] = p[j];
        }
    }
    CHECK(sg.end() == 0 && !buf.busy && buf.syncs == 1);
    for (const Decl &x : d) {
        if (x.flags & STAGE_OUT) CHECK(memcmp(x.host.data(), x.want.data(), x.bytes) == 0);
        else CHECK(x.host == pattern(x.bytes + 1, (int)(&x - d.data())));      // (an input's host side is left alone)
        CHECK(x.host[x.bytes] == pattern(x.bytes + 1, (int)(&x - d.data()))[x.bytes]);
    }
}

int main()
{
    everyKind({});
    everyKind({1});
    everyKind({16, 17, 15, 1, 3, 4096, 33, 100, 5, 64});
    everyKind({40, 0, 8, 0, 0, 31, 32, 1, 0, 7, 1000003, 2, 2, 2, 2});
    {
        std::vector<size_t> many;
        for (int i = 0; i < STAGE_MAX_PARTS; i++) many.push_back((size_t)(i * 7919) % 97);
        everyKind(many);                                            // the table full: still a stage
    }

    // a fetch copies its prefix only, and flush() passes a fetched part over; a held part goes home by fetch() alone
    {
        Buf buf;
        std::vector<uint8_t> a(100, 0xEE), b(100, 0xEE), h(100, 0xEE);
        TestStage sg(MemDev{&buf});
        const int aP = sg.out(a.data(), 100), bP = sg.out(b.data(), 100), hP = sg.held(h.data(), 100);
        CHECK(sg.begin() == 0);
        memset(sg.ptr<uint8_t>(aP), 1, 100), memset(sg.ptr<uint8_t>(bP), 2, 100), memset(sg.ptr<uint8_t>(hP), 3, 100);
        CHECK(sg.fetch(aP, 10) == 0);
        CHECK(all(a.data(), 10, 1) && all(a.data() + 10, 90, 0xEE) && all(b.data(), 100, 0xEE));
        CHECK(sg.flush() == 0 && buf.syncs == 1 && buf.busy);
        CHECK(all(a.data() + 10, 90, 0xEE) && all(b.data(), 100, 2) && all(h.data(), 100, 0xEE));
        CHECK(sg.fetch(hP, 37) == 0 && all(h.data(), 37, 3) && all(h.data() + 37, 63, 0xEE));
        CHECK(sg.fetch(hP, 1000) == 0 && all(h.data(), 100, 3));   // (more than the part: the part)
        CHECK(sg.end() == 0 && buf.syncs == 2 && !buf.busy && buf.copiesOut == 4);
    }

    // a null host pointer where the call makes the part optional: no room, nothing copied, a null device pointer; a part of 0
    // bytes shares its offset with the next one and is not null; a held part takes its room without a host pointer
    {
        Buf buf;
        std::vector<uint8_t> in0 = pattern(48, 1), out0(8, 0xEE);
        TestStage sg(MemDev{&buf});
        const int a = sg.in(in0.data(), 48), noIn = sg.in(nullptr, 800), noOut = sg.out(nullptr, 800), noBoth = sg.inout(nullptr, 800);
        const int empty = sg.in(in0.data(), 0), emptyNull = sg.out(nullptr, 0), b = sg.out(out0.data(), 8), h = sg.held(nullptr, 64);
        CHECK(sg.total() == 48 + 16 + 64);
        CHECK(sg.begin() == 0 && buf.copiesIn == 1);
        CHECK(!sg.ptr<void>(noIn) && !sg.ptr<void>(noOut) && !sg.ptr<void>(noBoth));
        CHECK(sg.ptr<uint8_t>(a) == buf.p && sg.ptr<uint8_t>(empty) == buf.p + 48 && sg.ptr<uint8_t>(emptyNull) == buf.p + 48);
        CHECK(sg.ptr<uint8_t>(b) == buf.p + 48 && sg.ptr<uint8_t>(h) == buf.p + 64);
        memset(sg.ptr<uint8_t>(h), 9, 64);                          // (room that is the part's own)
        memset(sg.ptr<uint8_t>(b), 4, 8);
        CHECK(sg.fetch(h, 64) == 0 && sg.fetch(noOut) == 0);        // (nowhere to copy to: nothing is copied)
        CHECK(sg.end() == 0 && buf.copiesOut == 1 && all(out0.data(), 8, 4));
    }

    // zeroed parts are zero in a dirty buffer, neighbours in one fill, and what lies between them stays as it was
    {
        Buf buf;
        TestStage sg(MemDev{&buf});
        const int z0 = sg.local(100, true), z1 = sg.local(0, true), z2 = sg.local(33, true), keep = sg.local(50), z3 = sg.local(7, true);
        CHECK(sg.begin() == 0 && buf.fills == 2);
        CHECK(all(sg.ptr<uint8_t>(z0), 100, 0) && all(sg.ptr<uint8_t>(z2), 33, 0) && all(sg.ptr<uint8_t>(z3), 7, 0));
        CHECK(all(sg.ptr<uint8_t>(keep), 50, 0xA5) && sg.ptr<uint8_t>(z1) == sg.ptr<uint8_t>(z2));
        CHECK(sg.end() == 0);
    }

    // begin on a buffer in use is refused and leaves the first stage as it was; once that has ended, the buffer serves the next
    {
        Buf buf;
        std::vector<uint8_t> in0 = pattern(64, 5), out0(64, 0), in1 = pattern(4096, 6);
        TestStage first(MemDev{&buf});
        const int i0 = first.in(in0.data(), 64), o0 = first.out(out0.data(), 64);
        CHECK(first.begin() == 0);
        const unsigned char *was = buf.p;
        {
            TestStage second(MemDev{&buf});
            second.in(in1.data(), 4096);
            CHECK(second.begin() == -99 && !buf.why.empty());
            CHECK(buf.p == was && buf.moves == 1 && buf.copiesIn == 1 && buf.busy);
        }                                                           // (a stage that never began gives nothing back)
        CHECK(buf.busy && memcmp(first.ptr<uint8_t>(i0), in0.data(), 64) == 0);
        memcpy(first.ptr<uint8_t>(o0), first.ptr<uint8_t>(i0), 64);
        CHECK(first.end() == 0 && !buf.busy && out0 == in0);
        TestStage third(MemDev{&buf});
        const int i1 = third.in(in1.data(), 4096);
        CHECK(third.begin() == 0 && buf.moves == 2 && memcmp(third.ptr<uint8_t>(i1), in1.data(), 4096) == 0);
    }                                                               // (... and a stage that goes out of scope gives the buffer back)

    // an error path gives the buffer back: a copy that fails in begin(), and a return between begin() and end()
    {
        Buf buf;
        std::vector<uint8_t> in0 = pattern(64, 7);
        buf.failCopyIn = 1;
        {
            TestStage sg(MemDev{&buf});
            sg.in(in0.data(), 64), sg.in(in0.data(), 32), sg.in(in0.data(), 16);
            CHECK(sg.begin() == -6 && buf.busy && buf.copiesIn == 2);
        }
        CHECK(!buf.busy);
        {
            TestStage sg(MemDev{&buf});
            sg.in(in0.data(), 64);
            CHECK(sg.begin() == 0 && buf.busy);
        }
        CHECK(!buf.busy && buf.syncs == 0);
    }

    // one declaration more than the table holds: refused, not written past the table, and the buffer is not taken
    {
        Buf buf;
        std::vector<uint8_t> in0 = pattern(16, 8);
        TestStage sg(MemDev{&buf});
        for (int i = 0; i < STAGE_MAX_PARTS; i++) CHECK(sg.in(in0.data(), 16) == i);
        const size_t total = sg.total();
        CHECK(sg.in(in0.data(), 16) == 0 && sg.out(in0.data(), 1 << 20) == 0 && sg.total() == total);
        CHECK(sg.begin() == -99 && !buf.why.empty() && !buf.busy && !buf.p && buf.copiesIn == 0);
    }
    if (failures) return 1;
    printf("ok\n");
    return 0;
}
