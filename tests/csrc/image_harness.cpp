// CPU harness for gridfour_amd/csrc/gvrs_image_common.h, the host/device-shared restatement of the reference's image loops
// (ExperimentalImageStorage.java:242-256, :275-286; DemoCOG.java:735-770): the same functions the kernels inline -- the split, the
// join and the packed-word accumulator of the reduce -- compiled with g++ into a program of its own and called item by item.
// Built by tests/image_cases.py for tests/test_image_shared_header.py, once more with -fsanitize=address,undefined.
//   image_harness split  in out : int32 model, int64 n, n words            -> 3 planes of n int32
//   image_harness join   in out : int32 model, int64 n, 3 planes of n int32 -> n words
//   image_harness reduce in out : int32 factor, int64 width, int64 height, width * height words -> (width / f) * (height / f) words
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../gridfour_amd/csrc/gvrs_image_common.h"

namespace {

std::vector<uint8_t> readAll(const char *path)
{
    std::vector<uint8_t> b;
    FILE *f = fopen(path, "rb");
    if (!f) return b;
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) b.insert(b.end(), buf, buf + n);
    fclose(f);
    return b;
}

bool writeAll(const char *path, const void *p, size_t n)
{
    FILE *f = fopen(path, "wb");
    if (!f) return false;
    const bool ok = n == 0 || fwrite(p, 1, n, f) == n;
    return fclose(f) == 0 && ok;
}

template <class T>
T take(const std::vector<uint8_t> &b, size_t &at)
{
    T v{};
    if (at + sizeof(T) <= b.size()) memcpy(&v, b.data() + at, sizeof(T));
    at += sizeof(T);
    return v;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    const std::string mode = argv[1];
    const std::vector<uint8_t> in = readAll(argv[2]);
    size_t at = 0;
    const int32_t first = take<int32_t>(in, at);
    if (mode == "reduce") {
        const int64_t width = take<int64_t>(in, at), height = take<int64_t>(in, at);
        if (first < 1 || first > GF_IMAGE_MAX_FACTOR || width < 0 || height < 0 || in.size() != at + (size_t)(width * height) * 4) return 3;
        std::vector<uint32_t> img((size_t)(width * height));
        if (!img.empty()) memcpy(img.data(), in.data() + at, img.size() * 4);
        const int64_t ow = width / first, oh = height / first;
        std::vector<uint32_t> out((size_t)(ow * oh));
        for (int64_t i = 0; i < oh; i++)
            for (int64_t j = 0; j < ow; j++) out[(size_t)(i * ow + j)] = gf_img_reduce_word(img.data(), width, first, i, j);
        return writeAll(argv[3], out.data(), out.size() * 4) ? 0 : 4;
    }
    const int64_t n = take<int64_t>(in, at);
    if (first < 0 || first > 1 || n < 0) return 3;
    if (mode == "split") {
        if (in.size() != at + (size_t)n * 4) return 3;
        std::vector<int32_t> out((size_t)n * 3);
        for (int64_t i = 0; i < n; i++) {
            uint32_t w;
            memcpy(&w, in.data() + at + (size_t)i * 4, 4);
            int32_t p[3];
            gf_img_split(first, w, p);
            for (int k = 0; k < 3; k++) out[(size_t)(k * n + i)] = p[k];
        }
        return writeAll(argv[3], out.data(), out.size() * 4) ? 0 : 4;
    }
    if (mode == "join") {
        if (in.size() != at + (size_t)n * 12) return 3;
        std::vector<int32_t> p((size_t)n * 3);
        if (!p.empty()) memcpy(p.data(), in.data() + at, p.size() * 4);
        std::vector<uint32_t> out((size_t)n);
        for (int64_t i = 0; i < n; i++) out[(size_t)i] = gf_img_join(first, p[(size_t)i], p[(size_t)(n + i)], p[(size_t)(2 * n + i)]);
        return writeAll(argv[3], out.data(), out.size() * 4) ? 0 : 4;
    }
    return 2;
}
