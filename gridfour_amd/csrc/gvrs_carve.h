// gvrs_carve.h -- the layout of a buffer that holds several parts, stated once: the parts are added in order, each gets its offset,
// and the sum is what the buffer must hold (DevBuf::ensure / PinBuf::ensure of gvrs_api_internal.h take the Carve itself).  Every
// part starts at a multiple of 16 bytes and is rounded up to one.  Plain C++, no HIP include: the host tests build it alone.
#pragma once

#include <cstddef>

struct Carve {
    size_t total = 0;                                   // bytes of the parts so far: the sum of their rounded sizes
    // a part of `bytes` bytes (0 is allowed: it shares its offset with the next part); align: a multiple of 16
    size_t add(size_t bytes, size_t align = 16)
    {
        const size_t at = total;
        total += (bytes + align - 1) / align * align;
        return at;
    }
    // one array per element: at[e] = the offset of count items of itemBytes[e] bytes (+ extra bytes behind them)
    void each(int n, size_t count, const size_t *itemBytes, size_t *at, size_t extra = 0)
    {
        for (int e = 0; e < n; e++) at[e] = add(count * itemBytes[e] + extra);
    }
};
