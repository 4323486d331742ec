// The yardstick of tools/tabulate_rate.py: rocprim::radix_sort_keys on the same 32-bit keys the symbol tabulation sorts.  Compiled
// into the tool's own small library (tools/bin/libtab_rocprim.so) only; the product links no rocPRIM.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include <rocprim/rocprim.hpp>

extern "C" {

int tr_sort_temp_bytes(size_t n, size_t *bytes)
{
    *bytes = 0;
    return (int)rocprim::radix_sort_keys(nullptr, *bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr, n, 0, 32, (hipStream_t) nullptr);
}

int tr_sort(void *temp, size_t bytes, const uint32_t *in, uint32_t *out, size_t n, void *stream)
{
    return (int)rocprim::radix_sort_keys(temp, bytes, in, out, n, 0, 32, (hipStream_t)stream);
}

}  // extern "C"
