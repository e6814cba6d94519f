// ugp_sort.hpp -- the device radix sort (rocprim) behind one call.  Only the files that sort include it: it compiles rocprim.
#pragma once
#include <rocprim/device/device_radix_sort.hpp>

#include "ugp_dense.hpp"

namespace ugp {

// (kin, vin)[0, n) stably by the low `bits` of the key into (kout, vout); tmp grows to the sort's temporary storage.
template <typename K>
hipError_t sort_pairs(DBuf<unsigned char> &tmp, const K *kin, K *kout, const uint32_t *vin, uint32_t *vout, size_t n, unsigned bits,
                      hipStream_t st) {
    size_t bytes = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, bytes, kin, kout, vin, vout, n, 0u, bits, st);
    if (e == hipSuccess) e = tmp.alloc(bytes);
    if (e == hipSuccess) e = rocprim::radix_sort_pairs(tmp.p, bytes, kin, kout, vin, vout, n, 0u, bits, st);
    return e;
}

}  // namespace ugp
