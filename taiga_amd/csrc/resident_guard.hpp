// resident_guard.hpp — argument and state checks of the resident NTT entry
// points (tg_poly_upload, tg_ntt_resident, tg_poly_download). PRODUCT CODE.
//
// Plain C++ with no HIP runtime dependency, so that the host probe
// (tests/host/resident_guard_probe.cpp) runs the very code the shim runs.
#pragma once

#include <stdint.h>

#include "../../include/taiga_gpu.h"

namespace taiga {

// largest transform size the NTT entry points take: 2^28 elements
constexpr uint32_t TG_NTT_MAX_K = 28;

// k is the caller's size argument; poly_k is the size of the polynomial the
// context holds, or -1 when it holds none. k is tested as the unsigned value
// it arrives as, before it is shifted by or converted to a signed type:
// TG_ERR_BADARG for k > TG_NTT_MAX_K, then, where the call needs resident
// data, TG_ERR_STATE unless a polynomial of exactly 2^k elements is resident.
// On TG_OK *n_out is the element count 2^k; otherwise it is 0.
inline int ntt_size_guard(uint32_t k, int poly_k, bool need_resident, uint64_t* n_out) {
  *n_out = 0;
  if (k > TG_NTT_MAX_K) return TG_ERR_BADARG;
  if (need_resident && (poly_k < 0 || (uint32_t)poly_k != k)) return TG_ERR_STATE;
  *n_out = (uint64_t)1 << k;
  return TG_OK;
}

}  // namespace taiga
