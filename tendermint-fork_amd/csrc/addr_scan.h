// addr_scan.h — GetByAddress (types/validator_set.go:270-278) by one wavefront: the scan of
// evidence_lookup_kernel (evidence.hip) and lca_lookup_kernel (lca.hip).  Device only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "evidence_free.h"

namespace tmed {

constexpr uint32_t kScanLanes = 64;  // one wavefront

// The first validator, in index order, of the nv whose 20-byte addresses start at `set` (five dwords
// each, 4-byte aligned) that equals `want` under bytes.Equal; kEvNone for nobody.  Every lane of the
// wavefront calls it with the same arguments and gets the same answer: the lanes stride over the
// set, the first stride in which a lane matches ends the scan, and the lowest matching lane of that
// stride (from the ballot) is the first match.  The loop is wave-uniform.
__device__ __forceinline__ uint32_t wave_first_address(const uint32_t want[5], const uint32_t *set, uint32_t nv,
                                                       uint32_t lane) {
  for (uint32_t base = 0; base < nv; base += kScanLanes) {
    const uint32_t v = base + lane;
    const bool m = v < nv && ev_addr_match(want, set + 5 * (size_t)v);
    const unsigned long long hit = __ballot(m);
    if (hit) return base + (uint32_t)__ffsll(hit) - 1;
  }
  return kEvNone;
}

}  // namespace tmed
