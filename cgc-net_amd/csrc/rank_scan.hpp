// The rank of a 256-bin histogram held by one wave, four bins per lane (rank.hip: the histogram of a window; region.hip: the histogram
// of a region): an inclusive prefix sum over the 64 lanes in registers, and the bin in which a given rank falls.
#pragma once
#include <stdint.h>

#include "common.hpp"

namespace {

// The inclusive prefix sum of x over the 64 lanes, in registers (DPP): the lane's three left neighbours inside its row of 16, then
// shifts by 4 and 8 inside the row, then the last lane of rows 0 and 2 into rows 1 and 3, then lane 31 into rows 2 and 3.  A lane
// that a step does not write, or whose source lies outside its row, adds 0.
template <int CTRL, int ROW_MASK, int BANK_MASK>
__device__ __forceinline__ uint32_t rank_dpp(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, BANK_MASK, false);
}
__device__ __forceinline__ uint32_t rank_wave_scan(uint32_t x) {
  uint32_t v = x + rank_dpp<0x111, 0xf, 0xf>(x);                        // row_shr:1
  v += rank_dpp<0x112, 0xf, 0xf>(x);                                    // row_shr:2
  v += rank_dpp<0x113, 0xf, 0xf>(x);                                    // row_shr:3
  v += rank_dpp<0x114, 0xf, 0xe>(v);                                    // row_shr:4, lanes 4 .. 15 of a row
  v += rank_dpp<0x118, 0xf, 0xc>(v);                                    // row_shr:8, lanes 8 .. 15
  v += rank_dpp<0x142, 0xa, 0xf>(v);                                    // row_bcast:15, rows 1 and 3
  v += rank_dpp<0x143, 0xc, 0xf>(v);                                    // row_bcast:31, rows 2 and 3
  return v;
}

// the value of rank k < n: c the lane's four bins, incl the inclusive scan of their sums
__device__ __forceinline__ int rank_value(const uint4& c, uint32_t incl, uint32_t k) {
  const unsigned long long above = __ballot(incl > k);                  // not 0: the last lane's incl is n > k
  const int lane = __builtin_ctzll(above);
  const uint32_t c0 = __builtin_amdgcn_readlane(c.x, lane), c1 = __builtin_amdgcn_readlane(c.y, lane);
  const uint32_t c2 = __builtin_amdgcn_readlane(c.z, lane), c3 = __builtin_amdgcn_readlane(c.w, lane);
  uint32_t below = __builtin_amdgcn_readlane(incl, lane) - (c0 + c1 + c2 + c3);      // <= k
  int bin = 4 * lane;
  below += c0;
  if (below > k) return bin;
  below += c1;
  if (below > k) return bin + 1;
  below += c2;
  return below > k ? bin + 2 : bin + 3;
}

}  // namespace
