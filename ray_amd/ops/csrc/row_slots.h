// A bf16 logits row read in place through the aligned 16-byte slots that cover it, and the
// order-preserving 16-bit key of a bf16 value. Shared by sample.hip and logprobs.hip.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ uint32_t key_of(uint32_t h) {  // h: bf16 bits
  if (h == 0x8000u) h = 0;                                // -0 == +0
  return (h & 0x8000u) ? (~h & 0xffffu) : (h | 0x8000u);
}
__device__ __forceinline__ float val_of(uint32_t key) {
  const uint32_t h = (key & 0x8000u) ? (key & 0x7fffu) : (~key & 0xffffu);
  return __uint_as_float(h << 16);
}
__device__ __forceinline__ uint32_t key_of_val(float v) {
  return key_of(__float_as_uint(v) >> 16);
}

// A row as the aligned 16-byte slots that cover it. Slot j holds the elements with indices
// j * 8 - off .. j * 8 - off + 7; those outside [0, V) (only in the first and the last
// slot) are replaced by -inf, which weighs nothing, is never the maximum of a row that has
// a finite logit and sits below every top-k or top-p threshold.
struct Row {
  const uint4* base;  // the row's start rounded down to 16 bytes
  int off;            // elements between base and the row's start (0..7)
  int V;
  int nslots;
  __device__ __forceinline__ uint4 load(int j) const {
    uint4 u = base[j];
    if (j == 0 || j == nslots - 1) {
      uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int i = j * 8 + e - off;
        if (i < 0 || i >= V)
          w[e >> 1] = (e & 1) ? ((w[e >> 1] & 0x0000ffffu) | 0xff800000u)
                              : ((w[e >> 1] & 0xffff0000u) | 0x0000ff80u);
      }
      u = make_uint4(w[0], w[1], w[2], w[3]);
    }
    return u;
  }
};

// The row of V elements that starts at rowp (any 2-byte alignment).
__device__ __forceinline__ Row row_at(const bf16_t* rowp, int V) {
  Row row;
  row.off = (int)(((uintptr_t)rowp >> 1) & 7);
  row.base = reinterpret_cast<const uint4*>(rowp - row.off);
  row.V = V;
  row.nslots = (row.off + V + 7) >> 3;
  return row;
}

constexpr uint32_t kNegInf2 = 0xff80ff80u;  // two bf16 -inf

}  // namespace
