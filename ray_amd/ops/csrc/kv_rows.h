// The cache-row mover shared by kv_insert_kernel, kv_copy_kernel (kv_slots.hip) and
// kv_append_kernel (attn_extend.hip): a workgroup of kKvThreads moves kKvBlockRows positions
// of one (row, head), K and V, into a [.., Tmax, 64] bf16 cache. A 128-byte row is 8 lanes x
// 16 B; thread x owns chunk x & 7 of position (x >> 3) of each pass.
#pragma once
#include "common.h"

constexpr int kKvThreads = 256;
constexpr int kKvRowsPerPass = kKvThreads / 8;  // 32 positions: one 16-byte lane chunk each
constexpr int kKvPasses = 2;
constexpr int kKvBlockRows = kKvRowsPerPass * kKvPasses;

// sk, sv / dk, dv: position 0 of the source / destination rows AT THIS LANE'S CHUNK
// (+ (threadIdx.x & 7) * 8 elements); `sstride`: elements between source positions (the
// destination's is 64). Moves positions t0 .. min(t0 + kKvBlockRows, len) - 1; the caller has
// tested t0 < len and that 0 .. len - 1 are real positions of both sides.
// No branch in here, so all four loads are in flight before the first store: a lane past the
// row's end moves position len - 1 instead, the same bytes that position's own lane writes.
__device__ __forceinline__ void kv_move_rows(const bf16_t* sk, const bf16_t* sv, long sstride,
                                             bf16_t* dk, bf16_t* dv, int t0, int len) {
  const int r = threadIdx.x >> 3;
  // (byte offsets: the position's 64-bit multiply-add then carries the base address of K and
  // of V, with no shift and add behind it on the way to the loads)
  const char* sk8 = reinterpret_cast<const char*>(sk);
  const char* sv8 = reinterpret_cast<const char*>(sv);
  uint4 kk[kKvPasses], vv[kKvPasses];
#pragma unroll
  for (int u = 0; u < kKvPasses; ++u) {
    const int t = min(t0 + u * kKvRowsPerPass + r, len - 1);
    kk[u] = *reinterpret_cast<const uint4*>(sk8 + (long)t * (sstride * 2));
    vv[u] = *reinterpret_cast<const uint4*>(sv8 + (long)t * (sstride * 2));
  }
#pragma unroll
  for (int u = 0; u < kKvPasses; ++u) {
    const int t = min(t0 + u * kKvRowsPerPass + r, len - 1);
    *reinterpret_cast<uint4*>(dk + (long)t * 64) = kk[u];
    *reinterpret_cast<uint4*>(dv + (long)t * 64) = vv[u];
  }
}
