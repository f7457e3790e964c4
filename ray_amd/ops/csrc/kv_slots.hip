// Slot bookkeeping of the continuous-batching GPT-2 engine (models/gpt2_engine.py): a
// persistent K/V cache of S slots that requests enter and leave independently, between
// replays of one captured decode step. Three entry points, all capturable: every index they
// use (slot id, length, output column) is read ON THE DEVICE and checked there before it
// addresses memory; a bad value skips the work and never writes outside a tensor.
//
// ra_kv_insert: the admission path. Moves one layer's K/V of a prefill into slots of a
// wider cache.
//
//   qkv [Bn, Tp, 3, H, 64]           the layer's c_attn output for the right-padded prompts
//   k_cache, v_cache [S, H, Tmax, 64]   as attn_decode.hip
//   slots, lens [Bn] int32
//
// For every row b with 0 <= slots[b] < S, t in [0, min(lens[b], Tp, Tmax)) and every h:
// k_cache[slots[b], h, t, :] = qkv[b, t, 1, h, :], the same for V with index 2. Nothing
// else is written. Layout as attn_decode.hip: a 128-byte row is 8 lanes x 16 B, and for a
// fixed (b, h) consecutive t are contiguous in the cache, so one wave-wide store writes
// 1 KiB; the reads are whole 128-byte segments at stride 3 * H * 128 B. Grid (ceil(n / 64),
// H, Bn) with n = min(Tp, Tmax); a workgroup owns 64 positions of one (b, h), K and V, and
// moves them with kv_rows.h's kv_move_rows (shared with ra_kv_copy and attn_extend.hip's
// append): four 16-byte loads per lane in flight before the first store; workgroups past
// lens[b] exit after reading it. No LDS.
//
// ra_kv_copy: the shared-prefix path. Copies cached rows from one cache to another, all
// layers, K and V, in one launch.
//
//   src_k, src_v [L, P, H, Tsrc, 64], dst_k, dst_v [L, S, H, Tdst, 64]
//   src_rows, dst_rows, lens [Bn] int32
//
// For every b with 0 <= src_rows[b] < P, 0 <= dst_rows[b] < S and 0 <= lens[b] <=
// min(Tsrc, Tdst), every layer l, head h and t < lens[b]:
// dst[l, dst_rows[b], h, t, :] = src[l, src_rows[b], h, t, :]; any other b is skipped and
// nothing else is written. Built as ra_kv_insert: grid (ceil(n / 64), L * H, Bn) with
// n = min(Tsrc, Tdst), a workgroup owns 64 positions of one (l, h, b), K and V, the same
// kv_move_rows (here both sides are 1 KiB contiguous per wave instruction), no LDS.
//
// ra_slot_advance: the per-token path, after the sampler, one thread per slot.
//
//   tok [S] int64, lens [S] int32 (the cache's), n_out, max_new [S] int32, active [S] uint8,
//   out [S, cap] int64, eos (-1: none)
//
// An active slot with 0 <= n_out[s] < cap stores out[s, n_out[s]] = tok[s], adds 1 to
// n_out[s] and becomes inactive if n_out[s] >= max_new[s] or tok[s] == eos; an active slot
// with any other n_out[s] becomes inactive without a write. Every slot that is inactive
// after that, the ones that already were included, gets lens[s] = kSlotInactive on every
// call: decode_step adds 1 to every lens each step, and the re-pin keeps an idle slot from
// ever walking back into [0, Tmax). A slot retired here is already inactive for the
// decode_step that follows.
#include "kv_rows.h"

namespace {

constexpr int kD = 64;
constexpr int kSlotInactive = -(1 << 30);

__global__ __launch_bounds__(kKvThreads) void kv_insert_kernel(
    const bf16_t* __restrict__ qkv, bf16_t* __restrict__ kc, bf16_t* __restrict__ vc,
    const int* __restrict__ slots, const int* __restrict__ lens, int Tp, int H, int S, int Tmax) {
  const int b = blockIdx.z, h = blockIdx.y;
  const int slot = slots[b];
  if (slot < 0 || slot >= S) return;
  const int len = min(lens[b], min(Tp, Tmax));  // real positions of both tensors
  const int t0 = blockIdx.x * kKvBlockRows;
  if (t0 >= len) return;
  const int c = threadIdx.x & 7;
  // qkv[b, 0, 1, h] (K; V is H * kD further) and the cache's [slot, h, 0]
  const bf16_t* src = qkv + ((long)b * Tp * 3 + 1) * H * kD + (long)h * kD + c * 8;
  const long dst0 = (((long)slot * H + h) * Tmax) * kD + c * 8;
  kv_move_rows(src, src + (long)H * kD, 3L * H * kD, kc + dst0, vc + dst0, t0, len);
}

__global__ __launch_bounds__(kKvThreads) void kv_copy_kernel(
    const bf16_t* __restrict__ sk, const bf16_t* __restrict__ sv, bf16_t* __restrict__ dk,
    bf16_t* __restrict__ dv, const int* __restrict__ src_rows, const int* __restrict__ dst_rows,
    const int* __restrict__ lens, int H, int P, int Tsrc, int S, int Tdst) {
  const int b = blockIdx.z, l = blockIdx.y / H, h = blockIdx.y % H;
  const int sr = src_rows[b], dr = dst_rows[b], len = lens[b];
  if (sr < 0 || sr >= P || dr < 0 || dr >= S || len < 0 || len > min(Tsrc, Tdst)) return;
  const int t0 = blockIdx.x * kKvBlockRows;
  if (t0 >= len) return;  // (len <= min(Tsrc, Tdst): real positions of both caches)
  const int c = threadIdx.x & 7;
  const long src0 = ((((long)l * P + sr) * H + h) * Tsrc) * kD + c * 8;
  const long dst0 = ((((long)l * S + dr) * H + h) * Tdst) * kD + c * 8;
  kv_move_rows(sk + src0, sv + src0, kD, dk + dst0, dv + dst0, t0, len);
}

__global__ __launch_bounds__(64) void slot_advance_kernel(
    const long* __restrict__ tok, int* __restrict__ lens, int* __restrict__ n_out,
    const int* __restrict__ max_new, unsigned char* __restrict__ active, long* __restrict__ out,
    int S, int cap, long eos) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  bool act = active[s] != 0;
  if (act) {
    const int n = n_out[s];
    if (n < 0 || n >= cap) {
      act = false;
    } else {
      const long t = tok[s];
      out[(long)s * cap + n] = t;
      n_out[s] = n + 1;
      if (n + 1 >= max_new[s] || (eos >= 0 && t == eos)) act = false;
    }
    if (!act) active[s] = 0;
  }
  if (!act) lens[s] = kSlotInactive;
}

}  // namespace

// qkv, k_cache, v_cache 16-byte aligned. Runs on the caller's stream; no host
// synchronisation, no allocation; slots and lens stay on the device and are only read.
RA_EXPORT int ra_kv_insert(const void* qkv, void* k_cache, void* v_cache, const int* slots,
                           const int* lens, int Bn, int Tp, int H, int S, int Tmax,
                           hipStream_t st) {
  if (Bn <= 0 || Tp <= 0 || H <= 0 || S <= 0 || Tmax <= 0 || Bn > 65535 || H > 65535 ||
      Tp > (1 << 22) || Tmax > (1 << 22))
    return hipErrorInvalidValue;
  if ((((uintptr_t)qkv | (uintptr_t)k_cache | (uintptr_t)v_cache) & 15) || slots == nullptr ||
      lens == nullptr)
    return hipErrorInvalidValue;
  const int n = Tp < Tmax ? Tp : Tmax;
  hipLaunchKernelGGL(kv_insert_kernel, dim3((n + kKvBlockRows - 1) / kKvBlockRows, H, Bn),
                     dim3(kKvThreads), 0, st, (const bf16_t*)qkv, (bf16_t*)k_cache,
                     (bf16_t*)v_cache, slots, lens, Tp, H, S, Tmax);
  return hipGetLastError();
}

// All four caches 16-byte aligned, src and dst distinct tensors. Runs on the caller's stream;
// no host synchronisation, no allocation; the three index vectors stay on the device and are
// only read.
RA_EXPORT int ra_kv_copy(const void* src_k, const void* src_v, void* dst_k, void* dst_v,
                         const int* src_rows, const int* dst_rows, const int* lens, int Bn, int L,
                         int H, int P, int Tsrc, int S, int Tdst, hipStream_t st) {
  if (Bn <= 0 || L <= 0 || H <= 0 || P <= 0 || S <= 0 || Tsrc <= 0 || Tdst <= 0 || Bn > 65535 ||
      (long)L * H > 65535 || Tsrc > (1 << 22) || Tdst > (1 << 22))
    return hipErrorInvalidValue;
  if ((((uintptr_t)src_k | (uintptr_t)src_v | (uintptr_t)dst_k | (uintptr_t)dst_v) & 15) ||
      src_rows == nullptr || dst_rows == nullptr || lens == nullptr)
    return hipErrorInvalidValue;
  const int n = Tsrc < Tdst ? Tsrc : Tdst;
  hipLaunchKernelGGL(kv_copy_kernel, dim3((n + kKvBlockRows - 1) / kKvBlockRows, L * H, Bn),
                     dim3(kKvThreads), 0, st, (const bf16_t*)src_k, (const bf16_t*)src_v,
                     (bf16_t*)dst_k, (bf16_t*)dst_v, src_rows, dst_rows, lens, H, P, Tsrc, S, Tdst);
  return hipGetLastError();
}

// eos < 0: none. Runs on the caller's stream; no host synchronisation, no allocation.
RA_EXPORT int ra_slot_advance(const long* tok, int* lens, int* n_out, const int* max_new,
                              unsigned char* active, long* out, int S, int cap, long eos,
                              hipStream_t st) {
  if (S <= 0 || cap <= 0 || tok == nullptr || lens == nullptr || n_out == nullptr ||
      max_new == nullptr || active == nullptr || out == nullptr)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(slot_advance_kernel, dim3((S + 63) / 64), dim3(64), 0, st, tok, lens, n_out,
                     max_new, active, out, S, cap, eos);
  return hipGetLastError();
}
