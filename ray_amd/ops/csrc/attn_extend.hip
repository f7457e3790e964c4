// Multi-query ("extend") attention over a K/V cache, head_dim 64, bf16: several new tokens
// for rows that already hold cached positions. The operation behind shared prompt prefixes
// and chunked prefill in the GPT-2 engine (models/gpt2_engine.py).
//
//   qkv_new [Bn, Tn, 3, H, 64]          packed c_attn output of the new tokens, right-padded
//   k_cache, v_cache [S, H, Tmax, 64]   as attn_decode.hip / kv_slots.hip, written in place
//   slots, base, n_new [Bn] int32 ON THE DEVICE
//   out [Bn, Tn, H, 64]                 (= the proj GEMM's input, as attn.hip writes it)
//
// A row is active when 0 <= slots[b] < S, base[b] >= 0, 1 <= n_new[b] <= Tn and
// base[b] + n_new[b] <= Tmax. An active row appends its n_new K/V rows at positions
// base .. base + n_new - 1 of cache row slots[b] (bitwise), and query i < n_new attends over
// keys 0 .. base + i; out rows i >= n_new are zero. An inactive row writes nothing to the
// caches and gets zero output. Everything is read and bounds-checked on the device: no host
// read, capturable. Slots are distinct among the active rows (the caller's contract).
//
// Two launches on one stream (the UNFUSED form): kv_append_kernel, which is kv_slots.hip's
// kv_insert_kernel with a per-row position offset (both move their rows with kv_rows.h's
// kv_move_rows), then attn_extend_kernel, which reads every
// key, old and new, from the cache. So the tile loop has ONE K/V source, and no workgroup
// reads a cache position that another workgroup of its own launch is writing. (Fused, the
// new keys would have to come from qkv_new, at another row stride, in every tile past
// `base`: a second addressing mode in the hot loop to save one ~2 us launch.)
//
// attn_extend_kernel is the forward of attn.hip on another address map, and runs the same
// tile body (attn_mfma.h's fwd_tile, so the two cannot drift apart): S^T = K.Q^T with
// v_mfma_f32_32x32x16_bf16, so a lane owns one query and the online softmax is lane-local in
// the log2 domain (lazy rescaling included); P^T's accumulators are the B operand of
// O^T = V^T.P^T; K/V tiles of 64 keys in the swizzled LDS image, double buffered, two tiles
// of loads in flight; O leaves whole-row through LDS. The helpers are attn_mfma.h's.
// Grid (ceil(Tn / 128), H, Bn), 4 waves x 32 queries. What differs from attn.hip:
//   * the (b, h) K/V stream k_cache[slot, h] is contiguous (128-byte rows), tiles are plain
//     row tiles of it;
//   * the causal boundary key <= base + i is not tile aligned: tiles that reach past
//     base + (the wave's first query) take a per-element compare-and-SELECT, the tiles below
//     it no mask at all;
//   * cache rows at or past base + n_new hold leftovers (NaN included) and the stream ends
//     at Tmax rows: every tile load clamps its row index to the row's last valid position
//     base + n_new - 1, so neither a NaN nor an address past the stream ever exists; the
//     clamped duplicates lie above every query's boundary and are masked by the same compare;
//   * Tn and n_new are arbitrary: a padding lane repeats the row's last real query (Q rows
//     at or past n_new are never loaded) and stores zeros; O rows at or past Tn are never
//     stored; waves and workgroups without a real query only store zeros.
// The keys of a query are summed in an order that depends on its own position, base and
// n_new only (64-key tiles from key 0; the wave-wide rescale vote is over queries of the same
// row), never on Bn, Tn, the slot id or the other rows: a row's output bits do not depend on
// its batch-mates. No key split, no float atomics.
//
// Measured (scripts/gpt2_prefix_bench.py, profiles/r11/prefix.md; H = 12, Tmax = 1024, device
// time per call of both launches, (Bn, base, n_new)): (1, 512, 32) 13.1 us, (8, 512, 32)
// 13.1 us, (8, 0, 512) 26.0 us, (1, 896, 128) 20.6 us, 4.3-7.1x the torch composition. Per
// K/V byte the short suffixes are not behind the long ones (1020 GB/s at (8, 512, 32) against
// 484 at (8, 0, 512); 128 at (1, 512, 32) against 153 at (1, 896, 128)): what costs is
// Bn = 1, twelve workgroups each walking its tiles alone. So a 32- or 64-query block with
// the waves splitting the keys and merging through LDS was not built.
#include "attn_mfma.h"
#include "kv_rows.h"

#include <type_traits>

namespace {

constexpr int kD = 64;
constexpr int kTile = 64 * 64;  // elements of one [64 keys][64] LDS image
constexpr int kQBlk = 128;      // queries per workgroup: 4 waves x 32

// ---------------------------------------------------------------- the row's device-side check
struct ExtendRow {
  int slot, base, n;  // n = 0: inactive
};
__device__ __forceinline__ ExtendRow extend_row(const int* slots, const int* base,
                                                const int* n_new, int b, int S, int Tn, int Tmax) {
  ExtendRow r{slots[b], base[b], n_new[b]};
  // (base <= Tmax - n: no overflow, whatever the three hold)
  const bool ok = r.slot >= 0 && r.slot < S && r.base >= 0 && r.n >= 1 && r.n <= Tn &&
                  r.base <= Tmax - r.n;
  if (!ok) r.n = 0;
  return r;
}

// ---------------------------------------------------------------- append
// kv_slots.hip's kv_insert_kernel with the destination shifted by base[b]: a workgroup owns
// 64 new positions of one (b, h), K and V, and moves them with kv_rows.h's kv_move_rows.
__global__ __launch_bounds__(kKvThreads) void kv_append_kernel(
    const bf16_t* __restrict__ qkv, bf16_t* __restrict__ kc, bf16_t* __restrict__ vc,
    const int* __restrict__ slots, const int* __restrict__ base, const int* __restrict__ n_new,
    int Tn, int H, int S, int Tmax) {
  const int b = blockIdx.z, h = blockIdx.y;
  const ExtendRow row = extend_row(slots, base, n_new, b, S, Tn, Tmax);
  const int t0 = blockIdx.x * kKvBlockRows;
  if (t0 >= row.n) return;  // (n <= Tn and base + n <= Tmax: real positions of both tensors)
  const int c = threadIdx.x & 7;
  const bf16_t* src = qkv + ((long)b * Tn * 3 + 1) * H * kD + (long)h * kD + c * 8;
  const long dst0 = (((long)row.slot * H + h) * Tmax + row.base) * kD + c * 8;
  kv_move_rows(src, src + (long)H * kD, 3L * H * kD, kc + dst0, vc + dst0, t0, row.n);
}

// ---------------------------------------------------------------- attention
// zero rows [i0, i1) of one (b, h) of `out` (ob: row 0, row stride C), by `nthr` threads
__device__ __forceinline__ void zero_rows(bf16_t* ob, int i0, int i1, int C, int tid, int nthr) {
  for (int i = i0 + (tid >> 3); i < i1; i += nthr >> 3)
    *reinterpret_cast<u32x4*>(ob + (long)i * C + (tid & 7) * 8) = u32x4{0, 0, 0, 0};
}

__global__ __launch_bounds__(256) void attn_extend_kernel(
    const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ kc, const bf16_t* __restrict__ vc,
    const int* __restrict__ slots, const int* __restrict__ base, const int* __restrict__ n_new,
    bf16_t* __restrict__ out, int Tn, int H, int S, int Tmax, float sc_log2) {
  __shared__ __attribute__((aligned(16))) bf16_t lds[2 * 2 * kTile];  // [buf][K, V]
  const int qb = gridDim.x - 1 - blockIdx.x;  // the block with the most keys first
  const int h = blockIdx.y, b = blockIdx.z;
  const int C = H * kD;
  const int q0 = qb * kQBlk;
  const ExtendRow row = extend_row(slots, base, n_new, b, S, Tn, Tmax);
  bf16_t* ob = out + (long)b * Tn * C + h * kD;  // out[b, 0, h]; query i at ob + i * C
  if (q0 >= row.n) {  // no real query here (an inactive row: every block)
    zero_rows(ob, q0, min(q0 + kQBlk, Tn), C, threadIdx.x, 256);
    return;
  }
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, hh = lane >> 5;
  const LaneOffs lo(lane);
  const int last = row.base + row.n - 1;                    // the row's last valid cache position
  const int nkeys = row.base + min(q0 + kQBlk, row.n);      // keys 0 .. nkeys-1 serve this block
  const int ntiles = (nkeys + 63) >> 6;
  const int wave_q = q0 + 32 * w;
  const bool live = wave_q < row.n;                         // wave-uniform: it has a real query
  const int qi = min(wave_q + r, row.n - 1);                // padding lanes repeat the last one
  const int qpos = row.base + qi;                           // this lane attends over 0 .. qpos
  const int wave_pmin = row.base + wave_q;
  const int wave_pmax = row.base + min(wave_q + 31, row.n - 1);

  bf16x8_t qf[4];
  if (live) {
    const bf16_t* qp = qkv + (((long)b * Tn + qi) * 3) * C + h * kD + 8 * hh;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) qf[kk] = ld8(qp + 16 * kk);
  } else {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) qf[kk] = bf16x8_t{};
  }
  f32x16 o[2] = {f32x16{}, f32x16{}};
  float m_run = -INFINITY, l_run = 0.f;

  // The (slot, h) stream: rows 0 .. last are valid and finite. The resource ends there as
  // well; the clamp below already keeps every offset inside it.
  const long stream = ((long)row.slot * H + h) * Tmax * kD;
  const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(kc + stream), 0, (last + 1) * kD * 2, 0x00020000);
  const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(vc + stream), 0, (last + 1) * kD * 2, 0x00020000);
  const int trow = threadIdx.x >> 3, tcol = (threadIdx.x & 7) * 16;
  auto load_kv = [&](KV& x, int t) __attribute__((always_inline)) {
    const int o0 = min(t * 64 + trow, last) * (kD * 2) + tcol;
    const int o1 = min(t * 64 + 32 + trow, last) * (kD * 2) + tcol;
    x.k.v0 = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rk, o0, 0, 0));
    x.k.v1 = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rk, o1, 0, 0));
    x.v.v0 = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rv, o0, 0, 0));
    x.v.v1 = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rv, o1, 0, 0));
  };
  auto store_kv = [&](const KV& x, int t) __attribute__((always_inline)) {
    bf16_t* d = lds + (t & 1) * 2 * kTile;
    tile_store(x.k, d);
    tile_store(x.v, d + kTile);
  };
  // The diagonal tiles mask keys > qpos, the clamped duplicates included. Unlike attn.hip, a
  // lane's tile can be masked whole (its qpos below the tile, a later query of the wave
  // inside it): in fwd_tile's lazy rescaling mt = -inf, m_new = m_run, alpha = 1, p = 0.
  // Tile 0 holds key 0 for every lane, so m_run is finite from then on.
  auto body = [&](int t, auto diag_c) __attribute__((always_inline)) {
    const bf16_t* Ks = lds + (t & 1) * 2 * kTile;
    fwd_tile<decltype(diag_c)::value>(Ks, Ks + kTile, lo, qf, t * 64, qpos, hh, sc_log2, o,
                                      m_run, l_run);
  };
  auto compute = [&](int t) __attribute__((always_inline)) {
    const int kv0 = t * 64;
    if (live && kv0 <= wave_pmax) {
      if (kv0 + 63 > wave_pmin) body(t, std::true_type{});
      else body(t, std::false_type{});
    }
  };
  // 2-deep register prefetch: tile t+2's loads are in flight during tiles t and t+1
  auto step = [&](int t, KV& held, KV& next) __attribute__((always_inline)) {
    if (t + 2 < ntiles) load_kv(next, t + 2);
    compute(t);
    if (t + 1 < ntiles) store_kv(held, t + 1);
    __syncthreads();
  };
  KV A, B;
  load_kv(A, 0);
  load_kv(B, 1);  // ntiles == 1: rows clamped to `last`, loaded and never used
  store_kv(A, 0);
  kv_move(A, B);
  __syncthreads();
  for (int t = 0; t < ntiles; t += 2) {
    step(t, A, B);
    if (t + 1 < ntiles) step(t + 1, B, A);
  }
  // Every wave is past the last tile's barrier: the images are dead, O leaves through
  // wave-private regions of them, 8 whole 128-byte rows per store instruction.
  const int nrows = min(32, Tn - wave_q);  // rows of this wave that exist in `out`
  if (!live) {
    zero_rows(ob, wave_q, wave_q + max(nrows, 0), C, lane, 64);
    return;
  }
  bf16_t* img = lds + w * 2048;
  const bool real = wave_q + r < row.n;
  const float inv = 1.f / l_run;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = real ? o[dt][4 * g + j] * inv : 0.f;
      *reinterpret_cast<uint2*>(img + img_off(r, 4 * dt + g) + 4 * hh) = pack4(v);
    }
  wave_lds_order();
  bf16_t* g0 = ob + (long)wave_q * C;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int orow = 8 * s + (lane >> 3), ch = lane & 7;
    if (orow < nrows)
      *reinterpret_cast<u32x4*>(g0 + (long)orow * C + ch * 8) =
          *reinterpret_cast<const u32x4*>(img + img_off(orow, ch));
  }
}

}  // namespace

// qkv_new, k_cache, v_cache, out 16-byte aligned; scale > 0. Runs on the caller's stream: the
// append launch, then the attention launch; no host synchronisation, no allocation; slots,
// base and n_new stay on the device and are only read.
RA_EXPORT int ra_attn_extend(const void* qkv_new, void* k_cache, void* v_cache, const int* slots,
                             const int* base, const int* n_new, void* out, int Bn, int Tn, int H,
                             int S, int Tmax, float scale, hipStream_t st) {
  if (Bn <= 0 || Tn <= 0 || H <= 0 || S <= 0 || Tmax <= 0 || Bn > 65535 || H > 65535 ||
      Tn > (1 << 22) || Tmax > (1 << 22) || !(scale > 0.f))
    return hipErrorInvalidValue;
  if ((((uintptr_t)qkv_new | (uintptr_t)k_cache | (uintptr_t)v_cache | (uintptr_t)out) & 15) ||
      slots == nullptr || base == nullptr || n_new == nullptr)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(kv_append_kernel, dim3((Tn + kKvBlockRows - 1) / kKvBlockRows, H, Bn),
                     dim3(kKvThreads), 0, st, (const bf16_t*)qkv_new, (bf16_t*)k_cache,
                     (bf16_t*)v_cache, slots, base, n_new, Tn, H, S, Tmax);
  hipLaunchKernelGGL(attn_extend_kernel, dim3((Tn + kQBlk - 1) / kQBlk, H, Bn), dim3(256), 0, st,
                     (const bf16_t*)qkv_new, (const bf16_t*)k_cache, (const bf16_t*)v_cache, slots,
                     base, n_new, (bf16_t*)out, Tn, H, S, Tmax, scale * 1.4426950408889634f);
  return hipGetLastError();
}
