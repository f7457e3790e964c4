// Single-query (decode) attention over a growing K/V cache, head_dim 64, bf16, for
// autoregressive GPT-2 generation. One launch appends the new token's K/V to the cache
// and attends over the row's cached positions plus the new one.
//
//   qkv_new [B, 3, H, 64]     the c_attn output of the one new token (attn.hip's packing)
//   k_cache, v_cache [B, H, Tmax, 64]   each (b, h) one contiguous stream, any Tmax
//   lens [B] int32 ON THE DEVICE: cached positions of row b before this call
//   out [B, H, 64]
//
// A row with 0 <= lens[b] < Tmax writes k/v to position lens[b] and attends over
// 0..lens[b]; any other row is inactive (no cache write, zero output). lens is only read,
// in the kernel: no host read, so one captured launch serves every position. Positions
// past lens[b] are never LOADED (the cache there holds leftovers of right-padded prompts,
// possibly NaN), which is what masking means here.
//
// Memory-bound and launch-bound. Layout: a K (or V) row is 128 B = 8 lanes x 16 B, so one
// wave-wide 16-byte load covers 8 consecutive rows (1 KiB contiguous) and lane
// (g = lane >> 3, c = lane & 7) holds dims 8c..8c+7 of row g. K/V go global -> VGPR, no
// LDS staging; kU K loads and kU V loads are issued per lane before the first use. q
// (pre-multiplied by scale * log2 e) sits in registers, a score is 8 FMAs plus a 3-step
// shuffle over the 8 lanes of a row, and each 8-lane group keeps its own online softmax
// (running max / sum in the log2 domain, as attn.hip) and its own 8 output dims. Groups
// are merged by shuffles, the 4 waves of a workgroup through LDS.
//
// Split-KV: grid (S, H, B). Split s owns keys [s * chunk, (s + 1) * chunk) of the row's
// n = lens[b] + 1 keys, chunk = ceil(n / S) rounded up to 32. S == 1 writes `out`
// directly; S > 1 writes per-split (m, l, unnormalised O) in fp32 and a second kernel
// merges the S partials in index order. A split without keys has m = -inf, l = 0 and
// weight 0 in the merge (never exp2(-inf - -inf)). No float atomics in this file: the
// same inputs give the same bits every run. The split that owns position lens[b] takes
// that key from qkv_new (not from the cache it is writing) and does the append.
#include "common.h"

namespace {

constexpr int kD = 64;
constexpr int kWaves = 4;
constexpr int kThreads = kWaves * 64;
constexpr int kU = 4;                       // rows in flight per lane (x2: K and V)
constexpr int kWaveKeys = 8 * kU;           // 32 rows = 4 KiB per wave per step
constexpr int kBlockKeys = kWaves * kWaveKeys;
constexpr int kMaxSplits = 256;

struct DecodeArgs {
  const bf16_t* qkv;  // [B,3,H,64]
  bf16_t* kc;         // [B,H,Tmax,64]
  bf16_t* vc;
  const int* lens;    // [B]
  bf16_t* out;        // [B,H,64]
  float* part_o;      // [B*H,S,64]
  float* part_ml;     // [B*H,S,2]
  int H, Tmax, S;
  float sc_log2;
};

__device__ __forceinline__ float dexp2(float x) { return __builtin_amdgcn_exp2f(x); }

template <bool DIRECT>
__global__ __launch_bounds__(kThreads) void attn_decode_kernel(DecodeArgs a) {
  __shared__ float sm_o[kWaves][kD];
  __shared__ float sm_m[kWaves], sm_l[kWaves];
  const int s = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int g = lane >> 3, c = lane & 7;
  const int H = a.H, Tmax = a.Tmax;
  const int len = a.lens[b];
  const bool active = len >= 0 && len < Tmax;
  const int n = active ? len + 1 : 0;  // keys of this row, the new one included
  const int chunk = ((n + a.S - 1) / a.S + 31) & ~31;
  const int k0 = s * chunk;
  const int k1 = min(k0 + chunk, n);

  const bf16_t* qn = a.qkv + ((long)(b * 3) * H + h) * kD + c * 8;
  const bf16_t* kn = qn + (long)H * kD;
  const bf16_t* vn = kn + (long)H * kD;
  const long row0 = ((long)b * H + h) * Tmax;
  bf16_t* kc = a.kc + row0 * kD + c * 8;
  bf16_t* vc = a.vc + row0 * kD + c * 8;

  float q[8];
  unpack8(*reinterpret_cast<const uint4*>(qn), q);
#pragma unroll
  for (int i = 0; i < 8; ++i) q[i] *= a.sc_log2;

  float m = -INFINITY, l = 0.f, o[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = 0.f;

  // wave-uniform trip count; rows >= k1 are predicated off per 8-lane group
  for (int base = k0 + w * kWaveKeys; base < k1; base += kBlockKeys) {
    uint4 kk[kU], vv[kU];
    bool ok[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int key = base + u * 8 + g;
      ok[u] = key < k1;
      kk[u] = make_uint4(0, 0, 0, 0);
      vv[u] = make_uint4(0, 0, 0, 0);
      if (ok[u]) {
        const bool nw = key == len;
        kk[u] = *reinterpret_cast<const uint4*>(nw ? kn : kc + (long)key * kD);
        vv[u] = *reinterpret_cast<const uint4*>(nw ? vn : vc + (long)key * kD);
        if (nw) {  // the append: key == len < Tmax, and only the split that owns it
          *reinterpret_cast<uint4*>(kc + (long)key * kD) = kk[u];
          *reinterpret_cast<uint4*>(vc + (long)key * kD) = vv[u];
        }
      }
    }
    float sc[kU];
    float mt = -INFINITY;
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      float kf[8];
      unpack8(kk[u], kf);
      float d = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) d = fmaf(q[i], kf[i], d);
      d += __shfl_xor(d, 1, 64);
      d += __shfl_xor(d, 2, 64);
      d += __shfl_xor(d, 4, 64);
      sc[u] = ok[u] ? d : -INFINITY;
      mt = fmaxf(mt, sc[u]);
    }
    const float m_new = fmaxf(m, mt);
    const float ms = (m_new == -INFINITY) ? 0.f : m_new;  // a group with no key yet
    const float alpha = dexp2(m - ms);                    // m = -inf: 0, and o = l = 0
    l *= alpha;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] *= alpha;
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const float p = dexp2(sc[u] - ms);  // masked row: exp2(-inf) = 0, v = 0
      float vf[8];
      unpack8(vv[u], vf);
      l += p;
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = fmaf(p, vf[i], o[i]);
    }
    m = m_new;
  }

  // merge the 8 row groups of the wave (lanes with equal c)
  float M = m;
#pragma unroll
  for (int x = 8; x < 64; x <<= 1) M = fmaxf(M, __shfl_xor(M, x, 64));
  const float f = (m == -INFINITY) ? 0.f : dexp2(m - M);
  l *= f;
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] *= f;
#pragma unroll
  for (int x = 8; x < 64; x <<= 1) {
    l += __shfl_xor(l, x, 64);
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] += __shfl_xor(o[i], x, 64);
  }
  if (g == 0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) sm_o[w][c * 8 + i] = o[i];
    if (c == 0) {
      sm_m[w] = M;
      sm_l[w] = l;
    }
  }
  __syncthreads();
  // merge the waves in index order: thread d owns output dim d
  if (threadIdx.x < kD) {
    const int d = threadIdx.x;
    float Mb = sm_m[0];
#pragma unroll
    for (int i = 1; i < kWaves; ++i) Mb = fmaxf(Mb, sm_m[i]);
    float L = 0.f, O = 0.f;
#pragma unroll
    for (int i = 0; i < kWaves; ++i) {
      const float fi = (sm_m[i] == -INFINITY) ? 0.f : dexp2(sm_m[i] - Mb);
      L = fmaf(fi, sm_l[i], L);
      O = fmaf(fi, sm_o[i][d], O);
    }
    const long bh = (long)b * H + h;
    if (DIRECT) {
      a.out[bh * kD + d] = f2bf(L > 0.f ? O / L : 0.f);
    } else {
      const long ps = bh * a.S + s;
      a.part_o[ps * kD + d] = O;
      if (d == 0) {
        a.part_ml[ps * 2] = Mb;
        a.part_ml[ps * 2 + 1] = L;
      }
    }
  }
}

// out[bh] = sum_s w_s O_s / sum_s w_s l_s, w_s = exp2(m_s - max m): one 64-thread block
// per (b, h), thread d = output dim d, the splits added in index order.
__global__ __launch_bounds__(kD) void attn_decode_merge_kernel(const float* __restrict__ part_o,
                                                               const float* __restrict__ part_ml,
                                                               bf16_t* __restrict__ out, int S) {
  const long bh = blockIdx.x;
  const int d = threadIdx.x;
  const float* ml = part_ml + bh * S * 2;
  const float* po = part_o + bh * S * kD + d;
  float M = -INFINITY;
  for (int i = 0; i < S; ++i) M = fmaxf(M, ml[2 * i]);
  float L = 0.f, O = 0.f;
  for (int i = 0; i < S; ++i) {
    const float mi = ml[2 * i];
    const float fi = (mi == -INFINITY) ? 0.f : dexp2(mi - M);
    L = fmaf(fi, ml[2 * i + 1], L);
    O = fmaf(fi, po[(long)i * kD], O);
  }
  out[bh * kD + d] = f2bf(L > 0.f ? O / L : 0.f);
}

int g_cus_d = 0;

}  // namespace

// Split count for a [B, H] decode over caches of capacity Tmax: up to two workgroups per
// CU when B * H alone leaves the chip idle (B = 1, H = 12: 12 pairs for 256 CUs), never
// less than one full 128-row step per split. The row lengths live on the device, so the
// choice depends on the capacity only.
RA_EXPORT int ra_attn_decode_splits(int B, int H, int Tmax) {
  if (B <= 0 || H <= 0 || Tmax <= 0) return 1;
  if (g_cus_d == 0) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&g_cus_d, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        g_cus_d <= 0)
      g_cus_d = 256;
  }
  // (measured at H = 12, Tmax = 1024, device time per call in us, profiles/r8/gpt2_decode.md:
  // B = 1: S 1/2/4/8/16/32 = 8.9/8.1/7.2/7.1/9.8/15.0; B = 8: 10.1/9.4/7.9/9.0/12.8/19.0, and
  // S = 6, whose 192-row chunks are no multiple of the 128-row step, 9.7; B = 64: S = 1
  // best. So: the largest power of two with B * H * S <= 2 * CUs and Tmax / S >= 128.)
  const long pairs = (long)B * H;
  const long cap = (Tmax + kBlockKeys - 1) / kBlockKeys;
  long S = 1;
  while (S < 64 && 2 * S <= cap && pairs * 2 * S <= 2L * g_cus_d) S *= 2;
  return (int)S;
}

namespace {
inline int resolve_splits(int B, int H, int Tmax, int splits) {
  return splits > 0 ? splits : ra_attn_decode_splits(B, H, Tmax);
}
}  // namespace

// fp32 elements of workspace that ra_attn_decode needs for this splits argument
// (0 = automatic); 0 when one split writes the output directly.
RA_EXPORT long ra_attn_decode_work(int B, int H, int Tmax, int splits) {
  if (B <= 0 || H <= 0 || Tmax <= 0 || splits < 0 || splits > kMaxSplits) return 0;
  const int S = resolve_splits(B, H, Tmax, splits);
  return S > 1 ? (long)B * H * S * (kD + 2) : 0;
}

// splits: 0 = ra_attn_decode_splits(B, H, Tmax), else the explicit count (<= 256). ws:
// ra_attn_decode_work floats (may be null when that is 0). All pointers 16-byte aligned.
// Runs on the caller's stream; no host synchronisation, no allocation, lens stays on the
// device and is not modified.
RA_EXPORT int ra_attn_decode(const void* qkv_new, void* k_cache, void* v_cache, const int* lens,
                             void* out, float* ws, int B, int H, int Tmax, float scale,
                             int splits, hipStream_t st) {
  if (B <= 0 || H <= 0 || Tmax <= 0 || B > 65535 || H > 65535 || Tmax > (1 << 22) ||
      splits < 0 || splits > kMaxSplits)
    return hipErrorInvalidValue;
  if ((((uintptr_t)qkv_new | (uintptr_t)k_cache | (uintptr_t)v_cache | (uintptr_t)out) & 15) ||
      lens == nullptr)
    return hipErrorInvalidValue;
  const int S = resolve_splits(B, H, Tmax, splits);
  if (S > 1 && ws == nullptr) return hipErrorInvalidValue;
  DecodeArgs a;
  a.qkv = (const bf16_t*)qkv_new;
  a.kc = (bf16_t*)k_cache;
  a.vc = (bf16_t*)v_cache;
  a.lens = lens;
  a.out = (bf16_t*)out;
  a.part_o = ws;
  a.part_ml = ws ? ws + (long)B * H * S * kD : nullptr;
  a.H = H;
  a.Tmax = Tmax;
  a.S = S;
  a.sc_log2 = scale * 1.4426950408889634f;
  if (S == 1) {
    hipLaunchKernelGGL(attn_decode_kernel<true>, dim3(1, H, B), dim3(kThreads), 0, st, a);
  } else {
    hipLaunchKernelGGL(attn_decode_kernel<false>, dim3(S, H, B), dim3(kThreads), 0, st, a);
    hipLaunchKernelGGL(attn_decode_merge_kernel, dim3(B * H), dim3(kD), 0, st, a.part_o,
                       a.part_ml, a.out, S);
  }
  return hipGetLastError();
}
