// Decode attention and the prefill insert over an INT8 K/V cache, head_dim 64: every
// 64-element K or V vector of one (row, head, position) is stored as 64 int8 values and one
// fp32 scale, 68 bytes where the bf16 cache of attn_decode.hip / kv_slots.hip takes 128.
//
//   k_cache, v_cache [B, H, Tmax, 64] int8;  k_scale, v_scale [B, H, Tmax] fp32
//
// The quantiser (ops/reference.py quantize_kv, bit for bit), in fp32:
//   s = absmax(x) / 127,  q = clamp(rint(x / (s > 0 ? s : 1)), -127, 127)
// Both quotients are IEEE divisions (__fdiv_rn: v_div_scale / v_div_fmas / v_div_fixup in the
// ISA, no bare v_rcp), rint rounds half to even, and contraction is off for the whole file
// (the attention's multiply-adds are explicit fmaf). A dequantised element is float(q) * s.
//
// ra_attn_decode_q8: attn_decode.hip's design re-derived for 64-byte rows.
//
//   qkv_new [B, 3, H, 64] bf16, lens [B] int32 ON THE DEVICE, out [B, H, 64] bf16
//
// A row with 0 <= lens[b] < Tmax quantises the new token's K and V, writes (q, s) at position
// lens[b] and attends over the dequantised positions 0..lens[b], the new one with its own
// dequantised values: the result is a function of the cache contents alone. Any other row is
// inactive (no write, zero output). Positions past lens[b] are never LOADED, neither their
// bytes nor their scales.
//
// Layout: a row is 4 lanes x 16 B, so one wave-wide 16-byte load covers 16 consecutive rows
// (1 KiB contiguous) and lane (g = lane >> 2, c = lane & 3) holds dims 16c..16c+15 of row g.
// K, V and their scales go global -> VGPR, no LDS staging: kU K loads, kU V loads and 2 kU
// scale loads are issued per lane before the first use, with no branch between them (a lane
// past the end loads the last valid row again and its score is set to -inf). A workgroup step
// is kU x 64 rows; load u of wave w covers rows base + 64 u + 16 w .., so the four waves
// share any chunk evenly. int8 -> fp32 is converted in registers and is exact. q
// (pre-multiplied by scale * log2 e) sits in registers; a score is 16 FMAs on the raw int8
// values, one multiply by k_scale and a 2-step shuffle over the row's 4 lanes; p * v_scale
// is one factor in front of the 16 output FMAs. Each 4-lane group keeps its own online
// softmax in the log2 domain and its own 16 output dims; groups merge by shuffles, the 4
// waves through LDS in wave order.
//
// Split-KV as attn_decode.hip: grid (S, H, B), S from ra_attn_decode_splits (unchanged),
// split s owns keys [s * chunk, (s + 1) * chunk) of the row's lens[b] + 1 keys, chunk =
// ceil(n / S) rounded up to 64. S == 1 writes `out`; S > 1 writes fp32 (m, l, O) per split
// and a second kernel merges them in index order. No float atomics: the same inputs give the
// same bits, and a row's bits depend on its own data and S only. The split that owns
// position lens[b] does the append after its loop over the cached rows: the 4 lanes of group
// 0 of wave 0 take the absmax of the new vector by shuffles, quantise it, store 16 B each
// and the scale, and add the key to their softmax from the quantised registers.
//
// ra_kv_insert_q8: ra_kv_insert (kv_slots.hip) with the quantiser in the middle.
//
//   qkv [Bn, Tp, 3, H, 64] bf16, caches and scales as above with S rows, slots, lens [Bn]
//
// For every row b with 0 <= slots[b] < S, t in [0, min(lens[b], Tp, Tmax)) and every h, the
// K vector qkv[b, t, 1, h] is quantised into k_cache / k_scale [slots[b], h, t] and V (index
// 2) likewise; nothing else is written. Grid (ceil(n / 64), H, Bn), a workgroup owns 64
// positions of one (b, h), K and V; a bf16 vector is 8 lanes x 16 B, four 16-byte loads per
// lane are in flight before the first use, the absmax goes over the 8 lanes by shuffles, a
// lane's 8 result bytes are merged with its neighbour's by a shuffle so that the even lanes
// store 16 B, and lane 0 of the vector stores the scale. No branch before the stores: a lane
// past the row's end redoes position len - 1, the same bytes that position's own lanes
// write. No LDS.
//
// Resources (gfx950, -O3, -Rpass-analysis=kernel-resource-usage) and measurements:
// profiles/r22/kv_q8.md.
#include "common.h"

#pragma clang fp contract(off)

extern "C" int ra_attn_decode_splits(int B, int H, int Tmax);  // attn_decode.hip

namespace {

constexpr int kD = 64;
constexpr int kWaves = 4;
constexpr int kThreads = kWaves * 64;
constexpr int kU = 4;                          // rows in flight per lane (x2: K and V)
constexpr int kLoadKeys = 16;                  // rows of one wave-wide 16-byte load
constexpr int kStepKeys = kWaves * kLoadKeys;  // rows of one load index across the workgroup
constexpr int kBlockKeys = kU * kStepKeys;     // 256 rows = 16 KiB of K per workgroup step
constexpr int kMaxSplits = 256;

struct DecodeQ8Args {
  const bf16_t* qkv;  // [B,3,H,64]
  int8_t* kc;         // [B,H,Tmax,64]
  int8_t* vc;
  float* ksc;         // [B,H,Tmax]
  float* vsc;
  const int* lens;    // [B]
  bf16_t* out;        // [B,H,64]
  float* part_o;      // [B*H,S,64]
  float* part_ml;     // [B*H,S,2]
  int H, Tmax, S;
  float sc_log2;
};

__device__ __forceinline__ float dexp2(float x) { return __builtin_amdgcn_exp2f(x); }

// The quantiser on N elements of a vector whose absmax over all its lanes is `amax`:
// returns the scale, qf gets the quantised values (integers in [-127, 127], as floats).
template <int N>
__device__ __forceinline__ float quantize(const float (&x)[N], float amax, float (&qf)[N]) {
  const float s = __fdiv_rn(amax, 127.f);
  const float safe = s > 0.f ? s : 1.f;
#pragma unroll
  for (int i = 0; i < N; ++i)
    qf[i] = fminf(fmaxf(rintf(__fdiv_rn(x[i], safe)), -127.f), 127.f);
  return s;
}

// four quantised values -> four int8 in one dword, element 0 in the low byte
__device__ __forceinline__ uint32_t pack_q4(const float* f) {
  return ((uint32_t)(int)f[0] & 0xffu) | (((uint32_t)(int)f[1] & 0xffu) << 8) |
         (((uint32_t)(int)f[2] & 0xffu) << 16) | ((uint32_t)(int)f[3] << 24);
}

// 16 consecutive int8 -> fp32, exact
__device__ __forceinline__ void cvt16(uint4 v, float (&f)[16]) {
  const int w[4] = {(int)v.x, (int)v.y, (int)v.z, (int)v.w};
#pragma unroll
  for (int d = 0; d < 4; ++d) {
#pragma unroll
    for (int j = 0; j < 4; ++j) f[4 * d + j] = (float)(int8_t)(w[d] >> (8 * j));
  }
}

__device__ __forceinline__ void unpack16(const bf16_t* p, float (&f)[16]) {
  float lo[8], hi[8];
  unpack8(*reinterpret_cast<const uint4*>(p), lo);
  unpack8(*reinterpret_cast<const uint4*>(p + 8), hi);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    f[i] = lo[i];
    f[8 + i] = hi[i];
  }
}

template <bool DIRECT>
__global__ __launch_bounds__(kThreads) void attn_decode_q8_kernel(DecodeQ8Args a) {
  __shared__ float sm_o[kWaves][kD];
  __shared__ float sm_m[kWaves], sm_l[kWaves];
  const int s = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int g = lane >> 2, c = lane & 3;
  const int H = a.H, Tmax = a.Tmax;
  const int len = a.lens[b];
  const bool active = len >= 0 && len < Tmax;
  const int n = active ? len + 1 : 0;  // keys of this row, the new one included
  const int chunk = ((n + a.S - 1) / a.S + kStepKeys - 1) & ~(kStepKeys - 1);
  const int k0 = s * chunk;
  const int kend = min(k0 + chunk, n - 1);  // the cached keys of this split: [k0, kend)

  const bf16_t* qn = a.qkv + ((long)(b * 3) * H + h) * kD + c * 16;
  const long row0 = ((long)b * H + h) * Tmax;
  const int8_t* kc = a.kc + row0 * kD + c * 16;
  const int8_t* vc = a.vc + row0 * kD + c * 16;
  const float* ksc = a.ksc + row0;
  const float* vsc = a.vsc + row0;

  float q[16];
  unpack16(qn, q);
#pragma unroll
  for (int i = 0; i < 16; ++i) q[i] *= a.sc_log2;

  float m = -INFINITY, l = 0.f, o[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) o[i] = 0.f;

  // block-uniform trip count; a row >= kend reloads row kend - 1 and scores -inf
  for (int base = k0; base < kend; base += kBlockKeys) {
    uint4 kk[kU], vv[kU];
    float ks[kU], vs[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int key = min(base + u * kStepKeys + w * kLoadKeys + g, kend - 1);
      kk[u] = *reinterpret_cast<const uint4*>(kc + (long)key * kD);
      vv[u] = *reinterpret_cast<const uint4*>(vc + (long)key * kD);
      ks[u] = ksc[key];
      vs[u] = vsc[key];
    }
    float sc[kU];
    float mt = -INFINITY;
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      float kf[16];
      cvt16(kk[u], kf);
      float d = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) d = fmaf(q[i], kf[i], d);
      d += __shfl_xor(d, 1, 64);
      d += __shfl_xor(d, 2, 64);
      const bool ok = base + u * kStepKeys + w * kLoadKeys + g < kend;
      sc[u] = ok ? d * ks[u] : -INFINITY;
      mt = fmaxf(mt, sc[u]);
    }
    const float m_new = fmaxf(m, mt);
    const float ms = (m_new == -INFINITY) ? 0.f : m_new;  // a group with no key yet
    const float alpha = dexp2(m - ms);                    // m = -inf: 0, and o = l = 0
    l *= alpha;
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] *= alpha;
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const float p = dexp2(sc[u] - ms);  // masked row: exp2(-inf) = 0
      const float pv = p * vs[u];
      float vf[16];
      cvt16(vv[u], vf);
      l += p;
#pragma unroll
      for (int i = 0; i < 16; ++i) o[i] = fmaf(pv, vf[i], o[i]);
    }
    m = m_new;
  }

  // the append (wave-uniform branch): len < Tmax, and only the split that owns key len. All
  // 16 groups of wave 0 quantise the same vector; group 0 stores it and attends to it.
  if (w == 0 && active && len >= k0 && len < k0 + chunk) {
    float x[16], kq[16], vq[16];
    unpack16(qn + (long)H * kD, x);
    float ka = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) ka = fmaxf(ka, fabsf(x[i]));
    ka = fmaxf(ka, __shfl_xor(ka, 1, 64));
    ka = fmaxf(ka, __shfl_xor(ka, 2, 64));
    const float ksn = quantize(x, ka, kq);
    unpack16(qn + 2L * H * kD, x);
    float va = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) va = fmaxf(va, fabsf(x[i]));
    va = fmaxf(va, __shfl_xor(va, 1, 64));
    va = fmaxf(va, __shfl_xor(va, 2, 64));
    const float vsn = quantize(x, va, vq);
    if (g == 0) {
      const long at = (row0 + len) * kD + c * 16;
      *reinterpret_cast<uint4*>(a.kc + at) =
          make_uint4(pack_q4(kq), pack_q4(kq + 4), pack_q4(kq + 8), pack_q4(kq + 12));
      *reinterpret_cast<uint4*>(a.vc + at) =
          make_uint4(pack_q4(vq), pack_q4(vq + 4), pack_q4(vq + 8), pack_q4(vq + 12));
      if (c == 0) {
        a.ksc[row0 + len] = ksn;
        a.vsc[row0 + len] = vsn;
      }
    }
    float d = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) d = fmaf(q[i], kq[i], d);
    d += __shfl_xor(d, 1, 64);
    d += __shfl_xor(d, 2, 64);
    const float sn = g == 0 ? d * ksn : -INFINITY;
    const float m_new = fmaxf(m, sn);
    const float ms = (m_new == -INFINITY) ? 0.f : m_new;
    const float alpha = dexp2(m - ms);
    const float p = dexp2(sn - ms);
    const float pv = p * vsn;
    l = fmaf(l, alpha, p);
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] = fmaf(pv, vq[i], o[i] * alpha);
    m = m_new;
  }

  // merge the 16 row groups of the wave (lanes with equal c)
  float M = m;
#pragma unroll
  for (int x = 4; x < 64; x <<= 1) M = fmaxf(M, __shfl_xor(M, x, 64));
  const float f = (m == -INFINITY) ? 0.f : dexp2(m - M);
  l *= f;
#pragma unroll
  for (int i = 0; i < 16; ++i) o[i] *= f;
#pragma unroll
  for (int x = 4; x < 64; x <<= 1) {
    l += __shfl_xor(l, x, 64);
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] += __shfl_xor(o[i], x, 64);
  }
  if (g == 0) {
#pragma unroll
    for (int i = 0; i < 16; ++i) sm_o[w][c * 16 + i] = o[i];
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
      a.out[bh * kD + d] = f2bf(L > 0.f ? __fdiv_rn(O, L) : 0.f);
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

// attn_decode.hip's merge: out[bh] = sum_s w_s O_s / sum_s w_s l_s, w_s = exp2(m_s - max m),
// one 64-thread block per (b, h), thread d = output dim d, the splits added in index order.
__global__ __launch_bounds__(kD) void attn_decode_q8_merge_kernel(
    const float* __restrict__ part_o, const float* __restrict__ part_ml, bf16_t* __restrict__ out,
    int S) {
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
  out[bh * kD + d] = f2bf(L > 0.f ? __fdiv_rn(O, L) : 0.f);
}

constexpr int kInsThreads = 256;
constexpr int kInsRowsPerPass = kInsThreads / 8;  // 32 positions: one 16-byte lane chunk each
constexpr int kInsPasses = 2;
constexpr int kInsBlockRows = kInsRowsPerPass * kInsPasses;

// One bf16 vector (8 lanes x 8 elements, this lane's in `raw`) -> its int8 row at `dst`
// (this vector's 64 bytes) and its scale at `sdst`; c = the lane's index in the vector.
__device__ __forceinline__ void quantize_store(uint4 raw, int c, int8_t* dst, float* sdst) {
  float x[8], qf[8];
  unpack8(raw, x);
  float am = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) am = fmaxf(am, fabsf(x[i]));
  am = fmaxf(am, __shfl_xor(am, 1, 64));
  am = fmaxf(am, __shfl_xor(am, 2, 64));
  am = fmaxf(am, __shfl_xor(am, 4, 64));
  const float s = quantize(x, am, qf);
  const uint32_t lo = pack_q4(qf), hi = pack_q4(qf + 4);
  const uint32_t nlo = __shfl_xor(lo, 1, 64), nhi = __shfl_xor(hi, 1, 64);
  if ((c & 1) == 0) *reinterpret_cast<uint4*>(dst + c * 8) = make_uint4(lo, hi, nlo, nhi);
  if (c == 0) *sdst = s;
}

__global__ __launch_bounds__(kInsThreads) void kv_insert_q8_kernel(
    const bf16_t* __restrict__ qkv, int8_t* __restrict__ kc, int8_t* __restrict__ vc,
    float* __restrict__ ksc, float* __restrict__ vsc, const int* __restrict__ slots,
    const int* __restrict__ lens, int Tp, int H, int S, int Tmax) {
  const int b = blockIdx.z, h = blockIdx.y;
  const int slot = slots[b];
  if (slot < 0 || slot >= S) return;
  const int len = min(lens[b], min(Tp, Tmax));  // real positions of both tensors
  const int t0 = blockIdx.x * kInsBlockRows;
  if (t0 >= len) return;
  const int c = threadIdx.x & 7, r = threadIdx.x >> 3;
  // qkv[b, 0, 1, h] (K; V is H * kD further) and the cache's [slot, h, 0]
  const bf16_t* src = qkv + ((long)b * Tp * 3 + 1) * H * kD + (long)h * kD + c * 8;
  const long row0 = ((long)slot * H + h) * Tmax;
  uint4 kk[kInsPasses], vv[kInsPasses];
#pragma unroll
  for (int u = 0; u < kInsPasses; ++u) {
    const int t = min(t0 + u * kInsRowsPerPass + r, len - 1);
    kk[u] = *reinterpret_cast<const uint4*>(src + (long)t * 3 * H * kD);
    vv[u] = *reinterpret_cast<const uint4*>(src + (long)t * 3 * H * kD + (long)H * kD);
  }
#pragma unroll
  for (int u = 0; u < kInsPasses; ++u) {
    const long at = row0 + min(t0 + u * kInsRowsPerPass + r, len - 1);
    quantize_store(kk[u], c, kc + at * kD, ksc + at);
    quantize_store(vv[u], c, vc + at * kD, vsc + at);
  }
}

}  // namespace

// k_cache, v_cache int8 [B, H, Tmax, 64], k_scale, v_scale fp32 [B, H, Tmax]; the rest as
// ra_attn_decode, ws sized by ra_attn_decode_work. qkv_new, the caches and out 16-byte
// aligned. Runs on the caller's stream; no host synchronisation, no allocation, lens stays on
// the device and is not modified.
RA_EXPORT int ra_attn_decode_q8(const void* qkv_new, void* k_cache, void* v_cache, float* k_scale,
                                float* v_scale, const int* lens, void* out, float* ws, int B,
                                int H, int Tmax, float scale, int splits, hipStream_t st) {
  if (B <= 0 || H <= 0 || Tmax <= 0 || B > 65535 || H > 65535 || Tmax > (1 << 22) ||
      splits < 0 || splits > kMaxSplits)
    return hipErrorInvalidValue;
  if ((((uintptr_t)qkv_new | (uintptr_t)k_cache | (uintptr_t)v_cache | (uintptr_t)out) & 15) ||
      (((uintptr_t)k_scale | (uintptr_t)v_scale) & 3) || k_scale == nullptr ||
      v_scale == nullptr || lens == nullptr)
    return hipErrorInvalidValue;
  const int S = splits > 0 ? splits : ra_attn_decode_splits(B, H, Tmax);
  if (S > 1 && ws == nullptr) return hipErrorInvalidValue;
  DecodeQ8Args a;
  a.qkv = (const bf16_t*)qkv_new;
  a.kc = (int8_t*)k_cache;
  a.vc = (int8_t*)v_cache;
  a.ksc = k_scale;
  a.vsc = v_scale;
  a.lens = lens;
  a.out = (bf16_t*)out;
  a.part_o = ws;
  a.part_ml = ws ? ws + (long)B * H * S * kD : nullptr;
  a.H = H;
  a.Tmax = Tmax;
  a.S = S;
  a.sc_log2 = scale * 1.4426950408889634f;
  if (S == 1) {
    hipLaunchKernelGGL(attn_decode_q8_kernel<true>, dim3(1, H, B), dim3(kThreads), 0, st, a);
  } else {
    hipLaunchKernelGGL(attn_decode_q8_kernel<false>, dim3(S, H, B), dim3(kThreads), 0, st, a);
    hipLaunchKernelGGL(attn_decode_q8_merge_kernel, dim3(B * H), dim3(kD), 0, st, a.part_o,
                       a.part_ml, a.out, S);
  }
  return hipGetLastError();
}

// qkv and the caches 16-byte aligned. Runs on the caller's stream; no host synchronisation,
// no allocation; slots and lens stay on the device and are only read.
RA_EXPORT int ra_kv_insert_q8(const void* qkv, void* k_cache, void* v_cache, float* k_scale,
                              float* v_scale, const int* slots, const int* lens, int Bn, int Tp,
                              int H, int S, int Tmax, hipStream_t st) {
  if (Bn <= 0 || Tp <= 0 || H <= 0 || S <= 0 || Tmax <= 0 || Bn > 65535 || H > 65535 ||
      Tp > (1 << 22) || Tmax > (1 << 22))
    return hipErrorInvalidValue;
  if ((((uintptr_t)qkv | (uintptr_t)k_cache | (uintptr_t)v_cache) & 15) ||
      (((uintptr_t)k_scale | (uintptr_t)v_scale) & 3) || k_scale == nullptr ||
      v_scale == nullptr || slots == nullptr || lens == nullptr)
    return hipErrorInvalidValue;
  const int n = Tp < Tmax ? Tp : Tmax;
  hipLaunchKernelGGL(kv_insert_q8_kernel, dim3((n + kInsBlockRows - 1) / kInsBlockRows, H, Bn),
                     dim3(kInsThreads), 0, st, (const bf16_t*)qkv, (int8_t*)k_cache,
                     (int8_t*)v_cache, k_scale, v_scale, slots, lens, Tp, H, S, Tmax);
  return hipGetLastError();
}
