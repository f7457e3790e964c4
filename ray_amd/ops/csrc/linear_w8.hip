// Weight-only int8 linear (W8A16, per-output-channel scales) for inference, and the
// dequantiser that serves its large-M side. The op behind GPT2.quantize_weights
// (models/gpt2.py): the four linears of every layer and the tied LM head at decode, where a
// step has few tokens and the linears are skinny GEMMs bound by the weight stream.
//
//   y[m, n] = bf16( s[n] * fp32(sum_k x[m, k] * q[n, k]) + b[n] )
//
//   x  [M, K]  bf16, row stride ldx (elements, % 8 == 0)
//   q  [N, K]  int8, contiguous, values in [-127, 127]
//   s  [N]     fp32                  b  [N] bf16 or null
//   y  [M, N]  bf16, row stride ldy >= N (% 8 == 0); bytes outside [M, N] keep their value
//
// K % 32 == 0, N % 32 == 0, any M >= 1. An int8 value is exact in bf16, so the MFMA operands
// are exact; the sum is fp32, the epilogue one fmaf, and the only rounding to bf16 is the last.
//
// ra_linear_w8: grid (N / 32, splits, ceil(M / 128)), one workgroup of 4 waves per 32 output
// channels x up to 128 tokens (TT = 1..4 token tiles of 32, 16 accumulator VGPRs each).
//   MFMA    v_mfma_f32_32x32x16_bf16, the weights as the A operand (channel on the lane) and
//           x^T as the B operand: the result has the token on the lane and 16 channels in the
//           registers.
//   loads   both operands go from global memory straight into VGPRs, k-contiguous; the
//           weights are used once and never touch LDS. A lane's weight load is 16 bytes = 16
//           consecutive k of its channel: lane half hh takes bytes [32 step + 16 hh, +16) and
//           feeds two MFMAs, so the k order inside a 32-k step is permuted (slot e of half hh
//           of MFMA h is k = 32 step + 16 hh + 8 h + e) and the x fragments come from the
//           same k: two 16-byte loads per token tile and step. Eight steps' weight loads are
//           in flight before the first conversion (then 4, 2, 1 for the tail of a run); the x
//           fragments follow in groups of 64 VGPRs. int8 -> bf16 is plain VALU converts.
//   K split the workgroup's 32-k steps [steps * j / splits, steps * (j + 1) / splits) are dealt
//           to its four waves in contiguous runs the same way (a run may be empty). The waves
//           merge their fp32 partials through LDS in wave order, ((p0 + p1) + p2) + p3: wave w
//           sums registers 4w..4w+3 of every tile, i.e. 4 consecutive channels per lane.
//   store   the merged [tokens][32] fp32 tile is staged in the same LDS and leaves as whole
//           row segments: 4 lanes x 16 bytes per token row of y (splits == 1: scale, bias and
//           the rounding happen here), or 8 lanes x 16 bytes per row of the fp32 workspace
//           [splits, M, N] (splits > 1), which linear_w8_reduce_kernel sums in split index
//           order before the same epilogue. Token rows past M are not stored; the padding lanes
//           of a token tail repeat the last real row.
// No atomics, no host read, one or two launches on the caller's stream: capturable.
//
// Invariance: a token's output bits depend on its own x row, on q, s, b and on (N, K,
// splits), never on M, the row's place in a tile or group, or the other rows. The k order is
// fixed by K and splits alone (split j, wave w, steps in order, MFMA h = 0 then 1; the chunking
// into 8/4/2/1 steps only moves loads), an MFMA output element is a function of its own
// operand row and column, and the merges add in a fixed order.
//
// ra_dequant_w8: w[n, k] = bf16(float(q[n, k]) * s[n]) into a caller's bf16 [N, K], 16 weights
// per thread (one 16-byte load, two 16-byte stores), K % 16 == 0. For large M (prompt passes)
// a skinny kernel would re-read x once per channel tile; there the library GEMM on the
// dequantised scratch is the right tool.
#include "attn_mfma.h"

#include <type_traits>

namespace {

constexpr int kMaxSplits = 64;
constexpr int kStageLd = 36;  // floats per token row of the staged [tokens][32] tile
constexpr int kCUs = 256;     // MI355X; the split choice is a function of N and K only

typedef int i32x4 __attribute__((ext_vector_type(4)));

struct W8Args {
  const bf16_t* x;
  const int8_t* q;
  const float* s;
  const bf16_t* b;
  bf16_t* y;
  float* ws;
  long ldx, ldy;
  int M, N, K;
};

// 8 consecutive int8 (two dwords) -> the bf16 fragment, exact
__device__ __forceinline__ bf16x8_t cvt8(int lo, int hi) {
  bf16x8_t r;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    r[j] = (__bf16)(float)(int8_t)(lo >> (8 * j));
    r[4 + j] = (__bf16)(float)(int8_t)(hi >> (8 * j));
  }
  return r;
}

// y[m, n..n+7] = bf16(fmaf(s, d, b)): the one epilogue of both the fused and the reduced path
__device__ __forceinline__ void store8(const W8Args& a, long m, int n, f32x4 d0, f32x4 d1) {
  const f32x4 s0 = *reinterpret_cast<const f32x4*>(a.s + n);
  const f32x4 s1 = *reinterpret_cast<const f32x4*>(a.s + n + 4);
  float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (a.b) unpack8(*reinterpret_cast<const uint4*>(a.b + n), f);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[j] = fmaf(s0[j], d0[j], f[j]);
    f[4 + j] = fmaf(s1[j], d1[j], f[4 + j]);
  }
  *reinterpret_cast<uint4*>(a.y + m * a.ldy + n) = pack8(f);
}

// TT: 32-token tiles of this launch's groups. kFinal: one split, the epilogue runs here.
template <int TT, bool kFinal>
__global__ __launch_bounds__(256) void linear_w8_kernel(W8Args a) {
  __shared__ __attribute__((aligned(16))) float lds[4 * TT * 16 * 64];
  static_assert(4 * TT * 16 * 64 >= 32 * TT * kStageLd, "the stage reuses the partials' LDS");
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, hh = lane >> 5;
  const int n0 = blockIdx.x * 32, m0 = blockIdx.z * (32 * TT);
  // this workgroup's 32-k steps, then this wave's run of them
  const int steps = a.K >> 5, S = gridDim.y;
  const int g0 = steps * (int)blockIdx.y / S;  // K <= 2^24, splits <= 64: no overflow
  const int ng = steps * ((int)blockIdx.y + 1) / S - g0;
  const int k0 = 32 * (g0 + ng * w / 4), k1 = 32 * (g0 + ng * (w + 1) / 4);

  const int8_t* qp = a.q + (long)(n0 + r) * a.K + 16 * hh;
  const bf16_t* xp[TT];
#pragma unroll
  for (int t = 0; t < TT; ++t)  // a tail's padding lanes repeat the last real token
    xp[t] = a.x + (long)min(m0 + 32 * t + r, a.M - 1) * a.ldx + 16 * hh;
  f32x16 acc[TT];
#pragma unroll
  for (int t = 0; t < TT; ++t) acc[t] = f32x16{};

  auto run = [&](int k, auto n_c) __attribute__((always_inline)) {
    constexpr int NS = decltype(n_c)::value;  // NS steps' weight loads in flight
    constexpr int XS = NS < 8 / TT ? NS : (8 / TT > 0 ? 8 / TT : 1);  // steps per x group
    i32x4 wq[NS];
#pragma unroll
    for (int u = 0; u < NS; ++u)
      wq[u] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(qp + k + 32 * u));
#pragma unroll
    for (int g = 0; g < NS; g += XS) {
      bf16x8_t xf[XS][TT][2];
#pragma unroll
      for (int u = 0; u < XS; ++u)
#pragma unroll
        for (int t = 0; t < TT; ++t)
#pragma unroll
          for (int h = 0; h < 2; ++h) xf[u][t][h] = ld8(xp[t] + k + 32 * (g + u) + 8 * h);
#pragma unroll
      for (int u = 0; u < XS; ++u) {
        const bf16x8_t a0 = cvt8(wq[g + u][0], wq[g + u][1]);
        const bf16x8_t a1 = cvt8(wq[g + u][2], wq[g + u][3]);
#pragma unroll
        for (int t = 0; t < TT; ++t) {
          acc[t] = mfma32(a0, xf[u][t][0], acc[t]);
          acc[t] = mfma32(a1, xf[u][t][1], acc[t]);
        }
      }
    }
  };
  int k = k0;
  for (; k + 256 <= k1; k += 256) run(k, std::integral_constant<int, 8>{});
  if (k + 128 <= k1) {
    run(k, std::integral_constant<int, 4>{});
    k += 128;
  }
  if (k + 64 <= k1) {
    run(k, std::integral_constant<int, 2>{});
    k += 64;
  }
  if (k < k1) run(k, std::integral_constant<int, 1>{});

  // merge in wave order; wave w ends up with registers 4w..4w+3 of every tile, which are
  // channels 8w + 4hh + 0..3 of token 32t + r
#pragma unroll
  for (int t = 0; t < TT; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) lds[((w * TT + t) * 16 + i) * 64 + lane] = acc[t][i];
  __syncthreads();
  f32x4 sum[TT];
#pragma unroll
  for (int t = 0; t < TT; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float v = lds[((0 * TT + t) * 16 + 4 * w + j) * 64 + lane];
#pragma unroll
      for (int p = 1; p < 4; ++p) v += lds[((p * TT + t) * 16 + 4 * w + j) * 64 + lane];
      sum[t][j] = v;
    }
  __syncthreads();  // the partials are dead: the stage reuses their LDS
#pragma unroll
  for (int t = 0; t < TT; ++t)
    *reinterpret_cast<f32x4*>(lds + (32 * t + r) * kStageLd + 8 * w + 4 * hh) = sum[t];
  __syncthreads();

  const int rows = min(32 * TT, a.M - m0);
  if (kFinal) {
    for (int e = threadIdx.x; e < rows * 4; e += 256) {
      const int row = e >> 2, c = (e & 3) * 8;
      const float* d = lds + row * kStageLd + c;
      store8(a, m0 + row, n0 + c, *reinterpret_cast<const f32x4*>(d),
             *reinterpret_cast<const f32x4*>(d + 4));
    }
  } else {
    float* part = a.ws + ((long)blockIdx.y * a.M + m0) * a.N + n0;
    for (int e = threadIdx.x; e < rows * 8; e += 256) {
      const int row = e >> 3, c = (e & 7) * 4;
      *reinterpret_cast<f32x4*>(part + (long)row * a.N + c) =
          *reinterpret_cast<const f32x4*>(lds + row * kStageLd + c);
    }
  }
}

// Sums the splits' partials in split index order, 8 channels of one token per thread.
__global__ __launch_bounds__(256) void linear_w8_reduce_kernel(W8Args a, int S) {
  const int n8 = a.N >> 3;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)a.M * n8) return;
  const long m = i / n8;
  const int n = (int)(i - m * n8) * 8;
  const float* p = a.ws + m * a.N + n;
  const long slab = (long)a.M * a.N;
  f32x4 d0 = *reinterpret_cast<const f32x4*>(p), d1 = *reinterpret_cast<const f32x4*>(p + 4);
  for (int j = 1; j < S; ++j) {
    d0 += *reinterpret_cast<const f32x4*>(p + j * slab);
    d1 += *reinterpret_cast<const f32x4*>(p + j * slab + 4);
  }
  store8(a, m, n, d0, d1);
}

__global__ __launch_bounds__(256) void dequant_w8_kernel(const i32x4* __restrict__ q,
                                                         const float* __restrict__ s,
                                                         uint4* __restrict__ w, long n16,
                                                         int k16) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n16; i += (long)gridDim.x * 256) {
    const float sc = s[i / k16];
    const i32x4 v = q[i];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float f[8];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        f[j] = (float)(int8_t)(v[2 * h] >> (8 * j)) * sc;
        f[4 + j] = (float)(int8_t)(v[2 * h + 1] >> (8 * j)) * sc;
      }
      w[2 * i + h] = pack8(f);
    }
  }
}

template <int TT>
void launch_w8(const W8Args& a, int S, hipStream_t st) {
  const dim3 grid(a.N / 32, S, (a.M + 32 * TT - 1) / (32 * TT));
  if (S == 1)
    hipLaunchKernelGGL((linear_w8_kernel<TT, true>), grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((linear_w8_kernel<TT, false>), grid, dim3(256), 0, st, a);
}

}  // namespace

// Split count of the skinny kernel, a function of N and K only (never of M, so a token's bits
// do not move with the batch): as many splits as keep the grid within two workgroups per CU
// and leave every split at least 16 steps (four per wave), at most 8. N = 768, K = 3072: 6;
// the LM head and the wide layers: 1.
RA_EXPORT int ra_linear_w8_splits(int N, int K) {
  if (N < 32 || K < 32) return 1;
  const int tiles = N / 32, steps = K / 32;
  int S = 2 * kCUs / tiles;
  if (S > steps / 16) S = steps / 16;
  if (S > 8) S = 8;
  return S < 1 ? 1 : S;
}

namespace {
inline int resolve_splits(int N, int K, int splits) {
  return splits > 0 ? splits : ra_linear_w8_splits(N, K);
}
}  // namespace

// fp32 elements of workspace that ra_linear_w8 needs for this splits argument (0 =
// automatic): [splits, M, N], or 0 when one split writes y itself.
RA_EXPORT long ra_linear_w8_work(int M, int N, int K, int splits) {
  if (M <= 0 || N <= 0 || K <= 0 || splits < 0 || splits > kMaxSplits) return 0;
  const int S = resolve_splits(N, K, splits);
  return S > 1 ? (long)S * M * N : 0;
}

// splits: 0 = ra_linear_w8_splits(N, K), else the explicit count (<= 64). ws:
// ra_linear_w8_work floats (may be null when that is 0). x, q, s, b, y, ws 16-byte aligned,
// ldx and ldy in elements. Runs on the caller's stream; no host synchronisation, no allocation.
RA_EXPORT int ra_linear_w8(const void* x, long ldx, const void* q, const float* s, const void* b,
                           void* y, long ldy, float* ws, int M, int N, int K, int splits,
                           hipStream_t st) {
  if (M <= 0 || N < 32 || K < 32 || (N & 31) || (K & 31) || M > 32 * 65535 ||
      K > (1 << 24) || ldx < K || ldy < N || (ldx & 7) || (ldy & 7) || splits < 0 ||
      splits > kMaxSplits)
    return hipErrorInvalidValue;
  if (x == nullptr || q == nullptr || s == nullptr || y == nullptr ||
      (((uintptr_t)x | (uintptr_t)q | (uintptr_t)s | (uintptr_t)b | (uintptr_t)y |
        (uintptr_t)ws) & 15))
    return hipErrorInvalidValue;
  const int S = resolve_splits(N, K, splits);
  if (S > 1 && ws == nullptr) return hipErrorInvalidValue;
  const W8Args a{(const bf16_t*)x, (const int8_t*)q, s, (const bf16_t*)b, (bf16_t*)y, ws,
                 ldx, ldy, M, N, K};
  if (M <= 32)
    launch_w8<1>(a, S, st);
  else if (M <= 64)
    launch_w8<2>(a, S, st);
  else if (M <= 96)
    launch_w8<3>(a, S, st);
  else
    launch_w8<4>(a, S, st);
  if (S > 1) {
    const long threads = (long)M * (N / 8);
    hipLaunchKernelGGL(linear_w8_reduce_kernel, dim3((unsigned)((threads + 255) / 256)),
                       dim3(256), 0, st, a, S);
  }
  return hipGetLastError();
}

// w[n, k] = bf16(float(q[n, k]) * s[n]); q int8 [N, K] and w bf16 [N, K] contiguous and 16-byte
// aligned, K % 16 == 0. One launch on the caller's stream.
RA_EXPORT int ra_dequant_w8(const void* q, const float* s, void* w, int N, int K,
                            hipStream_t st) {
  if (N <= 0 || K < 16 || (K & 15) || q == nullptr || s == nullptr || w == nullptr ||
      (((uintptr_t)q | (uintptr_t)w) & 15))
    return hipErrorInvalidValue;
  const long n16 = (long)N * (K / 16);
  hipLaunchKernelGGL(dequant_w8_kernel, dim3(ra_grid(n16, 256)), dim3(256), 0, st,
                     (const i32x4*)q, s, (uint4*)w, n16, K / 16);
  return hipGetLastError();
}
