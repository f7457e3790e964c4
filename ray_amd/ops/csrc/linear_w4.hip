// Weight-only MXFP4 linear (W4A16, OCP microscaling: e2m1 elements, one e8m0 scale per 32
// consecutive k) for inference, and the dequantiser that serves its large-M side. The op behind
// GPT2.quantize_weights(fmt="mxfp4") (models/gpt2.py): the four linears of every layer and the
// tied LM head at decode, where a step has few tokens and the linears are skinny GEMMs bound by
// the weight stream. 4.25 bits per weight: 0.27x the bf16 bytes, 0.53x the int8 ones.
//
//   y[m, n] = bf16( fp32(sum_k x[m, k] * dq[n, k]) + b[n] )
//   dq[n, k] = e2m1(nibble k of row n) * 2^(s[n, k / 32] - 127)
//
//   x  [M, K]     bf16, row stride ldx (elements, % 8 == 0)
//   q  [N, K/2]   uint8, contiguous: byte j of a row holds k = 2j in its low nibble and
//                 k = 2j + 1 in its high nibble; a nibble is sign, then the code of
//                 {0, 0.5, 1, 1.5, 2, 3, 4, 6}
//   s  [N, K/32]  uint8 e8m0, contiguous, 2-byte aligned (rows are K/32 bytes, an even count)
//   b  [N]        bf16 or null
//   y  [M, N]     bf16, row stride ldy >= N (% 8 == 0); bytes outside [M, N] keep their value
//
// K % 64 == 0, N % 32 == 0, any M >= 1. dq is exact in bf16 for every code and every scale byte
// in [3, 254], so the MFMA operands are exact; the sum is fp32 and nothing is scaled after the
// MFMA: the epilogue adds the bias and rounds once. Scale bytes 0 and 255 (never produced by the
// quantiser) give an unspecified value but touch no memory.
//
// ra_linear_w4: grid (N / 32, splits, ceil(M / 128)), one workgroup of 4 waves per 32 output
// channels x up to 128 tokens (TT = 1..4 token tiles of 32, 16 accumulator VGPRs each).
//   MFMA    v_mfma_f32_32x32x16_bf16, the weights as the A operand (channel on the lane) and
//           x^T as the B operand: the result has the token on the lane and 16 channels in the
//           registers.
//   loads   both operands go from global memory straight into VGPRs, k-contiguous; the
//           weights are used once and never touch LDS. A lane's weight load is 16 bytes = 32
//           consecutive k of its channel = exactly one MX block. The k step is 64: lane half hh
//           takes block 2 step + hh and feeds four MFMAs from its four dwords, so slot e of
//           half hh of MFMA h is k = 64 step + 32 hh + 8 h + e, and the x fragments come from
//           the same k: four 16-byte loads, 64 contiguous bytes of the token's row, per token
//           tile and step. Eight steps' weight loads (512 k, 32 VGPRs) are in flight before the
//           first conversion (then 4, 2, 1 for the tail of a run); the x fragments follow in
//           groups of at most 64 VGPRs.
//   scales  a run of 8 steps needs 16 consecutive scale bytes of the lane's channel, two per
//           step, one per lane half: ONE 16-byte load per run, issued before the run's weight
//           loads (loads return in order, so it has landed when the first weight has); 8 / 4 /
//           2 bytes for the tails. The lane picks its byte with a shift by 16 (step & 1) + 8 hh.
//           A row of s starts on a 2-byte boundary and no better (24 bytes at K = 768), so these
//           loads are declared 2-byte aligned; global memory takes them as they are.
//   convert v_cvt_scalef32_pk_bf16_fp4: one byte (two e2m1) times the block scale -> two bf16,
//           four per weight dword = one A fragment. The scale operand is the float with the
//           bit pattern s << 23, i.e. 2^(s - 127) itself for s in [1, 254].
//   K split the workgroup's 64-k steps [steps * j / splits, steps * (j + 1) / splits) are dealt
//           to its four waves in contiguous runs the same way (a run may be empty). The waves
//           merge their fp32 partials through LDS in wave order, ((p0 + p1) + p2) + p3: wave w
//           sums registers 4w..4w+3 of every tile, i.e. 4 consecutive channels per lane.
//   store   the merged [tokens][32] fp32 tile is staged in the same LDS and leaves as whole
//           row segments: 4 lanes x 16 bytes per token row of y (splits == 1: bias and the
//           rounding happen here), or 8 lanes x 16 bytes per row of the fp32 workspace
//           [splits, M, N] (splits > 1), which linear_w4_reduce_kernel sums in split index
//           order before the same epilogue. Token rows past M are not stored; the padding lanes
//           of a token tail repeat the last real row.
// No atomics, no host read, one or two launches on the caller's stream: capturable.
//
// Invariance: a token's output bits depend on its own x row, on q, s, b and on (N, K,
// splits), never on M, the row's place in a tile or group, or the other rows. The k order is
// fixed by K and splits alone (split j, wave w, steps in order, MFMA h = 0, 1, 2, 3; the
// chunking into 8/4/2/1 steps only moves loads), an MFMA output element is a function of its
// own operand row and column, and the merges add in a fixed order.
//
// ra_dequant_w4: w[n, k] = bf16(dq[n, k]) into a caller's bf16 [N, K], one MX block per thread
// (one 16-byte load, one scale byte, four 16-byte stores) through the same convert, K % 32 == 0.
// For large M (prompt passes) a skinny kernel would re-read x once per channel tile; there the
// library GEMM on the dequantised scratch is the right tool.
//
// Compiler's figures (gfx950, -O3, kernel-resource-usage), scratch 0 everywhere:
//   linear_w4_kernel<TT, final/split>  VGPRs      LDS bytes
//     TT = 1                           80        16384
//     TT = 2                           104       32768
//     TT = 3                           190       49152
//     TT = 4                           220       65536
//   linear_w4_reduce_kernel            22        0
//   dequant_w4_kernel                  23        0
#include "attn_mfma.h"

#include <type_traits>

namespace {

constexpr int kMaxSplits = 64;
constexpr int kStageLd = 36;  // floats per token row of the staged [tokens][32] tile
constexpr int kCUs = 256;     // MI355X; the split choice is a function of N and K only

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
// scale runs start on 2-byte boundaries (header: scales)
typedef u32x4 __attribute__((aligned(2))) u32x4_a2;
typedef u32x2 __attribute__((aligned(2))) u32x2_a2;
typedef uint32_t __attribute__((aligned(2))) u32_a2;

struct W4Args {
  const bf16_t* x;
  const uint8_t* q;
  const uint8_t* s;
  const bf16_t* b;
  bf16_t* y;
  float* ws;
  long ldx, ldy;
  int M, N, K;
};

// the e8m0 byte in bits [sh, sh + 8) of v as the float 2^(byte - 127)
__device__ __forceinline__ float e8m0(uint32_t v, int sh) {
  return __uint_as_float(((v >> sh) & 0xffu) << 23);
}

// 8 consecutive e2m1 (one dword, low nibble first) times the block scale -> the bf16 fragment
__device__ __forceinline__ bf16x8_t cvt8(uint32_t v, float sc) {
  const bf16x2 p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, sc, 0);
  const bf16x2 p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, sc, 1);
  const bf16x2 p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, sc, 2);
  const bf16x2 p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, sc, 3);
  return bf16x8_t{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
}

// the 2 NS scale bytes of NS steps of one channel, as dwords (NS = 1: the low half of one)
template <int NS>
__device__ __forceinline__ void ld_scales(const uint8_t* p, uint32_t (&sw)[(NS + 1) / 2]) {
  if constexpr (NS == 8) {
    const u32x4 v = *reinterpret_cast<const u32x4_a2*>(p);
    sw[0] = v[0], sw[1] = v[1], sw[2] = v[2], sw[3] = v[3];
  } else if constexpr (NS == 4) {
    const u32x2 v = *reinterpret_cast<const u32x2_a2*>(p);
    sw[0] = v[0], sw[1] = v[1];
  } else if constexpr (NS == 2) {
    sw[0] = *reinterpret_cast<const u32_a2*>(p);
  } else {
    sw[0] = *reinterpret_cast<const uint16_t*>(p);
  }
}

// y[m, n..n+7] = bf16(d + b): the one epilogue of both the fused and the reduced path
__device__ __forceinline__ void store8(const W4Args& a, long m, int n, f32x4 d0, f32x4 d1) {
  float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (a.b) unpack8(*reinterpret_cast<const uint4*>(a.b + n), f);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[j] += d0[j];
    f[4 + j] += d1[j];
  }
  *reinterpret_cast<uint4*>(a.y + m * a.ldy + n) = pack8(f);
}

// TT: 32-token tiles of this launch's groups. kFinal: one split, the epilogue runs here.
template <int TT, bool kFinal>
__global__ __launch_bounds__(256) void linear_w4_kernel(W4Args a) {
  __shared__ __attribute__((aligned(16))) float lds[4 * TT * 16 * 64];
  static_assert(4 * TT * 16 * 64 >= 32 * TT * kStageLd, "the stage reuses the partials' LDS");
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, hh = lane >> 5;
  const int n0 = blockIdx.x * 32, m0 = blockIdx.z * (32 * TT);
  // this workgroup's 64-k steps, then this wave's run of them
  const int steps = a.K >> 6, S = gridDim.y;
  const int g0 = steps * (int)blockIdx.y / S;  // K <= 2^24, splits <= 64: no overflow
  const int ng = steps * ((int)blockIdx.y + 1) / S - g0;
  const int t0 = g0 + ng * w / 4, t1 = g0 + ng * (w + 1) / 4;

  // per step: 32 bytes of the channel's q row (16 per lane half), 2 of its s row, 64 x elements
  const uint8_t* qp = a.q + (long)(n0 + r) * (a.K >> 1) + 16 * hh;
  const uint8_t* sp = a.s + (long)(n0 + r) * (a.K >> 5);
  const bf16_t* xp[TT];
#pragma unroll
  for (int t = 0; t < TT; ++t)  // a tail's padding lanes repeat the last real token
    xp[t] = a.x + (long)min(m0 + 32 * t + r, a.M - 1) * a.ldx + 32 * hh;
  f32x16 acc[TT];
#pragma unroll
  for (int t = 0; t < TT; ++t) acc[t] = f32x16{};

  auto run = [&](int st, auto n_c) __attribute__((always_inline)) {
    constexpr int NS = decltype(n_c)::value;  // NS steps' weight loads in flight
    constexpr int XS = NS < 4 / TT ? NS : (4 / TT > 0 ? 4 / TT : 1);  // steps per x group
    uint32_t sw[(NS + 1) / 2];
    ld_scales<NS>(sp + 2 * st, sw);
    u32x4 wq[NS];
#pragma unroll
    for (int u = 0; u < NS; ++u)
      wq[u] = __builtin_nontemporal_load(
          reinterpret_cast<const u32x4*>(qp + 32l * (st + u)));
#pragma unroll
    for (int g = 0; g < NS; g += XS) {
      bf16x8_t xf[XS][TT][4];
#pragma unroll
      for (int u = 0; u < XS; ++u)
#pragma unroll
        for (int t = 0; t < TT; ++t)
#pragma unroll
          for (int h = 0; h < 4; ++h) xf[u][t][h] = ld8(xp[t] + 64l * (st + g + u) + 8 * h);
#pragma unroll
      for (int u = 0; u < XS; ++u) {
        const float sc = e8m0(sw[(g + u) >> 1], 16 * ((g + u) & 1) + 8 * hh);
#pragma unroll
        for (int h = 0; h < 4; ++h) {
          const bf16x8_t af = cvt8(wq[g + u][h], sc);
#pragma unroll
          for (int t = 0; t < TT; ++t) acc[t] = mfma32(af, xf[u][t][h], acc[t]);
        }
      }
    }
  };
  int st = t0;
  for (; st + 8 <= t1; st += 8) run(st, std::integral_constant<int, 8>{});
  if (st + 4 <= t1) {
    run(st, std::integral_constant<int, 4>{});
    st += 4;
  }
  if (st + 2 <= t1) {
    run(st, std::integral_constant<int, 2>{});
    st += 2;
  }
  if (st < t1) run(st, std::integral_constant<int, 1>{});

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
__global__ __launch_bounds__(256) void linear_w4_reduce_kernel(W4Args a, int S) {
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

// thread i: MX block i = 16 bytes of q, byte i of s, 32 bf16 of w
__global__ __launch_bounds__(256) void dequant_w4_kernel(const u32x4* __restrict__ q,
                                                         const uint8_t* __restrict__ s,
                                                         u32x4* __restrict__ w, long nblk) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nblk; i += (long)gridDim.x * 256) {
    const float sc = e8m0(s[i], 0);
    const u32x4 v = q[i];
#pragma unroll
    for (int h = 0; h < 4; ++h) w[4 * i + h] = __builtin_bit_cast(u32x4, cvt8(v[h], sc));
  }
}

template <int TT>
void launch_w4(const W4Args& a, int S, hipStream_t st) {
  const dim3 grid(a.N / 32, S, (a.M + 32 * TT - 1) / (32 * TT));
  if (S == 1)
    hipLaunchKernelGGL((linear_w4_kernel<TT, true>), grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((linear_w4_kernel<TT, false>), grid, dim3(256), 0, st, a);
}

}  // namespace

// Split count of the skinny kernel, a function of N and K only (never of M, so a token's bits
// do not move with the batch): as many splits as keep the grid within two workgroups per CU
// and leave every split at least 8 of the 64-k steps (two per wave, the same 512 k as the int8
// kernel's 16 steps of 32), at most 8. N = 768, K = 3072: 6; the LM head and the wide layers: 1.
RA_EXPORT int ra_linear_w4_splits(int N, int K) {
  if (N < 32 || K < 64) return 1;
  const int tiles = N / 32, steps = K / 64;
  int S = 2 * kCUs / tiles;
  if (S > steps / 8) S = steps / 8;
  if (S > 8) S = 8;
  return S < 1 ? 1 : S;
}

namespace {
inline int resolve_splits(int N, int K, int splits) {
  return splits > 0 ? splits : ra_linear_w4_splits(N, K);
}
}  // namespace

// fp32 elements of workspace that ra_linear_w4 needs for this splits argument (0 =
// automatic): [splits, M, N], or 0 when one split writes y itself.
RA_EXPORT long ra_linear_w4_work(int M, int N, int K, int splits) {
  if (M <= 0 || N <= 0 || K <= 0 || splits < 0 || splits > kMaxSplits) return 0;
  const int S = resolve_splits(N, K, splits);
  return S > 1 ? (long)S * M * N : 0;
}

// splits: 0 = ra_linear_w4_splits(N, K), else the explicit count (<= 64). ws:
// ra_linear_w4_work floats (may be null when that is 0). x, q, b, y, ws 16-byte aligned, s
// 2-byte aligned, ldx and ldy in elements. Runs on the caller's stream; no host
// synchronisation, no allocation.
RA_EXPORT int ra_linear_w4(const void* x, long ldx, const void* q, const void* s, const void* b,
                           void* y, long ldy, float* ws, int M, int N, int K, int splits,
                           hipStream_t st) {
  if (M <= 0 || N < 32 || K < 64 || (N & 31) || (K & 63) || M > 32 * 65535 ||
      K > (1 << 24) || ldx < K || ldy < N || (ldx & 7) || (ldy & 7) || splits < 0 ||
      splits > kMaxSplits)
    return hipErrorInvalidValue;
  if (x == nullptr || q == nullptr || s == nullptr || y == nullptr ||
      (((uintptr_t)x | (uintptr_t)q | (uintptr_t)b | (uintptr_t)y | (uintptr_t)ws) & 15) ||
      ((uintptr_t)s & 1))
    return hipErrorInvalidValue;
  const int S = resolve_splits(N, K, splits);
  if (S > 1 && ws == nullptr) return hipErrorInvalidValue;
  const W4Args a{(const bf16_t*)x, (const uint8_t*)q, (const uint8_t*)s, (const bf16_t*)b,
                 (bf16_t*)y, ws, ldx, ldy, M, N, K};
  if (M <= 32)
    launch_w4<1>(a, S, st);
  else if (M <= 64)
    launch_w4<2>(a, S, st);
  else if (M <= 96)
    launch_w4<3>(a, S, st);
  else
    launch_w4<4>(a, S, st);
  if (S > 1) {
    const long threads = (long)M * (N / 8);
    hipLaunchKernelGGL(linear_w4_reduce_kernel, dim3((unsigned)((threads + 255) / 256)),
                       dim3(256), 0, st, a, S);
  }
  return hipGetLastError();
}

// w[n, k] = bf16(dq[n, k]); q uint8 [N, K/2] and w bf16 [N, K] contiguous and 16-byte aligned,
// s uint8 [N, K/32] contiguous, K % 32 == 0. One launch on the caller's stream.
RA_EXPORT int ra_dequant_w4(const void* q, const void* s, void* w, int N, int K,
                            hipStream_t st) {
  if (N <= 0 || K < 32 || (K & 31) || q == nullptr || s == nullptr || w == nullptr ||
      (((uintptr_t)q | (uintptr_t)w) & 15))
    return hipErrorInvalidValue;
  const long nblk = (long)N * (K / 32);
  hipLaunchKernelGGL(dequant_w4_kernel, dim3(ra_grid(nblk, 256)), dim3(256), 0, st,
                     (const u32x4*)q, (const uint8_t*)s, (u32x4*)w, nblk);
  return hipGetLastError();
}
