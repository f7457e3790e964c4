// Batched multi-LoRA: y[b] += scale[a] * (x[b] . A[a]^T) . B[a]^T with the adapter a = idx[b]
// chosen per batch row ON THE DEVICE, bf16. The op behind per-request adapters in the GPT-2
// engine (models/lora.py, models/gpt2.py, models/gpt2_engine.py).
//
//   x        [Bn, T, Din]             contiguous
//   y        [Bn, T, Dout]            contiguous, read-modify-written IN PLACE
//   a_stack  [n_adapters, R, Din]     b_stack [n_adapters, Dout, R]
//   scale    [n_adapters] fp32        idx [Bn] int32, both only read, on the device
//
// For a row with 0 <= idx[b] < n_adapters and every token i:
//   t        = bf16(fp32 sum_k x[b,i,k] * A[a][:,k])                      (R values, one rounding)
//   y[b,i,:] = bf16(float(y[b,i,:]) + scale[a] * fp32 sum_r t[r] * B[a][:,r])
// Any other row is not touched: the workgroup leaves before its first load of x or y, so the
// bytes stay (NaN payloads included). That is how a base-model request (idx = -1) shares a
// batch with adapted ones. One launch on the caller's stream, no host read, no workspace, no
// atomics: capturable, and one capture serves every assignment of adapters to rows.
// R in {16, 32, 48, 64}; Din and Dout multiples of 64.
//
// One workgroup of 4 waves per (row, 32-token tile, group of 64-column chunks of Dout).
//   shrink  X = A[a] . x_tile^T on v_mfma_f32_32x32x16_bf16: both operands are 16-byte global
//           loads straight into VGPRs (A rows and x rows are both k-contiguous). The result has
//           r in the 16 registers and the token on the lane. The 4 waves split K in four
//           contiguous quarters and merge their fp32 partials through LDS in wave order, so
//           every wave ends up with the same whole X.
//   expand  Y^T = B[a] . X per 64-column chunk, the chunks dealt round-robin to the waves: the
//           bf16-converted accumulators of X are the B operand as they stand (no LDS round
//           trip). The k order inside such a step is permuted (element j of lane half h is row
//           16s + 8(j>>2) + 4h + (j&3) of X), so the b_stack fragment is loaded as two 8-byte
//           pieces from those same r.
//   store   Y^T has the token on the lane and 4 consecutive columns per register group: the
//           fp32 tile goes through a wave-private LDS image and leaves as whole 128-byte row
//           segments (8 lanes x 16 bytes per token row), where y is read, added to in fp32,
//           rounded once and written back. Token rows past T are not stored.
// Every column group recomputes X (one pass over A[a], 24-96 KB at GPT-2 small, L2 resident),
// which buys a grid of more than Bn workgroups at T = 1.
//
// Invariance: a token's bits depend only on its own x row, its own y row and its adapter. The
// k order of the shrink is fixed by Din alone (quarter w in 16-wide MFMA steps, then
// ((p0 + p1) + p2) + p3), that of the expand by R alone; an MFMA output element is a function
// of its own operand row and column only, so neither Bn, T, the place in the tile, the column
// grouping nor the other rows enter. Padding lanes of a token tail repeat the last real token
// and are dropped at the store.
#include "attn_mfma.h"

#include <type_traits>

namespace {

constexpr int kLd = 68;                      // floats per row of a wave's [32 tokens][64] stage
constexpr int kStage = 32 * kLd;             // floats of one wave's stage
constexpr int kLdsFloats = 4 * kStage;       // 34816 B; the merge needs 4 * 2 * 16 * 64 floats
static_assert(kLdsFloats >= 4 * 2 * 16 * 64, "the K-split partials must fit the stage");

__device__ __forceinline__ bf16x4_t ld4(const bf16_t* p) {
  return *reinterpret_cast<const bf16x4_t*>(p);
}

// NRB: 32-row blocks of X (R <= 32: 1, else 2). cpg: 64-column chunks per column group.
template <int NRB>
__global__ __launch_bounds__(256) void lora_add_kernel(
    bf16_t* __restrict__ y, const bf16_t* __restrict__ x, const bf16_t* __restrict__ As,
    const bf16_t* __restrict__ Bs, const float* __restrict__ scale, const int* __restrict__ idx,
    int T, int Din, int Dout, int R, int NA, int cpg) {
  __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
  const int b = blockIdx.z;
  const int a = idx[b];
  if (a < 0 || a >= NA) return;  // workgroup-uniform, before any barrier
  const int t0 = blockIdx.x * 32;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, hh = lane >> 5;

  // ---- shrink: X[rb] (rows r of A[a], columns = tokens), this wave's quarter of K
  const int tok = min(t0 + r, T - 1);  // a tail's padding lanes repeat the last real token
  const bf16_t* xp = x + ((long)b * T + tok) * Din + 8 * hh;
  const bf16_t* ap[NRB];
#pragma unroll
  for (int rb = 0; rb < NRB; ++rb)  // rows at or past R (R = 16, 48): repeat the last row; the
    ap[rb] = As + ((long)a * R + min(32 * rb + r, R - 1)) * Din + 8 * hh;  // expand never reads them
  f32x16 acc[NRB];
#pragma unroll
  for (int rb = 0; rb < NRB; ++rb) acc[rb] = f32x16{};
  const int kw = Din >> 2, k0 = w * kw;  // Din % 64 == 0: whole 16-wide steps
  auto steps = [&](int k, auto n_c) __attribute__((always_inline)) {
    constexpr int N = decltype(n_c)::value;  // N steps' loads in flight, then their MFMAs in k order
    bf16x8_t xf[N], af[N][NRB];
#pragma unroll
    for (int u = 0; u < N; ++u) {
      xf[u] = ld8(xp + k + 16 * u);
#pragma unroll
      for (int rb = 0; rb < NRB; ++rb) af[u][rb] = ld8(ap[rb] + k + 16 * u);
    }
#pragma unroll
    for (int u = 0; u < N; ++u)
#pragma unroll
      for (int rb = 0; rb < NRB; ++rb) acc[rb] = mfma32(af[u][rb], xf[u], acc[rb]);
  };
  int k = k0;
  for (; k + 64 <= k0 + kw; k += 64) steps(k, std::integral_constant<int, 4>{});
  for (; k < k0 + kw; k += 16) steps(k, std::integral_constant<int, 1>{});
  // merge in wave order: every wave reads the four partials and sums them the same way
#pragma unroll
  for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
    for (int i = 0; i < 16; ++i) lds[((w * NRB + rb) * 16 + i) * 64 + lane] = acc[rb][i];
  __syncthreads();
#pragma unroll
  for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      float s = lds[((0 * NRB + rb) * 16 + i) * 64 + lane];
#pragma unroll
      for (int p = 1; p < 4; ++p) s += lds[((p * NRB + rb) * 16 + i) * 64 + lane];
      acc[rb][i] = s;
    }
  __syncthreads();  // the partials are dead: the stages below reuse their LDS
  bf16x8_t tf[2 * NRB];  // t, rounded once: the B operand of expand step sg = 2 rb + s
#pragma unroll
  for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
    for (int s = 0; s < 2; ++s) tf[2 * rb + s] = acc_frag(acc[rb], s);

  // ---- expand + read-modify-write, chunk by chunk
  const float sc = scale[a];
  const int chunks = Dout >> 6;
  const int c0 = blockIdx.y * cpg, c1 = min(c0 + cpg, chunks);
  const int nrows = min(32, T - t0);
  const bf16_t* Bp = Bs + (long)a * Dout * R + 4 * hh;
  float* stg = lds + w * kStage;
  bf16_t* yrow = y + ((long)b * T + t0) * Dout;
  for (int c = c0 + w; c < c1; c += 4) {
    f32x16 yv[2] = {f32x16{}, f32x16{}};
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      const bf16_t* bp = Bp + (long)(c * 64 + 32 * nb + r) * R;
#pragma unroll
      for (int sg = 0; sg < 2 * NRB; ++sg)
        if (16 * sg < R)  // wave-uniform
          yv[nb] = mfma32(cat44(ld4(bp + 16 * sg), ld4(bp + 16 * sg + 8)), tf[sg], yv[nb]);
    }
    // register group g of block nb: columns 32 nb + 8 g + 4 hh + 0..3 of token r
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<f32x4*>(stg + r * kLd + 32 * nb + 8 * g + 4 * hh) =
            f32x4{yv[nb][4 * g], yv[nb][4 * g + 1], yv[nb][4 * g + 2], yv[nb][4 * g + 3]};
    wave_lds_order();
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int row = 8 * p + (lane >> 3), ch = lane & 7;
      if (row < nrows) {
        uint4* yp = reinterpret_cast<uint4*>(yrow + (long)row * Dout + c * 64 + ch * 8);
        const f32x4 d0 = *reinterpret_cast<const f32x4*>(stg + row * kLd + ch * 8);
        const f32x4 d1 = *reinterpret_cast<const f32x4*>(stg + row * kLd + ch * 8 + 4);
        float f[8];
        unpack8(*yp, f);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          f[j] = f[j] + sc * d0[j];
          f[4 + j] = f[4 + j] + sc * d1[j];
        }
        *yp = pack8(f);
      }
    }
    wave_lds_order();  // the next chunk overwrites the stage
  }
}

}  // namespace

// y, x, a_stack, b_stack 16-byte aligned. Runs on the caller's stream: no host synchronisation,
// no allocation; idx and scale stay on the device and are only read.
RA_EXPORT int ra_lora_add(void* y, const void* x, const void* a_stack, const void* b_stack,
                          const float* scale, const int* idx, int Bn, int T, int Din, int Dout,
                          int R, int NA, hipStream_t st) {
  if (Bn <= 0 || T <= 0 || NA <= 0 || Din < 64 || Dout < 64 || (Din & 63) || (Dout & 63) ||
      (R != 16 && R != 32 && R != 48 && R != 64) || T > (1 << 26))
    return hipErrorInvalidValue;
  if ((((uintptr_t)y | (uintptr_t)x | (uintptr_t)a_stack | (uintptr_t)b_stack) & 15) ||
      scale == nullptr || idx == nullptr)
    return hipErrorInvalidValue;
  const int tiles = (T + 31) / 32, chunks = Dout / 64;
  // Column groups: enough workgroups to fill the chip at small Bn * T, but never fewer than
  // four chunks (one per wave) in a group. The grouping does not enter the results.
  for (int b0 = 0; b0 < Bn; b0 += 65535) {
    const int nb = Bn - b0 < 65535 ? Bn - b0 : 65535;
    const long wgs = (long)nb * tiles;
    long want = (1024 + wgs - 1) / wgs;
    const int most = chunks / 4 > 0 ? chunks / 4 : 1;
    if (want > most) want = most;
    const int cpg = (chunks + (int)want - 1) / (int)want;
    const dim3 grid(tiles, (chunks + cpg - 1) / cpg, nb);
    bf16_t* yb = (bf16_t*)y + (long)b0 * T * Dout;
    const bf16_t* xb = (const bf16_t*)x + (long)b0 * T * Din;
    if (R <= 32)
      hipLaunchKernelGGL(lora_add_kernel<1>, grid, dim3(256), 0, st, yb, xb,
                         (const bf16_t*)a_stack, (const bf16_t*)b_stack, scale, idx + b0, T, Din,
                         Dout, R, NA, cpg);
    else
      hipLaunchKernelGGL(lora_add_kernel<2>, grid, dim3(256), 0, st, yb, xb,
                         (const bf16_t*)a_stack, (const bf16_t*)b_stack, scale, idx + b0, T, Din,
                         Dout, R, NA, cpg);
  }
  return hipGetLastError();
}
