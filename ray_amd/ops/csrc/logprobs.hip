// Per-token log-probabilities: for every row of logits, the logprob of a given token under
// the row's own softmax and the top_n largest entries with theirs, one launch, one
// workgroup per row, every index read and bounds-checked on the device (no host sync:
// capturable, and one capture serves every position). Semantics: ops/reference.py
// token_logprobs.
//
//   logits [B, >= V] bf16, row b at logits + b * row_stride (any stride >= V, any 2-byte
//          alignment: the [:, :vocab_size] view of the padded LM-head output is read in
//          place through the aligned 16-byte slots that cover it, row_slots.h)
//   tok    int64 [B]; a token outside [0, V) gives lp = NaN
//   rows, cols int32 [B] or null, active uint8 [B] or null: row b's results go to entry
//          (rows[b], cols[b]) of the [R, cap] tables; null rows: b, null cols: 0. A row
//          with active[b] == 0 or an entry outside the tables exits at once, writing nothing
//   lp fp32 [R, cap]; top_ids int32 and top_lp fp32 [R, cap, top_n]
//
// Three steps, the row read twice (the second time from L2), kBatch 16-byte loads in flight:
//   1. the maximum, as a float max per thread, a wave shuffle and one LDS word per wave.
//      The top_n-th largest of the 16 wave maxima is a lower bound T of the row's top_n-th
//      largest value (top_n elements at least reach it).
//   2. the sum of exp(x - max) in sample.hip's fixed point: every weight is rounded once to
//      2^-40 and the sums are integer sums, exact and order-free, so a row's bits depend
//      neither on its alignment nor on B or its row index. In the same pass every thread
//      keeps the (at most 8) largest of its own elements that reach T, sorted, as 32-bit
//      words (order key << 16 | ~local count): eight registers updated by an unrolled
//      max/min chain, no runtime-indexed array. Few elements reach T (on random rows,
//      little more than the top_n themselves), so the chain runs rarely.
//   3. the select keeps the full (value descending, index ascending) order through the
//      64-bit key (order key << 32 | ~index): top_n rounds of a wave maximum over the
//      threads' heads give each wave's top_n, one barrier, then wave 0 takes top_n rounds
//      over those 16 * 8 words. lse = max + log(sum) is evaluated in fp64 by wave 0 and
//      every result is rounded to fp32 once.
// Resources (gfx950, -O3, -Rpass-analysis=kernel-resource-usage): 68 VGPRs, no scratch, no
// spill, 1216 bytes of LDS.
#include "common.h"
#include "row_slots.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxTop = 8;
constexpr int kMaxV = 1 << 18;
constexpr int kBatch = 4;
constexpr float kFixOne = 1099511627776.0f;  // 2^40

typedef unsigned long long u64;

struct LogprobArgs {
  const bf16_t* logits;
  long row_stride;
  const long long* tok;
  const int* rows;
  const int* cols;
  const unsigned char* active;
  float* lp;
  int* top_ids;
  float* top_lp;
  int V, top_n, R, cap;
};

struct Shared {
  float wmax[kWaves];
  u64 red[kWaves];
  u64 cand[kWaves * kMaxTop];
};

__device__ __forceinline__ u64 wave_max64(u64 v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)v, d, 64);
    const uint32_t hi = __shfl_xor((uint32_t)(v >> 32), d, 64);
    const u64 o = ((u64)hi << 32) | lo;
    v = o > v ? o : v;
  }
  return v;
}
__device__ __forceinline__ u64 wave_sum64(u64 v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)v, d, 64);
    const uint32_t hi = __shfl_xor((uint32_t)(v >> 32), d, 64);
    v += ((u64)hi << 32) | lo;
  }
  return v;
}

// Calls f(j, slot) for every slot j = tid, tid + kThreads, ... of the row, kBatch loads in
// flight before the first use (whole slots of -inf past the row's end).
template <class F>
__device__ __forceinline__ void for_slots(const Row& row, F f) {
  const uint4 none = make_uint4(kNegInf2, kNegInf2, kNegInf2, kNegInf2);
  for (int j = threadIdx.x; j < row.nslots; j += kBatch * kThreads) {
    uint4 u[kBatch];
#pragma unroll
    for (int i = 0; i < kBatch; ++i)
      u[i] = j + i * kThreads < row.nslots ? row.load(j + i * kThreads) : none;
#pragma unroll
    for (int i = 0; i < kBatch; ++i) f(j + i * kThreads, u[i]);
  }
}

__global__ __launch_bounds__(kThreads) void token_logprobs_kernel(LogprobArgs a) {
  __shared__ Shared s;
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int V = a.V, n = a.top_n;
  const int r = a.rows ? a.rows[b] : b;
  const int c = a.cols ? a.cols[b] : 0;
  if ((a.active && !a.active[b]) || r < 0 || r >= a.R || c < 0 || c >= a.cap)
    return;  // block-uniform

  const bf16_t* rowp = a.logits + (long)b * a.row_stride;
  const Row row = row_at(rowp, V);

  // ---- 1: the maximum, and the bound T for the top-n candidates
  float m = -INFINITY;
  for_slots(row, [&](int, uint4 u) {
    float v[8];
    unpack8(u, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) m = fmaxf(m, v[e]);
  });
  m = wave_max(m);
  if (lane == 0) s.wmax[w] = m;
  __syncthreads();
  float maxv = s.wmax[0];
#pragma unroll
  for (int i = 1; i < kWaves; ++i) maxv = fmaxf(maxv, s.wmax[i]);
  float thr = INFINITY;
  if (n > 0) {  // lanes 0..15 of every wave rank the wave maxima; rank n - 1 is T
    const int i = lane & (kWaves - 1);
    const float mine = s.wmax[i];
    int rank = 0;
#pragma unroll
    for (int j = 0; j < kWaves; ++j) {
      const float o = s.wmax[j];
      rank += (o > mine || (o == mine && j < i)) ? 1 : 0;
    }
    const u64 votes = __ballot(lane < kWaves && rank == n - 1);
    // (no lane votes when a wave maximum is NaN-ordered oddly: then every element is a
    // candidate, which is slower and as correct)
    thr = votes ? __shfl(mine, __ffsll((long long)votes) - 1, 64) : -INFINITY;
  }

  // ---- 2: fixed-point sum of exp(x - max); this thread's largest elements >= T
  uint32_t l[kMaxTop];
#pragma unroll
  for (int i = 0; i < kMaxTop; ++i) l[i] = 0;
  u64 acc = 0;
  for_slots(row, [&](int j, uint4 u) {
    float v[8];
    unpack8(u, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      acc += (u64)__float2ull_rn(
          __builtin_amdgcn_exp2f((v[e] - maxv) * 1.4426950408889634f) * kFixOne);
      if (v[e] >= thr) {
        const int i = j * 8 + e - row.off;
        // the count of this thread's elements so far rises with the index, so the word's
        // order is (value descending, index ascending) inside the thread
        uint32_t x = (key_of_val(v[e]) << 16) | (0xffffu - (uint32_t)((j >> 10) * 8 + e));
        if ((unsigned)i < (unsigned)V && x > l[kMaxTop - 1]) {
#pragma unroll
          for (int q = 0; q < kMaxTop; ++q) {
            const uint32_t hi = l[q] > x ? l[q] : x;
            x = l[q] > x ? x : l[q];
            l[q] = hi;
          }
        }
      }
    }
  });
  static_assert(kThreads == 1 << 10, "the slot's round is j >> 10");
  acc = wave_sum64(acc);
  if (lane == 0) s.red[w] = acc;

  // ---- 3: every wave's top n by the 64-bit key, then wave 0's rounds over them
  if (n > 0) {
#pragma unroll
    for (int q = 0; q < kMaxTop; ++q) {
      if (q >= n) {  // block-uniform: wave 0 reads every word
        if (lane == 0) s.cand[w * kMaxTop + q] = 0;
        continue;
      }
      u64 g = 0;
      if (l[0] != 0) {
        const uint32_t cnt = 0xffffu - (l[0] & 0xffffu);
        const uint32_t i = (uint32_t)((tid + (int)(cnt >> 3) * kThreads) * 8 + (int)(cnt & 7) -
                                      row.off);
        g = ((u64)(l[0] >> 16) << 32) | (0xffffffffu - i);
      }
      const u64 best = wave_max64(g);
      if (g == best && g != 0) {  // at most one lane: the index makes the keys distinct
#pragma unroll
        for (int p = 0; p + 1 < kMaxTop; ++p) l[p] = l[p + 1];
        l[kMaxTop - 1] = 0;
      }
      if (lane == 0) s.cand[w * kMaxTop + q] = best;
    }
  }
  __syncthreads();
  if (w != 0) return;

  u64 total = 0;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) total += s.red[i];
  // lse in fp64: max + ln(total * 2^-40) (a row of one element gives exactly max)
  const double lse = (double)maxv + (log2((double)total) - 40.0) * 0.6931471805599453;

  if (lane == 0) {
    const long long t = a.tok[b];
    float lp = __uint_as_float(0x7fc00000u);
    if (t >= 0 && t < V) lp = (float)((double)bf2f(rowp[t]) - lse);
    a.lp[(long)r * a.cap + c] = lp;
  }
  if (n > 0) {
    u64 k0 = s.cand[lane], k1 = s.cand[lane + 64];
    static_assert(kWaves * kMaxTop == 128, "two words per lane of wave 0");
    u64 mine = 0;
#pragma unroll
    for (int q = 0; q < kMaxTop; ++q) {
      if (q < n) {
        const u64 best = wave_max64(k0 > k1 ? k0 : k1);
        if (best != 0) {
          if (k0 == best) k0 = 0;
          else if (k1 == best) k1 = 0;
        }
        if (lane == q) mine = best;
      }
    }
    if (lane < n) {
      const uint32_t i = 0xffffffffu - (uint32_t)mine;
      const bool ok = mine != 0 && i < (uint32_t)V;
      const long at = ((long)r * a.cap + c) * n + lane;
      a.top_ids[at] = ok ? (int)i : -1;
      a.top_lp[at] = ok ? (float)((double)val_of((uint32_t)(mine >> 32)) - lse) : -INFINITY;
    }
  }
}

}  // namespace

RA_EXPORT int ra_token_logprobs_max_top() { return kMaxTop; }

// One workgroup per row; see the head of this file. Runs on the caller's stream: no host
// synchronisation, no allocation, no workspace, every index is read on the device.
RA_EXPORT int ra_token_logprobs(const void* logits, long row_stride, const long long* tok,
                                const int* rows, const int* cols, const unsigned char* active,
                                float* lp, int* top_ids, float* top_lp, int B, int V, int top_n,
                                int R, int cap, hipStream_t st) {
  if (B <= 0 || V <= 0 || V > kMaxV || row_stride < V || top_n < 0 || top_n > kMaxTop ||
      R <= 0 || cap <= 0)
    return hipErrorInvalidValue;
  if (!logits || !tok || !lp || ((uintptr_t)logits & 1) || (top_n > 0 && (!top_ids || !top_lp)))
    return hipErrorInvalidValue;
  if (!rows && R < B) return hipErrorInvalidValue;
  LogprobArgs a;
  a.logits = (const bf16_t*)logits;
  a.row_stride = row_stride;
  a.tok = tok;
  a.rows = rows;
  a.cols = cols;
  a.active = active;
  a.lp = lp;
  a.top_ids = top_ids;
  a.top_lp = top_lp;
  a.V = V;
  a.top_n = top_n;
  a.R = R;
  a.cap = cap;
  hipLaunchKernelGGL(token_logprobs_kernel, dim3(B), dim3(kThreads), 0, st, a);
  return hipGetLastError();
}
