// Token sampler for autoregressive generation: temperature, top-k, top-p and a seed PER
// ROW, one launch, one workgroup per row, every parameter read on the device (no host
// sync: capturable, and one capture serves every position). Semantics: ops/reference.py
// sample_logits.
//
//   logits [B, >= V] bf16, row b at logits + b * row_stride (any stride >= V, any 2-byte
//          alignment: decode_step's [:, :vocab_size] view of the padded LM-head output is
//          read in place)
//   temperature, top_p fp32 [B]; top_k, steps int32 [B]; seeds int64 [B]
//   done uint8 [B] or null, eos int (-1: none): a row with done[b] emits eos, a row that
//          draws eos sets done[b]
//   tok_out int64 [B]
//
// The row is read from global memory (L2 after the first pass) by 16-byte loads, four in
// flight per thread; a row of at most 8185 logits is read once and stays in registers.
// Rows that are not 16-byte aligned are read through the aligned slots that cover them, the
// elements outside [0, V) replaced by -inf, so no load leaves the 16-byte blocks that hold
// the row. (Holding GPT-2's whole row in registers, seven slots per thread, spilled to
// scratch at 1024 threads; staging it in LDS was not tried.)
//
// Everything after the maximum runs on INTEGERS. A logit is its order-preserving 16-bit key
// (-0 folded onto +0); its weight exp((x - max) / T) is rounded once to 2^-40 fixed point
// (the maximum weighs exactly 2^40, so a sum over 2^18 tokens stays below 2^59). Sums of
// such weights are exact and order-free, which makes the LDS histogram atomics (integer)
// and the cross-wave combines deterministic: the same inputs give the same token every run.
//
// Passes over the row (each skipped when its rule is off):
//   1. maximum key and the lowest index holding it (the greedy answer);
//   2. histograms over the key's high byte: counts (top-k) and fixed-point mass;
//   3. the same over the low byte inside the bucket that holds the k-th largest key:
//      the k-th key exactly (ties at it are kept), and the kept mass;
//   4. top-p: the walk over the mass histograms from the top finds the bucket where the
//      mass above reaches p * total, one more low-byte mass histogram inside it (the one of
//      pass 3 is reused when it is the same bucket) gives the threshold key;
//   5. index-order prefix scan of the kept weights up to the first index whose running sum
//      exceeds floor(u * total).
// Histogram counters are replicated kRep times (lane & (kRep - 1)) so that the many logits
// that share a high byte do not serialise on one LDS address.
#include "common.h"
#include "row_slots.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kRep = 16;
constexpr int kBins = 256;
constexpr int kMaxV = 1 << 18;
constexpr float kFixOne = 1099511627776.0f;  // 2^40

typedef unsigned long long u64;

struct SampleArgs {
  const bf16_t* logits;
  long row_stride;
  const float* temperature;
  const int* top_k;
  const float* top_p;
  const long long* seeds;
  const int* steps;
  unsigned char* done;
  int eos;
  long long* tok_out;
  int V;
};

// floor(r * t / 2^24) for r < 2^24, t < 2^63, without a 128-bit product
__device__ __forceinline__ u64 mul_shift24(u64 r, u64 t) {
  return r * (t >> 24) + ((r * (t & 0xffffffull)) >> 24);
}

__device__ __forceinline__ u64 splitmix64(u64 seed, u64 step) {
  u64 z = seed + (step + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ u64 shfl_down64(u64 v, int d) {
  const uint32_t lo = __shfl_down((uint32_t)v, d, 64);
  const uint32_t hi = __shfl_down((uint32_t)(v >> 32), d, 64);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 shfl_up64(u64 v, int d) {
  const uint32_t lo = __shfl_up((uint32_t)v, d, 64);
  const uint32_t hi = __shfl_up((uint32_t)(v >> 32), d, 64);
  return ((u64)hi << 32) | lo;
}

constexpr int kBatch = 4;

// Calls f(j, slot) for every slot of the row that this thread owns (j = tid, tid +
// kThreads, ...). R > 0: the row sits in registers, R slots per thread, the slots past the
// row's end all -inf; R == 0: any length, re-read from global memory (L2) on every pass,
// kBatch slots at a time (whole slots of -inf past the row's end).
template <int R, class F>
__device__ __forceinline__ void for_slots(const Row& row, const uint4* regs, F f) {
  if constexpr (R > 0) {
#pragma unroll
    for (int r = 0; r < R; ++r) f((int)threadIdx.x + r * kThreads, regs[r]);
  } else {
    const uint4 none = make_uint4(kNegInf2, kNegInf2, kNegInf2, kNegInf2);
    for (int j = threadIdx.x; j < row.nslots; j += kBatch * kThreads) {
      uint4 u[kBatch];  // kBatch loads in flight before the first use
#pragma unroll
      for (int i = 0; i < kBatch; ++i)
        u[i] = j + i * kThreads < row.nslots ? row.load(j + i * kThreads) : none;
#pragma unroll
      for (int i = 0; i < kBatch; ++i) f(j + i * kThreads, u[i]);
    }
  }
}

struct Shared {
  u64 mass[kBins * kRep];       // replicated histograms of one pass
  uint32_t cnt[kBins * kRep];
  u64 m1[kBins], m2[kBins];     // reduced mass: high-byte level, low-byte level
  uint32_t c1[kBins];           // reduced counts of the current level
  u64 red[kWaves];
  u64 bc_u64[2];                // broadcast slots
  int bc_int[2];
};

__device__ __forceinline__ u64 block_reduce_max(u64 v, Shared& s) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const u64 o = shfl_down64(v, d);
    if (lane + d < 64 && o > v) v = o;
  }
  if (lane == 0) s.red[w] = v;
  __syncthreads();
  u64 r = s.red[0];
#pragma unroll
  for (int i = 1; i < kWaves; ++i) r = s.red[i] > r ? s.red[i] : r;
  __syncthreads();
  return r;
}

__device__ __forceinline__ u64 block_reduce_sum(u64 v, Shared& s) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const u64 o = shfl_down64(v, d);
    if (lane + d < 64) v += o;
  }
  if (lane == 0) s.red[w] = v;
  __syncthreads();
  u64 r = 0;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) r += s.red[i];
  __syncthreads();
  return r;
}

__device__ __forceinline__ void zero_hists(Shared& s) {
  for (int i = threadIdx.x; i < kBins * kRep; i += kThreads) {
    s.mass[i] = 0;
    s.cnt[i] = 0;
  }
  __syncthreads();
}

// Sums the kRep copies of every bin into m[] (and c1[] when counts are wanted).
__device__ __forceinline__ void reduce_hists(Shared& s, u64* m, bool counts) {
  __syncthreads();
  if (threadIdx.x < kBins) {
    const int b = threadIdx.x;
    u64 a = 0;
    uint32_t c = 0;
#pragma unroll
    for (int r = 0; r < kRep; ++r) {
      a += s.mass[b * kRep + r];
      c += s.cnt[b * kRep + r];
    }
    m[b] = a;
    if (counts) s.c1[b] = c;
  }
  __syncthreads();
}

// Over h[0..255], S(b) = h[b] + ... + h[255]: the largest b with S(b) >= target, and
// above = S(b + 1). (b = 0, above = S(1) when no bucket reaches the target.) Runs on wave 0,
// lane l owning bins 4l..4l+3; the result is broadcast to the block. Contains block syncs:
// call it from uniform control flow.
template <class T>
__device__ __forceinline__ void suffix_find(const T* h, u64 target, Shared& s, int& bucket,
                                            u64& above) {
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    u64 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (u64)h[lane * 4 + j];
    const u64 own = v[0] + v[1] + v[2] + v[3];
    u64 x = own;  // inclusive suffix sum over the lanes
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const u64 o = shfl_down64(x, d);
      if (lane + d < 64) x += o;
    }
    u64 suf = x - own;  // bins of the higher lanes
    int best = -1;
    u64 best_above = 0;
#pragma unroll
    for (int j = 3; j >= 0; --j) {
      if (best < 0 && suf + v[j] >= target) {
        best = j;
        best_above = suf;
      }
      suf += v[j];
    }
    const u64 votes = __ballot(best >= 0);
    if (votes == 0) {
      if (lane == 0) {
        s.bc_int[0] = 0;
        s.bc_u64[0] = x - v[0];
      }
    } else if (lane == 63 - __clzll(votes)) {
      s.bc_int[0] = lane * 4 + best;
      s.bc_u64[0] = best_above;
    }
  }
  __syncthreads();
  bucket = s.bc_int[0];
  above = s.bc_u64[0];
  __syncthreads();
}

// Sum of h[0..255], broadcast. Block syncs inside.
__device__ __forceinline__ u64 total_of(const u64* h, Shared& s) {
  const u64 v = threadIdx.x < kBins ? h[threadIdx.x] : 0;
  return block_reduce_sum(v, s);
}

template <int R>
__global__ __launch_bounds__(kThreads) void sample_kernel(SampleArgs a) {
  __shared__ Shared s;
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int V = a.V;
  const bool use_eos = a.done != nullptr && a.eos >= 0;
  if (use_eos && a.done[b]) {  // block-uniform
    if (tid == 0) a.tok_out[b] = a.eos;
    return;
  }

  const bf16_t* rowp = a.logits + (long)b * a.row_stride;
  Row row;
  row.off = (int)(((uintptr_t)rowp >> 1) & 7);
  row.base = reinterpret_cast<const uint4*>(rowp - row.off);
  row.V = V;
  row.nslots = (row.off + V + 7) >> 3;

  uint4 regs[R > 0 ? R : 1];
  if constexpr (R > 0) {  // the whole row, every load in flight at once
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int j = tid + r * kThreads;
      regs[r] = j < row.nslots ? row.load(j)
                               : make_uint4(kNegInf2, kNegInf2, kNegInf2, kNegInf2);
    }
  }

  // ---- pass 1: the maximum, and the lowest index that holds it
  float m = -INFINITY;
  uint32_t mi = 0xffffffffu;
  for_slots<R>(row, regs, [&](int j, uint4 u) {
    float v[8];
    unpack8(u, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if (v[e] > m) {  // ascending indices: the first of equal values stays
        m = v[e];
        mi = (uint32_t)(j * 8 + e - row.off);
      }
    }
  });
  const u64 best = block_reduce_max(((u64)key_of_val(m) << 32) | (0xffffffffu - mi), s);
  const float maxv = val_of((uint32_t)(best >> 32));
  const uint32_t maxkey = (uint32_t)(best >> 32);
  long long tok = (long long)(0xffffffffu - (uint32_t)best);
  if (tok >= V) tok = 0;  // (no finite logit in the row)

  const float T = a.temperature[b];
  if (T > 0.f && maxv > -INFINITY && maxv < INFINITY) {  // block-uniform
    const float inv_t2 = (1.0f / T) * 1.4426950408889634f;
    const int k_arg = a.top_k[b];
    const float p_arg = a.top_p[b];
    const bool k_on = k_arg > 0 && k_arg < V;
    const bool p_on = p_arg < 1.0f;
    auto weight = [&](float v) -> u64 {
      return (u64)__float2ull_rn(__builtin_amdgcn_exp2f((v - maxv) * inv_t2) * kFixOne);
    };
    uint32_t thr = 0;  // keys >= thr are kept
    u64 total = 0;
    const int rep = tid & (kRep - 1);

    if (!k_on && !p_on) {
      u64 acc = 0;
      for_slots<R>(row, regs, [&](int, uint4 u) {
        float v[8];
        unpack8(u, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc += weight(v[e]);
      });
      total = block_reduce_sum(acc, s);
    } else {
      // ---- pass 2: high-byte histograms of every element
      zero_hists(s);
      for_slots<R>(row, regs, [&](int, uint4 u) {
        float v[8];
        unpack8(u, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int slot = (int)(key_of_val(v[e]) >> 8) * kRep + rep;
          if (k_on) atomicAdd(&s.cnt[slot], 1u);
          const u64 wt = weight(v[e]);
          if (wt) atomicAdd(&s.mass[slot], wt);
        }
      });
      reduce_hists(s, s.m1, k_on);

      int b1 = -1;  // the bucket that holds the k-th largest key
      if (k_on) {
        u64 above_cnt;
        suffix_find(s.c1, (u64)k_arg, s, b1, above_cnt);
        // ---- pass 3: low-byte histograms inside bucket b1
        zero_hists(s);
        for_slots<R>(row, regs, [&](int, uint4 u) {
          float v[8];
          unpack8(u, v);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const uint32_t key = key_of_val(v[e]);
            if ((int)(key >> 8) == b1) {
              const int slot = (int)(key & 0xffu) * kRep + rep;
              atomicAdd(&s.cnt[slot], 1u);
              atomicAdd(&s.mass[slot], weight(v[e]));
            }
          }
        });
        reduce_hists(s, s.m2, true);
        int c_k;
        u64 above2;
        suffix_find(s.c1, (u64)k_arg - above_cnt, s, c_k, above2);
        thr = ((uint32_t)b1 << 8) | (uint32_t)c_k;
        // what top-k dropped leaves the mass histograms
        if (tid < kBins) {
          if (tid < c_k) s.m2[tid] = 0;
          if (tid < b1) s.m1[tid] = 0;
        }
        __syncthreads();
        const u64 kept_b1 = total_of(s.m2, s);
        if (tid == 0) s.m1[b1] = kept_b1;
        __syncthreads();
      }
      total = total_of(s.m1, s);

      if (p_on) {
        // ---- pass 4: keep a key iff the kept mass above it is < p * total
        const u64 pr = p_arg > 0.f ? (u64)(p_arg * 16777216.0f) : 0;
        u64 P = mul_shift24(pr, total);
        if (P < 1) P = 1;  // the top value class always survives
        int bp;
        u64 above_m;
        suffix_find(s.m1, P, s, bp, above_m);
        if (bp != b1) {  // (bp > b1: every key of that bucket passed top-k)
          zero_hists(s);
          for_slots<R>(row, regs, [&](int, uint4 u) {
            float v[8];
            unpack8(u, v);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const uint32_t key = key_of_val(v[e]);
              if ((int)(key >> 8) == bp)
                atomicAdd(&s.mass[(int)(key & 0xffu) * kRep + rep], weight(v[e]));
            }
          });
          reduce_hists(s, s.m2, false);
        }
        int cp;
        u64 above_m2;
        suffix_find(s.m2, P - above_m, s, cp, above_m2);
        const uint32_t pkey = ((uint32_t)bp << 8) | (uint32_t)cp;
        thr = pkey > thr ? pkey : thr;
        total = above_m + above_m2 + s.m2[cp];
      }
    }
    if (thr > maxkey) thr = maxkey;
    // key order is value order, so the scan compares floats (keys up to -inf's: keep all)
    const float thr_v = thr <= 0x007fu ? -INFINITY : val_of(thr);

    // ---- pass 5: the first index whose running kept mass exceeds floor(u * total)
    const u64 r24 = splitmix64((u64)a.seeds[b], (u64)(long long)a.steps[b]) >> 40;
    const u64 target = mul_shift24(r24, total);
    const int lane = tid & 63, w = tid >> 6;
    if (tid == 0) s.bc_int[1] = -1;
    __syncthreads();
    u64 run = 0;  // mass of the tiles before this one
    auto tile = [&](int j, uint4 u) -> bool {  // true: the token is found (block-uniform)
      float v[8];
      unpack8(u, v);
      u64 wt[8];
      u64 own = 0;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        wt[e] = v[e] >= thr_v ? weight(v[e]) : 0;
        own += wt[e];
      }
      u64 inc = own;  // inclusive prefix over the wave, in lane order
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const u64 o = shfl_up64(inc, d);
        if (lane >= d) inc += o;
      }
      if (lane == 63) s.red[w] = inc;
      __syncthreads();
      u64 before = run, all = 0;
#pragma unroll
      for (int i = 0; i < kWaves; ++i) {
        if (i < w) before += s.red[i];
        all += s.red[i];
      }
      const u64 excl = before + inc - own;
      if (excl <= target && target < excl + own) {  // at most one thread of the block
        u64 c = excl;
        int hit = -1;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          c += wt[e];
          if (hit < 0 && c > target) hit = j * 8 + e - row.off;
        }
        s.bc_int[1] = hit;
      }
      __syncthreads();
      run += all;
      const bool found = s.bc_int[1] >= 0;  // read between two barriers
      __syncthreads();
      return found;
    };
    if constexpr (R > 0) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (r * kThreads >= row.nslots) break;
        if (tile(tid + r * kThreads, regs[r])) break;
      }
    } else {
      const uint4 none = make_uint4(kNegInf2, kNegInf2, kNegInf2, kNegInf2);
      uint4 cur = tid < row.nslots ? row.load(tid) : none;
      for (int j = tid; j - tid < row.nslots; j += kThreads) {
        const int jn = j + kThreads;  // the next tile's load flies during this tile
        const uint4 nxt = jn < row.nslots ? row.load(jn) : none;
        if (tile(j, cur)) break;
        cur = nxt;
      }
    }
    if (s.bc_int[1] >= 0) tok = s.bc_int[1];
  }

  if (tid == 0) {
    a.tok_out[b] = tok;
    if (use_eos && tok == a.eos) a.done[b] = 1;
  }
}

}  // namespace

// Largest vocabulary the kernel takes (the fixed-point sums are sized for it).
RA_EXPORT int ra_sample_logits_max_v() { return kMaxV; }

// One workgroup per row; see the head of this file. Runs on the caller's stream: no host
// synchronisation, no allocation, every per-row parameter is read on the device.
RA_EXPORT int ra_sample_logits(const void* logits, long row_stride, const float* temperature,
                               const int* top_k, const float* top_p, const long long* seeds,
                               const int* steps, unsigned char* done, int eos, long long* tok_out,
                               int B, int V, hipStream_t st) {
  if (B <= 0 || V <= 0 || V > kMaxV || row_stride < V) return hipErrorInvalidValue;
  if (!logits || !temperature || !top_k || !top_p || !seeds || !steps || !tok_out ||
      ((uintptr_t)logits & 1))
    return hipErrorInvalidValue;
  SampleArgs a;
  a.logits = (const bf16_t*)logits;
  a.row_stride = row_stride;
  a.temperature = temperature;
  a.top_k = top_k;
  a.top_p = top_p;
  a.seeds = seeds;
  a.steps = steps;
  a.done = done;
  a.eos = eos;
  a.tok_out = tok_out;
  a.V = V;
  // a row of at most one slot per thread (V <= 8185) stays in registers
  const int nslots = (V + 7 + 7) / 8;  // the most an unaligned row needs
  if (nslots <= kThreads)
    hipLaunchKernelGGL(sample_kernel<1>, dim3(B), dim3(kThreads), 0, st, a);
  else
    hipLaunchKernelGGL(sample_kernel<0>, dim3(B), dim3(kThreads), 0, st, a);
  return hipGetLastError();
}
