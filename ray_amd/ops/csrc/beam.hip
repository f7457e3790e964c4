// Beam search, one step per token on the device: G groups (prompts) of W <= 8 beams, row
// r = g * W + w of the logits buffer and of the K/V cache. Four entry points, one launch each
// on the caller's stream, every index and length read and bounds-checked on the device: no
// host read, no allocation, no float atomics, capturable, one capture serves every step.
// Semantics: ops/reference.py beam_step / beam_kv_fork / beam_backtrace.
//
// ra_beam_topk, one workgroup of 1024 threads per row: the row's 2W largest logits (stored
// value descending, index ascending, -0 == +0: the token_logprobs order) with
// cand = score[r] + (x - lse), lse in fp64 from the 2^-40 fixed-point sum of logprobs.hip
// (integer sums: a row's bits depend on neither its alignment nor its batch-mates), the
// difference rounded to fp32 once, then one fp32 add. The bf16 row is read in place through
// row_slots.h, four 16-byte loads per lane in flight.
//   The select. logprobs.hip's eight-register chain per thread does not extend to 16 words
// without spilling, and a sort of per-wave lists needs 16 x 16 rounds. Here the full order
// is one 34-bit key per element, (16-bit value key, ~index), and the 2W-th largest key is
// found by a radix select over LDS integer histograms: the value key's high byte, then its
// low byte; only if more elements tie at that value than are wanted, the index's high and low
// nine bits among the ties (lowest index first). Every level is an LDS atomic increment per
// element and a 64-lane scan of the bins by wave 0; no private array is indexed at run time
// and nothing spills. Two things keep the levels cheap. (a) Only elements that reach T0, the
// 2W-th largest of the 16 wave maxima, take part: 2W elements reach T0, so the 2W largest all
// do, and on real rows few others. (b) The first pass (which also sums exp(x - max))
// compacts those elements as 64-bit keys into an LDS list; while it holds them all (2048),
// the later levels and the final gather walk the list and the row is read twice in all.
// A longer list (long runs of equal values) makes them walk the row again: slower, as exact.
// The elements at or above the threshold key are exactly the wanted ones (keys are
// distinct); they are gathered through an LDS counter and ranked by 16 lanes of wave 0.
//
// ra_beam_merge, one wave per group. The 2W * W <= 128 candidates sit two per lane as
// (order-preserving fp32 key << 32 | inverted (w, rank)); 2W wave-maximum rounds give the
// group's first 2W in (cand descending, w ascending, rank ascending) order. They are among
// the per-row lists because rounding is monotone within a row: lp = fl(x - lse) and
// cand = fl(score + lp) are non-decreasing in x, so an element outside its row's 2W largest
// has 2W row-mates that come before it in the group order (at least as large, and ahead of it
// in rank). Lane 0 then walks the 2W: an EOS candidate of rank < W becomes a finished
// hypothesis (cand / len_norm[t + 1], IEEE division, the table comes from the host: no powf),
// kept in the group's W-entry table if that has room or it beats the worst strictly; the first
// W others become the live beams, each in its parent's slot if that is still free, the rest
// in the lowest free slots (slot-stable: a surviving parent keeps its cache row).
//
// ra_beam_kv_fork: for every row with parent[r] != r copies positions [0, lens[r]) of cache
// row parent[r] onto row r, all layers, K and V, with kv_rows.h's kv_move_rows; grid
// (ceil(Tmax / 64), L * H, rows) as ra_kv_copy. Source and destination are the SAME tensors,
// which ra_kv_copy forbids. Disjointness: a row is written only by its own workgroups
// (destination r, once per (l, h, block)), and it is read only as parent[r'] of a row r' that
// has checked parent[parent[r']] == parent[r'], i.e. that the source is no destination of this
// launch. Hence no byte is both read and written, and no byte is written twice.
//
// ra_beam_backtrace: finalisation and read-out, one workgroup per group. Thread 0 offers the
// live beams of a group that is not done to a copy of the hypothesis table, one thread per
// returned hypothesis then follows par_hist / tok_hist backwards: a chain of dependent L2
// loads, once per call; at max_new_tokens = 1023 it takes 200 to 252 us (profiles/r20/beam.md).
// Resources (gfx950, -O3, -Rpass-analysis=kernel-resource-usage): beam_topk 114 VGPRs and
// 20816 bytes of LDS, beam_merge 15 and 320, beam_kv_fork 29 and none, beam_backtrace 18 and
// 132; no scratch and no spill in any of them.
#include "kv_rows.h"
#include "row_slots.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxW = 8;
constexpr int kMaxK = 2 * kMaxW;
constexpr int kMaxV = 1 << 18;
constexpr int kBatch = 4;
constexpr int kCap = 2048;
constexpr int kBins = 512;
constexpr uint32_t kNone = 0xffffffffu;
constexpr float kFixOne = 1099511627776.0f;  // 2^40
constexpr int kD = 64;

typedef unsigned long long u64;

static_assert(kMaxK <= kWaves, "T0 is the 2W-th largest of the wave maxima");
static_assert(kMaxV <= kBins * kBins, "two nine-bit levels cover an index");

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

// ------------------------------------------------------------------------------ beam_topk

struct TopkArgs {
  const bf16_t* logits;
  long row_stride;
  const float* score;
  const unsigned char* done;
  int* cand_tok;
  float* cand;
  int V, W;
};

struct TopkShared {
  float wmax[kWaves];
  u64 red[kWaves];
  uint32_t hist[2][kBins];
  u64 list[kCap];
  u64 top[kMaxK];
  uint32_t ncand, ntop;
  uint32_t sel_bin, sel_before;
};

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

// The 64-bit key of element i with value v: distinct per element, ordered by (value
// descending, index ascending) when compared as integers, never 0.
__device__ __forceinline__ u64 entry_of(float v, int i) {
  return ((u64)key_of_val(v) << 32) | (0xffffffffu - (uint32_t)i);
}

// Calls f(entry) for every element of the row that reaches thr: from the compacted list when
// it holds them all, from the row otherwise.
template <class F>
__device__ __forceinline__ void for_cands(const Row& row, const TopkShared& s, bool compact,
                                          float thr, F f) {
  if (compact) {
    for (uint32_t i = threadIdx.x; i < s.ncand; i += kThreads) f(s.list[i]);
  } else {
    for_slots(row, [&](int j, uint4 u) {
      float v[8];
      unpack8(u, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int i = j * 8 + e - row.off;
        if (v[e] >= thr && (unsigned)i < (unsigned)row.V) f(entry_of(v[e], i));
      }
    });
  }
}

// Wave 0: the first bin, walking hist[0 .. NB) downwards (DESC) or upwards, at which the
// running count reaches need (>= 1), and the count before it; kNone and the total if it
// never does. Results in s.sel_bin / s.sel_before; the caller puts barriers around the call.
template <int NB, bool DESC>
__device__ __forceinline__ void pick_bin(TopkShared& s, const uint32_t* hist, uint32_t need) {
  if (threadIdx.x >= 64) return;
  constexpr int P = NB / 64;
  const int lane = threadIdx.x;
  uint32_t c[P], tot = 0;
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const int pos = lane * P + i;
    c[i] = hist[DESC ? NB - 1 - pos : pos];
    tot += c[i];
  }
  uint32_t inc = tot;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(inc, d, 64);
    if (lane >= d) inc += o;
  }
  uint32_t run = inc - tot;
#pragma unroll
  for (int i = 0; i < P; ++i) {
    if (run < need && need <= run + c[i]) {  // true for one (lane, i) at the most
      const int pos = lane * P + i;
      s.sel_bin = DESC ? NB - 1 - pos : pos;
      s.sel_before = run;
    }
    run += c[i];
  }
  if (lane == 63 && inc < need) {
    s.sel_bin = kNone;
    s.sel_before = inc;
  }
}

__global__ __launch_bounds__(kThreads) void beam_topk_kernel(TopkArgs a) {
  __shared__ TopkShared s;
  const int r = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int V = a.V, K = 2 * a.W;
  if (a.done[r / a.W]) return;  // block-uniform: the merge does not read a done group's rows

  const bf16_t* rowp = a.logits + (long)r * a.row_stride;
  const Row row = row_at(rowp, V);
  (&s.hist[0][0])[tid] = 0;
  static_assert(2 * kBins == kThreads, "one histogram word per thread");
  if (tid == 0) s.ncand = s.ntop = 0;

  // ---- the maximum, and the bound T0 for the candidates
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
  float thr;
  {  // lanes 0..15 of every wave rank the wave maxima; rank K - 1 is T0
    const int i = lane & (kWaves - 1);
    const float mine = s.wmax[i];
    int rank = 0;
#pragma unroll
    for (int j = 0; j < kWaves; ++j) {
      const float o = s.wmax[j];
      rank += (o > mine || (o == mine && j < i)) ? 1 : 0;
    }
    const u64 votes = __ballot(lane < kWaves && rank == K - 1);
    thr = votes ? __shfl(mine, __ffsll((long long)votes) - 1, 64) : -INFINITY;
  }

  // ---- fixed-point sum of exp(x - max); the candidates' list and first histogram
  u64 acc = 0;
  for_slots(row, [&](int j, uint4 u) {
    float v[8];
    unpack8(u, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      acc += (u64)__float2ull_rn(
          __builtin_amdgcn_exp2f((v[e] - maxv) * 1.4426950408889634f) * kFixOne);
      const int i = j * 8 + e - row.off;
      if (v[e] >= thr && (unsigned)i < (unsigned)V) {
        const u64 x = entry_of(v[e], i);
        atomicAdd(&s.hist[0][(uint32_t)(x >> 40)], 1u);
        const uint32_t at = atomicAdd(&s.ncand, 1u);
        if (at < (uint32_t)kCap) s.list[at] = x;
      }
    }
  });
  acc = wave_sum64(acc);
  if (lane == 0) s.red[w] = acc;
  __syncthreads();
  const bool compact = s.ncand <= (uint32_t)kCap;

  // ---- the threshold key: the K-th largest entry (0: fewer than K elements, all are taken)
  u64 cut = 0;
  pick_bin<256, true>(s, s.hist[0], (uint32_t)K);
  __syncthreads();
  const uint32_t b1 = s.sel_bin, above1 = s.sel_before;
  if (b1 != kNone) {  // block-uniform, as every branch below
    for_cands(row, s, compact, thr, [&](u64 x) {
      if ((uint32_t)(x >> 40) == b1) atomicAdd(&s.hist[1][(uint32_t)(x >> 32) & 255u], 1u);
    });
    __syncthreads();
    pick_bin<256, true>(s, s.hist[1], (uint32_t)K - above1);
    __syncthreads();
    const uint32_t b2 = s.sel_bin;  // (a bin: hist[1] holds hist[0][b1] >= K - above1 elements)
    const uint32_t key = (b1 << 8) | b2;
    const uint32_t above = above1 + s.sel_before;
    const uint32_t ties = s.hist[1][b2 & 255u];
    cut = (u64)key << 32;
    if (above + ties > (uint32_t)K) {
      // more ties at the threshold value than places: the K - above with the lowest indices
      __syncthreads();
      (&s.hist[0][0])[tid] = 0;
      __syncthreads();
      for_cands(row, s, compact, thr, [&](u64 x) {
        if ((uint32_t)(x >> 32) == key) atomicAdd(&s.hist[0][(0xffffffffu - (uint32_t)x) >> 9], 1u);
      });
      __syncthreads();
      pick_bin<kBins, false>(s, s.hist[0], (uint32_t)K - above);
      __syncthreads();
      const uint32_t i1 = s.sel_bin, before1 = s.sel_before;
      for_cands(row, s, compact, thr, [&](u64 x) {
        const uint32_t i = 0xffffffffu - (uint32_t)x;
        if ((uint32_t)(x >> 32) == key && (i >> 9) == i1) atomicAdd(&s.hist[1][i & 511u], 1u);
      });
      __syncthreads();
      pick_bin<kBins, false>(s, s.hist[1], (uint32_t)K - above - before1);
      __syncthreads();
      cut |= 0xffffffffu - ((i1 << 9) | s.sel_bin);
    }
  }

  // ---- gather the entries at or above the threshold (at most K), rank them, write
  for_cands(row, s, compact, thr, [&](u64 x) {
    if (x >= cut) {
      const uint32_t at = atomicAdd(&s.ntop, 1u);
      if (at < (uint32_t)kMaxK) s.top[at] = x;
    }
  });
  __syncthreads();
  if (tid >= kMaxK) return;
  const int n = min((int)s.ntop, K);
  const u64 mine = tid < n ? s.top[tid] : 0;
  int rank = 0;
#pragma unroll
  for (int j = 0; j < kMaxK; ++j) rank += (j < n && s.top[j] > mine) ? 1 : 0;
  u64 total = 0;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) total += s.red[i];
  // lse in fp64: max + ln(total * 2^-40), as logprobs.hip
  const double lse = (double)maxv + (log2((double)total) - 40.0) * 0.6931471805599453;
  const long out = (long)r * K;
  if (tid < n) {
    const float lp = (float)((double)val_of((uint32_t)(mine >> 32)) - lse);
    a.cand_tok[out + rank] = (int)(0xffffffffu - (uint32_t)mine);
    a.cand[out + rank] = a.score[r] + lp;
  } else if (tid < K) {
    a.cand_tok[out + tid] = -1;  // ranks n .. K - 1: the row has fewer than K elements
    a.cand[out + tid] = -INFINITY;
  }
}

// ----------------------------------------------------------------------------- beam_merge

struct BeamState {
  const int* cand_tok;
  const float* cand;
  const float* len_norm;  // [max_new + 1]
  long long* tok;         // [N] the next decode_step input
  int* parent;            // [N]
  float* score;           // [N]
  int* tok_hist;          // [max_new, N]
  int* par_hist;          // [max_new, N]
  float* hyp_score;       // [G, W]
  int* hyp_step;
  int* hyp_par;
  int* hyp_ord;
  int* hyp_n;             // [G] hypotheses accepted so far
  unsigned char* done;    // [G]
  int* step;              // [G]
  int G, W, max_new, eos, early;
};

// The group's W-entry hypothesis table with n accepted so far: a new one takes a free entry,
// or the worst one's (lowest score, the latest among equals) if it is strictly better.
// Returns the new n.
__device__ __forceinline__ int hyp_offer(float* sc, int* st, int* pa, int* od, int n, int W,
                                         float score, int step, int par) {
  int at = n;
  if (n >= W) {
    at = 0;
    for (int i = 1; i < W; ++i)
      if (sc[i] < sc[at] || (sc[i] == sc[at] && od[i] > od[at])) at = i;
    if (!(score > sc[at])) return n;
  }
  sc[at] = score;
  st[at] = step;
  pa[at] = par;
  od[at] = n;
  return n + 1;
}

__device__ __forceinline__ uint32_t f32_key(float v) {
  uint32_t u = __float_as_uint(v);
  if (u == 0x80000000u) u = 0;  // -0 == +0
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(64) void beam_merge_kernel(BeamState a) {
  __shared__ int c_tok[kMaxK], c_w[kMaxK], l_tok[kMaxW], l_w[kMaxW], l_slot[kMaxW];
  __shared__ float c_val[kMaxK], l_val[kMaxW];
  const int g = blockIdx.x, lane = threadIdx.x;
  const int W = a.W, K = 2 * W, N = a.G * W, base = g * W;
  const int t = a.step[g];
  if (a.done[g] || t < 0 || t >= a.max_new) {  // a done group's beams emit EOS, nothing else
    if (lane < W) {
      a.tok[base + lane] = a.eos;
      a.parent[base + lane] = base + lane;
    }
    return;
  }

  // ---- the group's first 2W candidates
  u64 k0 = 0, k1 = 0;
  if (lane < W * K)
    k0 = ((u64)f32_key(a.cand[(long)base * K + lane]) << 32) |
         (255u - (uint32_t)((lane / K) * 16 + lane % K));
  if (lane + 64 < W * K)
    k1 = ((u64)f32_key(a.cand[(long)base * K + lane + 64]) << 32) |
         (255u - (uint32_t)(((lane + 64) / K) * 16 + (lane + 64) % K));
  u64 mine = 0;
#pragma unroll
  for (int q = 0; q < kMaxK; ++q) {
    if (q < K) {
      const u64 best = wave_max64(k0 > k1 ? k0 : k1);
      if (best != 0) {
        if (k0 == best) k0 = 0;
        else if (k1 == best) k1 = 0;
      }
      if (lane == q) mine = best;
    }
  }
  if (lane < K) {
    const uint32_t wr = 255u - ((uint32_t)mine & 255u);
    const int w = min((int)(wr >> 4), W - 1), rank = min((int)(wr & 15u), K - 1);
    const long at = (long)(base + w) * K + rank;
    c_tok[lane] = mine != 0 ? a.cand_tok[at] : -1;
    c_val[lane] = a.cand[at];
    c_w[lane] = w;
  }
  __syncthreads();
  if (lane != 0) return;

  // ---- the walk
  float* hs = a.hyp_score + (long)g * W;
  int* hst = a.hyp_step + (long)g * W;
  int* hp = a.hyp_par + (long)g * W;
  int* ho = a.hyp_ord + (long)g * W;
  const float norm = a.len_norm[t + 1];
  int n = a.hyp_n[g], live = 0;
  for (int q = 0; q < K; ++q) {
    const int tk = c_tok[q];
    if (tk < 0) continue;  // the padding of a row with fewer than 2W elements
    if (tk == a.eos) {
      if (q < W) n = hyp_offer(hs, hst, hp, ho, n, W, __fdiv_rn(c_val[q], norm), t, base + c_w[q]);
    } else if (live < W) {
      l_tok[live] = tk;
      l_val[live] = c_val[q];
      l_w[live] = c_w[q];
      ++live;
    }
  }
  a.hyp_n[g] = n;

  // ---- slot-stable placement
  uint32_t used = 0;
  for (int i = 0; i < live; ++i) {
    const bool own = !((used >> l_w[i]) & 1u);
    l_slot[i] = own ? l_w[i] : -1;
    if (own) used |= 1u << l_w[i];
  }
  for (int i = 0; i < live; ++i) {
    if (l_slot[i] < 0) {
      l_slot[i] = __ffs((int)~used) - 1;  // live <= W: a slot below W is free
      used |= 1u << l_slot[i];
    }
    const int r = base + l_slot[i];
    a.tok[r] = l_tok[i];
    a.parent[r] = base + l_w[i];
    a.score[r] = l_val[i];
    a.tok_hist[(long)t * N + r] = l_tok[i];
    a.par_hist[(long)t * N + r] = base + l_w[i];
  }
  for (int w = 0; w < W; ++w) {
    if ((used >> w) & 1u) continue;  // fewer than W candidates: a dead beam
    const int r = base + w;
    a.tok[r] = a.eos;
    a.parent[r] = r;
    a.score[r] = -INFINITY;
    a.tok_hist[(long)t * N + r] = a.eos;
    a.par_hist[(long)t * N + r] = r;
  }

  // ---- done?
  if (n >= W) {
    bool done = a.early != 0;
    if (!done) {
      float worst = hs[0];
      for (int i = 1; i < W; ++i) worst = fminf(worst, hs[i]);
      done = live == 0 || worst >= __fdiv_rn(l_val[0], norm);
    }
    if (done) a.done[g] = 1;
  }
  a.step[g] = t + 1;
}

// --------------------------------------------------------------------------- beam_kv_fork

// sk / dk (and sv / dv) are ONE tensor. The qualifiers hold all the same: what a thread writes
// through dk (row r) it never reads through sk (row p != r); see the head of this file.
__global__ __launch_bounds__(kKvThreads) void beam_kv_fork_kernel(
    const bf16_t* __restrict__ sk, const bf16_t* __restrict__ sv, bf16_t* __restrict__ dk,
    bf16_t* __restrict__ dv, const int* __restrict__ parent, const int* __restrict__ lens, int H,
    int S, int Tmax) {
  const int r = blockIdx.z, l = blockIdx.y / H, h = blockIdx.y % H;
  const int p = parent[r], len = lens[r];
  if (p == r || p < 0 || p >= S || len <= 0 || len > Tmax) return;
  if (parent[p] != p) return;  // the source is itself a destination
  const int t0 = blockIdx.x * kKvBlockRows;
  if (t0 >= len) return;
  const int c = threadIdx.x & 7;
  const long src0 = ((((long)l * S + p) * H + h) * Tmax) * kD + c * 8;
  const long dst0 = ((((long)l * S + r) * H + h) * Tmax) * kD + c * 8;
  kv_move_rows(sk + src0, sv + src0, kD, dk + dst0, dv + dst0, t0, len);
}

// ------------------------------------------------------------------------- beam_backtrace

struct TraceArgs {
  BeamState s;
  long long* out;  // [G, R, max_new]
  float* out_score;
  int* out_len;
  int R;
};

__global__ __launch_bounds__(64) void beam_backtrace_kernel(TraceArgs b) {
  __shared__ float sc[kMaxW];
  __shared__ int st[kMaxW], pa[kMaxW], od[kMaxW], held;
  const BeamState& a = b.s;
  const int g = blockIdx.x, j = threadIdx.x;
  const int W = a.W, N = a.G * W, base = g * W;
  const int len = max(0, min(a.step[g], a.max_new));  // the steps this group has taken
  if (j == 0) {
    int n = max(0, min(a.hyp_n[g], 1 << 30));
    for (int i = 0; i < min(n, W); ++i) {
      sc[i] = a.hyp_score[(long)g * W + i];
      st[i] = a.hyp_step[(long)g * W + i];
      pa[i] = a.hyp_par[(long)g * W + i];
      od[i] = a.hyp_ord[(long)g * W + i];
    }
    if (!a.done[g] && len > 0)
      for (int w = 0; w < W; ++w)
        n = hyp_offer(sc, st, pa, od, n, W, __fdiv_rn(a.score[base + w], a.len_norm[len]), len,
                      base + w);
    held = min(n, W);
  }
  __syncthreads();
  if (j >= b.R) return;
  long long* out = b.out + ((long)g * b.R + j) * a.max_new;
  int at = -1;  // the hypothesis of rank j by (score descending, insertion ascending)
  for (int i = 0; i < held; ++i) {
    int rank = 0;
    for (int q = 0; q < held; ++q)
      rank += (sc[q] > sc[i] || (sc[q] == sc[i] && od[q] < od[i])) ? 1 : 0;
    if (rank == j) at = i;
  }
  int n_tok = 0;
  float score = -INFINITY;
  if (at >= 0) {
    const int s = max(0, min(st[at], len));
    score = sc[at];
    n_tok = s < len ? s + 1 : len;  // a hypothesis that ended with EOS counts it
    int p = pa[at];
    for (int i = s - 1; i >= 0; --i) {
      if (p < base || p >= base + W) p = base;  // (never in a table this file wrote)
      out[i] = a.tok_hist[(long)i * N + p];
      p = a.par_hist[(long)i * N + p];
    }
  }
  for (int i = at >= 0 ? max(0, min(st[at], len)) : 0; i < a.max_new; ++i) out[i] = a.eos;
  b.out_score[(long)g * b.R + j] = score;
  b.out_len[(long)g * b.R + j] = n_tok;
}

bool state_ok(const BeamState& a) {
  return a.G > 0 && a.W >= 1 && a.W <= kMaxW && a.max_new >= 1 && a.max_new <= (1 << 20) &&
         (long)a.G * a.W <= (1 << 20) && a.eos >= 0 && a.len_norm && a.tok && a.parent &&
         a.score && a.tok_hist && a.par_hist && a.hyp_score && a.hyp_step && a.hyp_par &&
         a.hyp_ord && a.hyp_n && a.done && a.step;
}

}  // namespace

RA_EXPORT int ra_beam_max() { return kMaxW; }

// The two launches of a beam step; the state is the flat list of ops/functional.py's
// beam_state. Runs on the caller's stream: no host synchronisation, no allocation.
RA_EXPORT int ra_beam_step(const void* logits, long row_stride, int V, int* cand_tok, float* cand,
                           const float* len_norm, long long* tok, int* parent, float* score,
                           int* tok_hist, int* par_hist, float* hyp_score, int* hyp_step,
                           int* hyp_par, int* hyp_ord, int* hyp_n, unsigned char* done, int* step,
                           int G, int W, int max_new, int eos, int early, hipStream_t st) {
  BeamState a{cand_tok, cand,     len_norm, tok,     parent,  score, tok_hist, par_hist, hyp_score,
              hyp_step, hyp_par, hyp_ord,  hyp_n,   done,    step,  G,        W,        max_new,
              eos,      early};
  if (!state_ok(a) || !logits || ((uintptr_t)logits & 1) || !cand_tok || !cand || V <= 0 ||
      V > kMaxV || row_stride < V)
    return hipErrorInvalidValue;
  TopkArgs k{(const bf16_t*)logits, row_stride, score, done, cand_tok, cand, V, W};
  hipLaunchKernelGGL(beam_topk_kernel, dim3(G * W), dim3(kThreads), 0, st, k);
  hipLaunchKernelGGL(beam_merge_kernel, dim3(G), dim3(64), 0, st, a);
  return hipGetLastError();
}

// k, v [L, S, H, Tmax, 64] bf16, 16-byte aligned, written in place; parent, lens int32 [S].
RA_EXPORT int ra_beam_kv_fork(void* k, void* v, const int* parent, const int* lens, int L, int H,
                              int S, int Tmax, hipStream_t st) {
  if (L <= 0 || H <= 0 || S <= 0 || Tmax <= 0 || S > 65535 || (long)L * H > 65535 ||
      Tmax > (1 << 22) || !parent || !lens || !k || !v || (((uintptr_t)k | (uintptr_t)v) & 15))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(beam_kv_fork_kernel, dim3((Tmax + kKvBlockRows - 1) / kKvBlockRows, L * H, S),
                     dim3(kKvThreads), 0, st, (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)k,
                     (bf16_t*)v, parent, lens, H, S, Tmax);
  return hipGetLastError();
}

// out int64 [G, R, max_new], out_score fp32 [G, R], out_len int32 [G, R]; the state is read only.
RA_EXPORT int ra_beam_backtrace(const float* len_norm, const float* score, const int* tok_hist,
                                const int* par_hist, const float* hyp_score, const int* hyp_step,
                                const int* hyp_par, const int* hyp_ord, const int* hyp_n,
                                const unsigned char* done, const int* step, long long* out,
                                float* out_score, int* out_len, int G, int W, int max_new, int eos,
                                int R, hipStream_t st) {
  if (G <= 0 || W < 1 || W > kMaxW || R < 1 || R > W || max_new < 1 || max_new > (1 << 20) ||
      (long)G * W > (1 << 20) || eos < 0 || !len_norm || !score || !tok_hist || !par_hist ||
      !hyp_score || !hyp_step || !hyp_par || !hyp_ord || !hyp_n || !done || !step || !out ||
      !out_score || !out_len)
    return hipErrorInvalidValue;
  TraceArgs b;
  b.s = BeamState{nullptr,
                  nullptr,
                  len_norm,
                  nullptr,
                  nullptr,
                  const_cast<float*>(score),
                  const_cast<int*>(tok_hist),
                  const_cast<int*>(par_hist),
                  const_cast<float*>(hyp_score),
                  const_cast<int*>(hyp_step),
                  const_cast<int*>(hyp_par),
                  const_cast<int*>(hyp_ord),
                  const_cast<int*>(hyp_n),
                  const_cast<unsigned char*>(done),
                  const_cast<int*>(step),
                  G,
                  W,
                  max_new,
                  eos,
                  0};
  b.out = out;
  b.out_score = out_score;
  b.out_len = out_len;
  b.R = R;
  hipLaunchKernelGGL(beam_backtrace_kernel, dim3(G), dim3(64), 0, st, b);
  return hipGetLastError();
}
