// Logit processors of the GPT-2 serving stack: repetition / presence / frequency penalties,
// logit bias and a minimum length before EOS, applied IN PLACE to rows of logits as a
// function of each row's own token history and per-slot parameters. One launch, one
// workgroup per logits row, every index and length read and bounds-checked on the device
// (no host read, no workspace, no atomic on global memory: capturable, and one capture
// serves every position). Semantics: ops/reference.py logit_process, bit for bit.
//
//   logits [B, >= V] bf16, row b at logits + b * row_stride (any stride >= V, any 2-byte
//          alignment: the [:, :vocab_size] view of the padded LM-head output in place)
//   rows int32 [B] or null (b): the context row r of logits row b; active uint8 [B] or null
//   prompt int32 [R, P], prompt_len int32 [R]; out int64 [R, cap], n_out int32 [R]
//   extra int64 [B, W] or null, n_extra int32 [B]: the tokens after out[r, :n_out[r]]
//   repetition, presence, frequency fp32 [R]; min_new int32 [R]
//   bias_ids int32 [R, NB], bias_vals fp32 [R, NB], n_bias int32 [R]; eos (< 0: none)
//
// A row with active[b] == 0, r outside [0, R), a length outside its table or all-neutral
// parameters exits at once and keeps its bytes. Token ids outside [0, V) are ignored.
//
// The work is sparse (a few hundred named tokens against 50257 columns), so the row is
// never streamed. The one hazard is a token that is named many times (in the history, in
// the bias list, as EOS): its element must be read raw and written exactly once. So:
//   1. the workgroup builds the set of distinct named tokens in LDS, an open-addressing
//      table (linear probing, multiplicative hash) of kSlots = 2 * kMaxContext keys, never
//      more than half full. A key is claimed with an integer atomicCAS; its word of facts
//      is built with integer atomicAdd (bits 0..15: occurrences among the generated tokens)
//      and atomicOr (bit 16: in the prompt, bit 17: EOS banned, bits 20..26: 1 + the index
//      in the bias list). Integer LDS atomics are exact and order-free: the slot a token
//      lands in may differ from run to run, its word may not. The bias list is at most one
//      wave wide: wave 0 holds it in a register per lane and a lane whose id occurs at a
//      lower lane stands back (64 shuffles), so the lowest index wins without a minimum.
//   2. after ONE barrier the lanes stride over the table; each occupied entry does one
//      2-byte global load, the fp32 arithmetic of the reference with every step rounded on
//      its own (no contraction: the pragma below; IEEE division) and one 2-byte global
//      store. Entries are independent, so the loads are in flight together. A NaN result
//      is stored as the canonical quiet NaN, as the reference does.
// Resources (gfx950, -O3, -Rpass-analysis=kernel-resource-usage): 21 VGPRs, no scratch, no
// spill, 65536 bytes of LDS (two workgroups per CU). Measured: profiles/r17/logit_process.md.
#include "common.h"

namespace {

constexpr int kThreads = 512;
constexpr int kMaxBias = 64;         // one wave
constexpr int kMaxContext = 4096;    // P + cap + W + NB + 1, by the tables' shapes
constexpr int kSlots = 2 * kMaxContext;
constexpr int kHashShift = 32 - 13;  // log2(kSlots) = 13
constexpr int kMaxV = 1 << 18;
constexpr int kEmpty = -1;
constexpr uint32_t kCountMask = 0xffffu, kInPrompt = 1u << 16, kBanned = 1u << 17;
constexpr int kBiasShift = 20;
static_assert(kSlots == 1 << 13, "the hash keeps 13 bits");
static_assert(kMaxContext < (int)kCountMask, "a count fits its field");
static_assert(kMaxBias <= 64 && kMaxBias < (1 << (27 - kBiasShift)), "one wave, seven bits");

struct ProcArgs {
  bf16_t* logits;
  long row_stride;
  const int* rows;
  const unsigned char* active;
  const int* prompt;
  const int* prompt_len;
  const long long* out;
  const int* n_out;
  const long long* extra;
  const int* n_extra;
  const float* repetition;
  const float* presence;
  const float* frequency;
  const int* min_new;
  const int* bias_ids;
  const float* bias_vals;
  const int* n_bias;
  int V, R, P, cap, W, NB, eos;
};

struct Table {
  int key[kSlots];
  uint32_t fact[kSlots];
};

// The entry of token v (0 <= v < V), claimed if new. The table is never full, so the probe
// ends; no lane waits for another.
__device__ __forceinline__ int entry_of(Table& t, int v) {
  uint32_t s = ((uint32_t)v * 2654435761u) >> kHashShift;
  for (;;) {
    const int prev = atomicCAS(&t.key[s], kEmpty, v);
    if (prev == kEmpty || prev == v) return (int)s;
    s = (s + 1) & (kSlots - 1);
  }
}

__device__ __forceinline__ float processed(float x, uint32_t fact, float rp, float pp, float fp,
                                           const float* bias_vals) {
#pragma clang fp contract(off)
  const uint32_t cnt = fact & kCountMask;
  if (cnt != 0 || (fact & kInPrompt)) x = x > 0.f ? x / rp : x * rp;
  if (cnt != 0) {
    const float f = fp * (float)cnt;
    x = x - f;
    x = x - pp;
  }
  const uint32_t bi = (fact >> kBiasShift) & 0x7fu;
  if (bi != 0) x = x + bias_vals[bi - 1];
  if (fact & kBanned) x = -INFINITY;
  return x;
}

__global__ __launch_bounds__(kThreads) void logit_process_kernel(ProcArgs a) {
  __shared__ Table t;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int V = a.V;
  // ---- the row's context, checked before it addresses anything (block-uniform)
  if (a.active && !a.active[b]) return;
  const int r = a.rows ? a.rows[b] : b;
  if (r < 0 || r >= a.R) return;
  const int pl = a.prompt_len[r], no = a.n_out[r], nb = a.n_bias[r];
  const int ne = a.extra ? a.n_extra[b] : 0;
  if (pl < 0 || pl > a.P || no < 0 || no > a.cap || ne < 0 || ne > a.W || nb < 0 || nb > a.NB)
    return;
  const float rp = a.repetition[r], pp = a.presence[r], fp = a.frequency[r];
  const int mn = a.min_new[r];
  if (rp == 1.f && pp == 0.f && fp == 0.f && nb == 0 && mn == 0) return;  // neutral

  for (int i = tid; i < kSlots; i += kThreads) {
    t.key[i] = kEmpty;
    t.fact[i] = 0;
  }
  __syncthreads();

  // ---- 1: the distinct named tokens and what names them
  const int* prow = a.prompt + (long)r * a.P;
  for (int i = tid; i < pl; i += kThreads) {
    const int v = prow[i];
    if (v >= 0 && v < V) atomicOr(&t.fact[entry_of(t, v)], kInPrompt);
  }
  const long long* orow = a.out + (long)r * a.cap;
  const long long* erow = a.extra ? a.extra + (long)b * a.W : nullptr;
  for (int i = tid; i < no + ne; i += kThreads) {
    const long long v = i < no ? orow[i] : erow[i - no];
    if (v >= 0 && v < V) atomicAdd(&t.fact[entry_of(t, (int)v)], 1u);
  }
  if (tid < 64) {  // wave 0: the bias list, the lowest index of an id wins
    const int id = tid < nb ? a.bias_ids[(long)r * a.NB + tid] : -1;
    bool first = id >= 0 && id < V;
    for (int j = 0; j < kMaxBias; ++j) {
      const int o = __shfl(id, j, 64);
      if (j < tid && o == id) first = false;
    }
    if (first) atomicOr(&t.fact[entry_of(t, id)], (uint32_t)(tid + 1) << kBiasShift);
  }
  if (tid == 64 && a.eos >= 0 && a.eos < V && (long)no + ne < (long)mn)
    atomicOr(&t.fact[entry_of(t, a.eos)], kBanned);
  __syncthreads();

  // ---- 2: every named element once: load, the rules, store
  bf16_t* rowp = a.logits + (long)b * a.row_stride;
  const float* bv = a.bias_vals + (long)r * a.NB;
  for (int i = tid; i < kSlots; i += kThreads) {
    const int v = t.key[i];
    if (v == kEmpty) continue;
    const float x = processed(bf2f(rowp[v]), t.fact[i], rp, pp, fp, bv);
    rowp[v] = x != x ? (bf16_t)0x7fc0 : f2bf(x);
  }
}

}  // namespace

RA_EXPORT int ra_logit_process_max_bias() { return kMaxBias; }
RA_EXPORT int ra_logit_process_max_context() { return kMaxContext; }

// One workgroup per logits row; see the head of this file. Runs on the caller's stream: no
// host synchronisation, no allocation, no workspace, every index is read on the device.
RA_EXPORT int ra_logit_process(void* logits, long row_stride, const int* rows,
                               const unsigned char* active, const int* prompt,
                               const int* prompt_len, const long long* out, const int* n_out,
                               const long long* extra, const int* n_extra,
                               const float* repetition, const float* presence,
                               const float* frequency, const int* min_new, const int* bias_ids,
                               const float* bias_vals, const int* n_bias, int B, int V, int R,
                               int P, int cap, int W, int NB, int eos, hipStream_t st) {
  if (B <= 0 || V <= 0 || V > kMaxV || row_stride < V || R <= 0 || P < 0 || cap < 0 || W < 0 ||
      NB < 0 || NB > kMaxBias)
    return hipErrorInvalidValue;
  if ((long)P + cap + W + NB + 1 > kMaxContext) return hipErrorInvalidValue;
  if (!logits || ((uintptr_t)logits & 1) || !prompt_len || !n_out || !repetition || !presence ||
      !frequency || !min_new || !n_bias)
    return hipErrorInvalidValue;
  if ((P > 0 && !prompt) || (cap > 0 && !out) || (NB > 0 && (!bias_ids || !bias_vals)))
    return hipErrorInvalidValue;
  if ((extra != nullptr) != (n_extra != nullptr) || (!extra && W != 0)) return hipErrorInvalidValue;
  if (!rows && R < B) return hipErrorInvalidValue;
  ProcArgs a;
  a.logits = (bf16_t*)logits;
  a.row_stride = row_stride;
  a.rows = rows;
  a.active = active;
  a.prompt = prompt;
  a.prompt_len = prompt_len;
  a.out = out;
  a.n_out = n_out;
  a.extra = extra;
  a.n_extra = n_extra;
  a.repetition = repetition;
  a.presence = presence;
  a.frequency = frequency;
  a.min_new = min_new;
  a.bias_ids = bias_ids;
  a.bias_vals = bias_vals;
  a.n_bias = n_bias;
  a.V = V;
  a.R = R;
  a.P = P;
  a.cap = cap;
  a.W = W;
  a.NB = NB;
  a.eos = eos;
  hipLaunchKernelGGL(logit_process_kernel, dim3(B), dim3(kThreads), 0, st, a);
  return hipGetLastError();
}
