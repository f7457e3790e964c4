// Speculative decoding in the continuous-batching GPT-2 engine (models/gpt2_engine.py): the
// two decisions of a speculative step that would otherwise cost a host round trip, choosing
// the draft tokens and accepting them. Conventions of kv_slots.hip: every index is read ON
// THE DEVICE and checked there before it addresses memory, a bad slot skips its work, there
// is no host synchronisation, no allocation, no float math and no atomic on global memory,
// everything runs on the caller's stream and is capturable, and a slot's results depend on
// that slot's data only. One workgroup per slot in both kernels.
//
// ra_spec_draft: prompt-lookup (n-gram) drafts.
//
//   tok0 [S] int64            the token just sampled for position p = lens[s]
//   hist [S, cap] int32       the request's tokens by absolute position; [0, p) is read
//   lens, n_out, max_new [S] int32, active [S] uint8
//   win [S, k + 1] int64, n_win [S] int32   (outputs)
//
// An inactive slot, or one with p outside [0, cap), gets n_win = 0 and keeps its win row.
// Otherwise win[s, 0] = tok0[s]; seq is hist[s, 0:p] followed by tok0, L = p + 1, and
// room = min(max_new - n_out, cap - p). For n = ngram_max down to ngram_min with n <= L - 1,
// the largest j with j + n <= L - 1 and seq[j : j+n] == seq[L-n : L] is looked for; the
// first n with a match wins. Then nd = min(k, room - 1) and draft i (1-based) is seq[q],
// q = j + n + i - 1, if q < L, else draft q - L + 1 (a continuation that reaches the end of
// seq runs on into the drafts). No match: nd = 0. n_win = 1 + max(nd, 0).
//
// How: a candidate is named by its end e = j + n (1 <= e <= p). Its match length m(e), the
// number of i < min(ngram_max, e) with seq[e-1-i] == seq[L-1-i] for all smaller i too, says
// for which n it matches: all n <= m(e). So the winning n is the largest m(e) and the
// winning e the largest one that reaches it: the maximum of the key (m(e) << 23) | e, taken
// by the lanes striding over e, a wave reduction and one LDS word per wave. Thread 0 writes
// the window. hist is read with plain global loads (a row is a few KiB: L2-resident).
//
// ra_spec_accept: thread 0 decides, then the workgroup copies one logits row.
//
//   win, n_win as above; cand [S, k + 1] int64: the sampler's token for position p + 1 + i,
//   from the logits after win[s, i]; logits_win [S, k + 1, Vp] bf16
//   in place: lens, n_out [S] int32, active [S] uint8, out [S, cap] int64, hist [S, cap]
//   int32, buf [S, Vp] bf16, n_drafted, n_accepted [S] int32; read: max_new [S], eos
//
// An active slot with 1 <= n_win <= k + 1, 0 <= n_out < cap and 0 <= p = lens[s] < cap:
// a = the largest i <= n_win - 1 with win[s, j] == cand[s, j-1] for all 1 <= j <= i. The
// tokens win[s, 0..a] are emitted, cut after the first eos (which is emitted) and at
// max(1, min(max_new - n_out, cap - n_out, cap - p)): m >= 1 tokens, stored at
// out[s, n_out ..] and hist[s, p ..]; n_out += m, lens += m, n_drafted += n_win - 1,
// n_accepted += m - 1. The slot becomes inactive on eos or when n_out >= max_new; if it
// stays active, buf[s, :] = logits_win[s, m-1, :] (16-byte vectors where Vp and the
// pointers allow them). An active slot with any other n_win / n_out / lens becomes inactive
// without a write. Every slot that is inactive afterwards gets lens[s] = kSlotInactive, on
// every call, as ra_slot_advance does.
#include "common.h"

namespace {

constexpr int kSlotInactive = -(1 << 30);
constexpr int kSpecThreads = 256;
constexpr int kSpecMaxK = 8;      // drafts per step
constexpr int kSpecMaxN = 8;      // n-gram length
constexpr int kSpecEndBits = 23;  // cap <= 1 << 22: an end position fits below the length

__device__ __forceinline__ long lmin(long a, long b) { return a < b ? a : b; }
__device__ __forceinline__ long lmax(long a, long b) { return a > b ? a : b; }

__global__ __launch_bounds__(kSpecThreads) void spec_draft_kernel(
    const long* __restrict__ tok0, const int* __restrict__ hist, const int* __restrict__ lens,
    const int* __restrict__ n_out, const int* __restrict__ max_new,
    const unsigned char* __restrict__ active, long* __restrict__ win, int* __restrict__ n_win,
    int cap, int k, int nmin, int nmax) {
  __shared__ int red[kSpecThreads / 64];
  const int s = blockIdx.x;
  const int p = lens[s];
  if (active[s] == 0 || p < 0 || p >= cap) {  // (the same for the whole workgroup)
    if (threadIdx.x == 0) n_win[s] = 0;
    return;
  }
  const int* h = hist + (long)s * cap;
  const long t0 = tok0[s];
  // the suffix, newest first: suf[0] = seq[L-1] = tok0, suf[i] = seq[L-1-i] = hist[p-i];
  // n <= L - 1 = p, so i <= p - 1 and the index stays >= 1
  const int ns = min(nmax, p);
  long suf[kSpecMaxN];
#pragma unroll
  for (int i = 0; i < kSpecMaxN; ++i) suf[i] = i == 0 ? t0 : (i < ns ? (long)h[p - i] : 0);
  int best = 0;
  for (int e = 1 + (int)threadIdx.x; e <= p; e += kSpecThreads) {
    int m = 0;
    bool run = true;
#pragma unroll
    for (int i = 0; i < kSpecMaxN; ++i) {
      run = run && i < ns && i < e && (long)h[e - 1 - i] == suf[i];
      m += run ? 1 : 0;
    }
    if (m) best = max(best, (m << kSpecEndBits) | e);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) best = max(best, __shfl_xor(best, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int w = 1; w < kSpecThreads / 64; ++w) best = max(best, red[w]);
  long* wrow = win + (long)s * (k + 1);
  wrow[0] = t0;
  int nd = 0;
  if ((best >> kSpecEndBits) >= nmin) {
    const int e = best & ((1 << kSpecEndBits) - 1);  // j + n: where the continuation starts
    const long room = lmin((long)max_new[s] - (long)n_out[s], (long)cap - p);
    nd = (int)lmax(0, lmin(k, room - 1));
    for (int i = 1; i <= nd; ++i) {
      const int q = e + i - 1;  // e <= p: q - p < i, an earlier draft of this loop
      wrow[i] = q < p ? (long)h[q] : (q == p ? t0 : wrow[q - p]);
    }
  }
  n_win[s] = 1 + nd;
}

template <bool VEC>
__global__ __launch_bounds__(kSpecThreads) void spec_accept_kernel(
    const long* __restrict__ win, const int* __restrict__ n_win, const long* __restrict__ cand,
    const bf16_t* __restrict__ logits_win, int* __restrict__ lens, int* __restrict__ n_out,
    const int* __restrict__ max_new, unsigned char* __restrict__ active, long* __restrict__ out,
    int* __restrict__ hist, bf16_t* __restrict__ buf, int* __restrict__ n_drafted,
    int* __restrict__ n_accepted, int cap, int k, int Vp, long eos) {
  __shared__ int src_row;  // the window row whose logits the slot keeps, -1: none
  const int s = blockIdx.x, W = k + 1;
  if (threadIdx.x == 0) {
    int keep = -1;
    bool act = active[s] != 0;
    if (act) {
      const int nw = n_win[s], n = n_out[s], p = lens[s];
      if (nw < 1 || nw > W || n < 0 || n >= cap || p < 0 || p >= cap) {
        act = false;
      } else {
        const long* w = win + (long)s * W;
        const long* c = cand + (long)s * W;
        int a = 0;
        while (a + 1 < nw && w[a + 1] == c[a]) ++a;
        const int mx = max_new[s];
        const long lim = lmax(1, lmin((long)mx - n, (long)cap - max(n, p)));
        int m = (int)lmin(a + 1, lim);
        bool hit = false;
        for (int i = 0; i < m; ++i) {
          const long t = w[i];
          out[(long)s * cap + n + i] = t;
          hist[(long)s * cap + p + i] = (int)t;
          if (eos >= 0 && t == eos) {
            m = i + 1;
            hit = true;
          }
        }
        n_out[s] = n + m;
        lens[s] = p + m;
        n_drafted[s] += nw - 1;
        n_accepted[s] += m - 1;
        if (hit || n + m >= mx) act = false; else keep = m - 1;
      }
      if (!act) active[s] = 0;
    }
    if (!act) lens[s] = kSlotInactive;
    src_row = keep;
  }
  __syncthreads();
  const int r = src_row;
  if (r < 0) return;
  const bf16_t* src = logits_win + ((long)s * W + r) * Vp;
  bf16_t* dst = buf + (long)s * Vp;
  if (VEC) {  // Vp % 8 == 0 and both tensors 16-byte aligned: every row is
    const uint4* s4 = reinterpret_cast<const uint4*>(src);
    uint4* d4 = reinterpret_cast<uint4*>(dst);
    const int nv = Vp >> 3;
    for (int i = threadIdx.x; i < nv; i += kSpecThreads * 4) {
      uint4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = i + u * kSpecThreads;
        if (j < nv) v[u] = s4[j];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = i + u * kSpecThreads;
        if (j < nv) d4[j] = v[u];
      }
    }
  } else {
    for (int i = threadIdx.x; i < Vp; i += kSpecThreads) dst[i] = src[i];
  }
}

}  // namespace

// k in 1..8, 1 <= ngram_min <= ngram_max <= 8. Runs on the caller's stream; no host
// synchronisation, no allocation.
RA_EXPORT int ra_spec_draft(const long* tok0, const int* hist, const int* lens, const int* n_out,
                            const int* max_new, const unsigned char* active, long* win,
                            int* n_win, int S, int cap, int k, int ngram_min, int ngram_max,
                            hipStream_t st) {
  if (S <= 0 || cap <= 0 || cap > (1 << 22) || k < 1 || k > kSpecMaxK || ngram_min < 1 ||
      ngram_min > ngram_max || ngram_max > kSpecMaxN)
    return hipErrorInvalidValue;
  if (tok0 == nullptr || hist == nullptr || lens == nullptr || n_out == nullptr ||
      max_new == nullptr || active == nullptr || win == nullptr || n_win == nullptr)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(spec_draft_kernel, dim3(S), dim3(kSpecThreads), 0, st, tok0, hist, lens,
                     n_out, max_new, active, win, n_win, cap, k, ngram_min, ngram_max);
  return hipGetLastError();
}

// eos < 0: none. Runs on the caller's stream; no host synchronisation, no allocation.
RA_EXPORT int ra_spec_accept(const long* win, const int* n_win, const long* cand,
                             const void* logits_win, int* lens, int* n_out, const int* max_new,
                             unsigned char* active, long* out, int* hist, void* buf,
                             int* n_drafted, int* n_accepted, int S, int cap, int k, int Vp,
                             long eos, hipStream_t st) {
  if (S <= 0 || cap <= 0 || cap > (1 << 22) || k < 1 || k > kSpecMaxK || Vp <= 0)
    return hipErrorInvalidValue;
  if (win == nullptr || n_win == nullptr || cand == nullptr || logits_win == nullptr ||
      lens == nullptr || n_out == nullptr || max_new == nullptr || active == nullptr ||
      out == nullptr || hist == nullptr || buf == nullptr || n_drafted == nullptr ||
      n_accepted == nullptr)
    return hipErrorInvalidValue;
  const bool vec = (Vp & 7) == 0 && (((uintptr_t)logits_win | (uintptr_t)buf) & 15) == 0;
  auto kern = vec ? spec_accept_kernel<true> : spec_accept_kernel<false>;
  hipLaunchKernelGGL(kern, dim3(S), dim3(kSpecThreads), 0, st, win, n_win, cand,
                     (const bf16_t*)logits_win, lens, n_out, max_new, active, out, hist,
                     (bf16_t*)buf, n_drafted, n_accepted, cap, k, Vp, eos);
  return hipGetLastError();
}
