// Rules about token SEQUENCES in the GPT-2 serving stack: banned sequences and no-repeat
// n-grams (ra_seq_ban, an in-place edit of rows of logits) and stop sequences
// (ra_stop_check, a cut of each row's output). Both depend on what a row has emitted so far,
// which lives on the device inside one captured step. Conventions of logit_proc.hip and
// spec.hip: one launch each on the caller's stream, every index and length read ON THE DEVICE
// and checked there before it addresses memory, no host read, no allocation, no workspace, no
// float math, no atomic: capturable, and one capture serves every position. Semantics:
// ops/reference.py seq_ban and stop_check, bit for bit.
//
// ra_seq_ban
//
//   logits [B, >= V] bf16, row b at logits + b * row_stride (any stride >= V, any 2-byte
//          alignment: the [:, :vocab_size] view of the padded LM-head output in place)
//   rows int32 [B] or null (b): the context row r of logits row b; active uint8 [B] or null
//   prompt int32 [R, P], prompt_len int32 [R]; out int64 [R, cap], n_out int32 [R]
//   extra int64 [B, W] or null, n_extra int32 [B]: the tokens after out[r, :n_out[r]]
//   bad int32 [R, kSeqMax, kSeqMaxLen], bad_len int32 [R, kSeqMax]; ngram int32 [R]
//
// The context c of row b is prompt[r, :prompt_len[r]] ++ out[r, :n_out[r]] ++ extra[b,
// :n_extra[b]], C tokens. One workgroup of 256 threads per logits row. It reads ngram[r] and
// the eight bad_len[r] first (block-uniform loads) and leaves at once when the row is
// skipped (inactive, r or a length out of range, ngram outside 0..8) or has no rule.
//   * no-repeat, n = ngram[r] >= 1, C >= n: the suffix c[C-n+1 : C] (at most 7 tokens) sits in
//     registers, newest first; the threads stride over the starts i in [0, C - n], compare
//     c[i+n-2-k] with suffix token k, newest first, leave at the first difference, and a
//     full match bans c[i+n-1]. Every compare is a plain global load of a row that is a few
//     KiB (L2-resident), as spec_draft in spec.hip does it.
//   * banned sequence q (thread q < kSeqMax) of length L: if L - 1 <= C and the last L - 1
//     context tokens equal bad[r, q, :L-1], it bans bad[r, q, L-1].
// A ban is ONE 2-byte store of bf16 -inf (0xFF80) to an id inside [0, V); nothing else is
// written and the row is never streamed. Every store writes the same constant, so the
// stores are order-free and a token banned twice is banned.
//
// ra_stop_check
//
//   out int64 [R, cap]; n_out, pos, hit int32 [R] (in place)
//   stops int32 [R, kSeqMax, kSeqMaxLen], stop_len int32 [R, kSeqMax]
//   active uint8 [R], lens int32 [R], done uint8 [R]: in place, each may be null
//
// One wave per row. The ends e in (pos, min(n_out, pos + max_span)] and the sequences q make
// up to span * 8 (end, sequence) pairs; the lanes stride over them in ascending order of the
// key (e << 3) | q, each pair costs at most 8 compares (newest token first), and a lane
// stops at its first match. The winner is the minimum key of the wave (shuffle reduction):
// the smallest end, and there the lowest q. Lane 0 writes: n_out = e, hit = q, active = 0,
// lens = kSlotInactive, done = 1, pos = e; without a match pos = the last end checked.
// active and done are never read. A row with n_out outside [0, cap] or pos outside
// [0, n_out] has nothing written.
//
// Resources (gfx950, -O3, -Rpass-analysis=kernel-resource-usage): seq_ban 12 VGPRs, stop_check
// 16 VGPRs; both no scratch, no spill, no LDS, occupancy 8. Measured: profiles/r19/seq_rules.md.
#include "common.h"

namespace {

constexpr int kSlotInactive = -(1 << 30);
constexpr int kSeqMax = 8;     // sequences per row and kind
constexpr int kSeqMaxLen = 8;  // tokens per sequence; the longest no-repeat n-gram
constexpr int kBanThreads = 256;
constexpr int kMaxV = 1 << 18;
constexpr int kMaxCap = 1 << 22;  // (e << 3) | q fits an int
constexpr bf16_t kNegInf = 0xff80;

struct BanArgs {
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
  const int* bad;
  const int* bad_len;
  const int* ngram;
  int V, R, P, cap, W;
};

// The three segments of a row's context behind one index: 0 <= i < pl + no + ne.
struct Context {
  const int* prompt;
  const long long* out;
  const long long* extra;
  int pl, no;
  __device__ __forceinline__ long long operator[](int i) const {
    if (i < pl) return (long long)prompt[i];
    i -= pl;
    return i < no ? out[i] : extra[i - no];
  }
};

__global__ __launch_bounds__(kBanThreads) void seq_ban_kernel(BanArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x;
  // ---- the row's context and rules, checked before they address anything (block-uniform)
  if (a.active && !a.active[b]) return;
  const int r = a.rows ? a.rows[b] : b;
  if (r < 0 || r >= a.R) return;
  const int n = a.ngram[r];
  if (n < 0 || n > kSeqMaxLen) return;
  const int pl = a.prompt_len[r], no = a.n_out[r];
  const int ne = a.extra ? a.n_extra[b] : 0;
  if (pl < 0 || pl > a.P || no < 0 || no > a.cap || ne < 0 || ne > a.W) return;
  const int* blen = a.bad_len + (long)r * kSeqMax;
  bool any_bad = false;
#pragma unroll
  for (int q = 0; q < kSeqMax; ++q) {
    const int L = blen[q];
    any_bad = any_bad || (L >= 1 && L <= kSeqMaxLen);
  }
  if (n == 0 && !any_bad) return;  // no rule

  const int C = pl + no + ne;  // <= P + cap + W, which the launch keeps below 2^31
  Context c;
  c.prompt = a.prompt + (long)r * a.P;
  c.out = a.out + (long)r * a.cap;
  c.extra = a.extra ? a.extra + (long)b * a.W : nullptr;
  c.pl = pl;
  c.no = no;
  bf16_t* rowp = a.logits + (long)b * a.row_stride;
  const int V = a.V;

  if (n >= 1 && C >= n) {
    // the suffix, newest first: s0 = c[C-1], ..., token k = c[C-1-k] for k < n - 1
    const long long s0 = n > 1 ? c[C - 1] : 0, s1 = n > 2 ? c[C - 2] : 0;
    const long long s2 = n > 3 ? c[C - 3] : 0, s3 = n > 4 ? c[C - 4] : 0;
    const long long s4 = n > 5 ? c[C - 5] : 0, s5 = n > 6 ? c[C - 6] : 0;
    const long long s6 = n > 7 ? c[C - 7] : 0;
    for (int i = tid; i <= C - n; i += kBanThreads) {
      const int e = i + n - 2;  // the newest token of the candidate's prefix
      bool m = true;
      m = m && (n <= 1 || c[e] == s0);
      m = m && (n <= 2 || c[e - 1] == s1);
      m = m && (n <= 3 || c[e - 2] == s2);
      m = m && (n <= 4 || c[e - 3] == s3);
      m = m && (n <= 5 || c[e - 4] == s4);
      m = m && (n <= 6 || c[e - 5] == s5);
      m = m && (n <= 7 || c[e - 6] == s6);
      if (m) {
        const long long t = c[e + 1];
        if (t >= 0 && t < V) rowp[t] = kNegInf;
      }
    }
  }
  if (any_bad && tid < kSeqMax) {
    const int L = blen[tid];
    if (L >= 1 && L <= kSeqMaxLen && L - 1 <= C) {
      const int* seq = a.bad + ((long)r * kSeqMax + tid) * kSeqMaxLen;
      bool m = true;
      for (int k = 0; k < L - 1 && m; ++k)  // newest first
        m = c[C - 1 - k] == (long long)seq[L - 2 - k];
      if (m) {
        const int t = seq[L - 1];
        if (t >= 0 && t < V) rowp[t] = kNegInf;
      }
    }
  }
}

__global__ __launch_bounds__(64) void stop_check_kernel(
    const long long* __restrict__ out, int* __restrict__ n_out, int* __restrict__ pos,
    const int* __restrict__ stops, const int* __restrict__ stop_len, int* __restrict__ hit,
    unsigned char* __restrict__ active, int* __restrict__ lens, unsigned char* __restrict__ done,
    int cap, int max_span) {
  const int r = blockIdx.x, lane = threadIdx.x;
  const int n = n_out[r], p = pos[r];
  if (n < 0 || n > cap || p < 0 || p > n || p == n) return;  // (the same for the whole wave)
  const int span = min(n - p, max_span);
  const long long* orow = out + (long)r * cap;
  const int* slen = stop_len + (long)r * kSeqMax;
  const int* srow = stops + (long)r * kSeqMax * kSeqMaxLen;
  constexpr int kNone = 0x7fffffff;
  int best = kNone;
  // pair j: end p + 1 + (j >> 3), sequence j & 7; j ascends with the key, so a lane's first
  // match is its smallest. span <= cap <= 2^22: span * 8 fits an int
  for (int j = lane; j < span * kSeqMax && best == kNone; j += 64) {
    const int e = p + 1 + (j >> 3), q = j & (kSeqMax - 1);
    const int L = slen[q];
    if (L < 1 || L > kSeqMaxLen || L > e) continue;
    const int* seq = srow + q * kSeqMaxLen;
    bool m = true;
#pragma unroll
    for (int k = 0; k < kSeqMaxLen; ++k)  // newest first; k < L <= e keeps e - 1 - k >= 0
      m = m && (k >= L || orow[e - 1 - k] == (long long)seq[L - 1 - k]);
    if (m) best = (e << 3) | q;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o, 64));
  if (lane != 0) return;
  if (best == kNone) {
    pos[r] = p + span;
    return;
  }
  const int e = best >> 3;
  n_out[r] = e;
  pos[r] = e;
  hit[r] = best & (kSeqMax - 1);
  if (active) active[r] = 0;
  if (lens) lens[r] = kSlotInactive;
  if (done) done[r] = 1;
}

}  // namespace

RA_EXPORT int ra_seq_max() { return kSeqMax; }
RA_EXPORT int ra_seq_max_len() { return kSeqMaxLen; }

// One workgroup per logits row; see the head of this file. Runs on the caller's stream: no
// host synchronisation, no allocation, no workspace, every index is read on the device.
RA_EXPORT int ra_seq_ban(void* logits, long row_stride, const int* rows,
                         const unsigned char* active, const int* prompt, const int* prompt_len,
                         const long long* out, const int* n_out, const long long* extra,
                         const int* n_extra, const int* bad, const int* bad_len,
                         const int* ngram, int B, int V, int R, int P, int cap, int W,
                         hipStream_t st) {
  if (B <= 0 || V <= 0 || V > kMaxV || row_stride < V || R <= 0 || P < 0 || cap < 0 || W < 0)
    return hipErrorInvalidValue;
  if ((long)P + cap + W > (1L << 30)) return hipErrorInvalidValue;
  if (!logits || ((uintptr_t)logits & 1) || !prompt_len || !n_out || !bad || !bad_len || !ngram)
    return hipErrorInvalidValue;
  if ((P > 0 && !prompt) || (cap > 0 && !out)) return hipErrorInvalidValue;
  if ((extra != nullptr) != (n_extra != nullptr) || (!extra && W != 0)) return hipErrorInvalidValue;
  if (!rows && R < B) return hipErrorInvalidValue;
  BanArgs a;
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
  a.bad = bad;
  a.bad_len = bad_len;
  a.ngram = ngram;
  a.V = V;
  a.R = R;
  a.P = P;
  a.cap = cap;
  a.W = W;
  hipLaunchKernelGGL(seq_ban_kernel, dim3(B), dim3(kBanThreads), 0, st, a);
  return hipGetLastError();
}

// One wave per row; active, lens and done may be null. max_span >= 0 bounds the ends looked
// at per row. Runs on the caller's stream: no host synchronisation, no allocation.
RA_EXPORT int ra_stop_check(const long long* out, int* n_out, int* pos, const int* stops,
                            const int* stop_len, int* hit, unsigned char* active, int* lens,
                            unsigned char* done, int R, int cap, int max_span, hipStream_t st) {
  if (R <= 0 || cap <= 0 || cap > kMaxCap || max_span < 0) return hipErrorInvalidValue;
  if (!out || !n_out || !pos || !stops || !stop_len || !hit) return hipErrorInvalidValue;
  hipLaunchKernelGGL(stop_check_kernel, dim3(R), dim3(64), 0, st, out, n_out, pos, stops,
                     stop_len, hit, active, lens, done, cap, max_span);
  return hipGetLastError();
}
