// Grammar-constrained decoding of the GPT-2 serving stack: a token-level DFA per request, kept
// as rows of one int16 table, bans IN PLACE the logits of the tokens its current state does
// not allow (grammar_mask) and follows the tokens the request emitted (grammar_advance).
// Semantics: ops/reference.py grammar_mask / grammar_advance, bit for bit. One launch each,
// every index read and bounds-checked on the device, no host read, no workspace, no atomic:
// capturable, and one capture serves every position.
//
//   table  int16 [N, Vt], Vt a multiple of 8 and the base 16-byte aligned, so every row is:
//          table[q, t] the state after token t in state q, negative: t is not allowed in q
//   state  int32 [R]: a context row's state (negative: unconstrained or dead, nothing to do)
//   logits [B, >= V] bf16, row b at logits + b * row_stride (any stride >= V, any 2-byte
//          alignment: the [:, :vocab_size] view of the padded LM-head output in place)
//   rows int32 [B] or null (b): the context row of logits row b; active uint8 [B] or null
//   extra int64 [B, W] or null, n_extra int32 [B]: tokens to walk from state[r] first (the
//          speculative window up to this row)
//
// grammar_mask is elementwise, so the grid is (row, chunk of the row's 16-byte slots). Every
// workgroup first repeats the row's walk: state[r], then at most W <= kMaxWalk dependent
// 2-byte table loads, all block-uniform; a row that is inactive, out of range, unconstrained
// or whose walk meets a forbidden token ends there and keeps its bytes. Then each lane takes
// aligned 16-byte slots of the LOGITS row (row_slots.h's view: slot j holds the elements
// j * 8 - off .. j * 8 - off + 7, off = the row's misalignment in elements). The 8 table
// entries of such a slot sit in the aligned table slots j - 1 and j; each is one 16-byte
// load reduced to 8 sign bits, and a shift by 8 - off picks the slot's own 8. kUnroll slots
// per lane are in flight together. A slot wholly inside [0, V): all 8 banned is one 16-byte
// store without a load, none banned is nothing, otherwise load, merge, store. The first and
// the last slot of a row may hold bytes of a neighbouring row (another workgroup's), so
// there the banned elements are stored one by one, 2 bytes each, and nothing else is touched.
//
// Resources (gfx950, -O3, -Rpass-analysis=kernel-resource-usage): grammar_mask_kernel 36 VGPRs,
// 41 SGPRs; grammar_advance_kernel 14 VGPRs, 22 SGPRs; no scratch, no spill, no LDS. Measured,
// the chunk included: profiles/r18/grammar.md.
#include "common.h"

namespace {

constexpr int kThreads = 64;
constexpr int kUnroll = 4;
constexpr int kGroup = kThreads * kUnroll;  // slots per workgroup pass; a chunk is a multiple
constexpr int kMaxWalk = 16;
constexpr int kMaxV = 1 << 18;
constexpr int kMaxStates = 32767;
constexpr int kDead = -2;

struct MaskArgs {
  bf16_t* logits;
  long row_stride;
  const short* table;
  const int* state;
  const int* rows;
  const unsigned char* active;
  const long long* extra;
  const int* n_extra;
  int V, N, Vt, R, W, chunk, nchunks;
};

// the sign bits of the 8 int16 of a table slot, element e at bit e
__device__ __forceinline__ uint32_t ban8(uint4 u) {
  auto two = [](uint32_t w) { return ((w >> 15) & 1u) | ((w >> 30) & 2u); };
  return two(u.x) | (two(u.y) << 2) | (two(u.z) << 4) | (two(u.w) << 6);
}

// word w of a logits slot with the elements named in the 2 bits of m2 set to bf16 -inf
__device__ __forceinline__ uint32_t banned_word(uint32_t w, uint32_t m2) {
  const uint32_t sel = ((m2 & 1u) ? 0x0000ffffu : 0u) | ((m2 & 2u) ? 0xffff0000u : 0u);
  return (w & ~sel) | (0xff80ff80u & sel);
}

__global__ __launch_bounds__(kThreads) void grammar_mask_kernel(MaskArgs a) {
  const int b = blockIdx.x / a.nchunks, c = blockIdx.x - b * a.nchunks;
  // ---- the row's state, every index checked before it addresses anything (block-uniform)
  if (a.active && !a.active[b]) return;
  const int r = a.rows ? a.rows[b] : b;
  if (r < 0 || r >= a.R) return;
  int q = a.state[r];
  if (q < 0 || q >= a.N) return;
  if (a.extra) {
    const int ne = a.n_extra[b];
    if (ne < 0 || ne > a.W) return;
    const long long* erow = a.extra + (long)b * a.W;
    for (int j = 0; j < ne; ++j) {
      const long long t = erow[j];
      if (t < 0 || t >= a.Vt) return;
      q = a.table[(long)q * a.Vt + t];
      if (q < 0 || q >= a.N) return;  // a forbidden draft: this row's logits are never used
    }
  }
  const uint4* trow = reinterpret_cast<const uint4*>(a.table + (long)q * a.Vt);
  const int tslots = a.Vt >> 3;

  bf16_t* rowp = a.logits + (long)b * a.row_stride;
  const int off = (int)(((uintptr_t)rowp >> 1) & 7);
  bf16_t* base = rowp - off;  // 16-byte aligned; only bytes inside the row are accessed
  const int V = a.V;
  const int nslots = (off + V + 7) >> 3;
  const int end = min(nslots, (c + 1) * a.chunk);

  for (int j0 = c * a.chunk + (int)threadIdx.x; j0 < end; j0 += kGroup) {
    uint32_t m[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {  // the table loads of kUnroll slots, in flight together
      const int j = j0 + u * kThreads;
      uint32_t lo = 0, hi = 0;
      if (j < end) {
        if (off != 0 && j >= 1 && j - 1 < tslots) lo = ban8(trow[j - 1]);
        if (j < tslots) hi = ban8(trow[j]);
      }
      m[u] = ((lo | (hi << 8)) >> (8 - off)) & 0xffu;
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int j = j0 + u * kThreads;
      if (j >= end) continue;
      const int i0 = j * 8 - off;  // the index of the slot's element 0
      if (i0 >= 0 && i0 + 8 <= V) {
        if (m[u] == 0) continue;
        uint4* p = reinterpret_cast<uint4*>(base + (long)j * 8);
        if (m[u] == 0xffu) {
          *p = make_uint4(0xff80ff80u, 0xff80ff80u, 0xff80ff80u, 0xff80ff80u);
        } else {
          uint4 x = *p;
          x.x = banned_word(x.x, m[u]);
          x.y = banned_word(x.y, m[u] >> 2);
          x.z = banned_word(x.z, m[u] >> 4);
          x.w = banned_word(x.w, m[u] >> 6);
          *p = x;
        }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int i = i0 + e;
          if (i >= 0 && i < V && ((m[u] >> e) & 1u)) rowp[i] = (bf16_t)0xff80;
        }
      }
    }
  }
}

struct AdvanceArgs {
  int* state;
  int* pos;
  const long long* out;
  const int* n_out;
  const short* table;
  int R, cap, N, Vt, max_steps;
};

__global__ __launch_bounds__(kThreads) void grammar_advance_kernel(AdvanceArgs a) {
  const int r = blockIdx.x * kThreads + threadIdx.x;
  if (r >= a.R) return;
  int q = a.state[r], p = a.pos[r];
  const int n = a.n_out[r];
  if (q < 0 || q >= a.N || p < 0 || p >= n || n > a.cap) return;
  const long long* orow = a.out + (long)r * a.cap;
  for (int s = 0; s < a.max_steps && p < n; ++s) {
    const long long t = orow[p];
    if (t < 0 || t >= a.Vt) break;
    const int nx = a.table[(long)q * a.Vt + t];
    ++p;
    if (nx < 0 || nx >= a.N) {
      q = kDead;
      break;
    }
    q = nx;
  }
  a.state[r] = q;
  a.pos[r] = p;
}

}  // namespace

RA_EXPORT int ra_grammar_max_walk() { return kMaxWalk; }
RA_EXPORT int ra_grammar_max_states() { return kMaxStates; }

// The slots of a row that one workgroup takes: kGroup = 256 (2048 elements), one pass of one
// wave, at every batch. Measured at GPT-2's vocabulary (profiles/r18/grammar.md): B = 1 is then
// 25 workgroups on 25 CUs and takes 3.4 us, and a chunk of 512 / 1024 / 2048 slots 4.8 / 7.8 /
// 13.5 us; at B = 576 (14400 workgroups, each repeating the row's walk) 256 and 512 slots tie
// at 15..17 us and 1024 takes 19 us, so a larger chunk buys nothing for a large batch either.
RA_EXPORT int ra_grammar_mask_chunk(int B, int V) {
  (void)B, (void)V;
  return kGroup;
}

// grammar_mask_kernel: grid = B * ceil(slots / chunk) workgroups of one wave; see the head of
// this file. chunk 0: ra_grammar_mask_chunk. Runs on the caller's stream: no host
// synchronisation, no allocation, no workspace.
RA_EXPORT int ra_grammar_mask(void* logits, long row_stride, const void* table, const int* state,
                              const int* rows, const unsigned char* active,
                              const long long* extra, const int* n_extra, int B, int V, int N,
                              int Vt, int R, int W, int chunk, hipStream_t st) {
  if (B <= 0 || V <= 0 || V > kMaxV || row_stride < V || N <= 0 || N > kMaxStates || Vt < V ||
      (Vt & 7) || R <= 0 || W < 0 || W > kMaxWalk)
    return hipErrorInvalidValue;
  if (!logits || ((uintptr_t)logits & 1) || !table || ((uintptr_t)table & 15) || !state)
    return hipErrorInvalidValue;
  if ((extra != nullptr) != (n_extra != nullptr) || (!extra && W != 0) || (extra && W == 0))
    return hipErrorInvalidValue;
  if (!rows && R < B) return hipErrorInvalidValue;
  if (chunk == 0) chunk = ra_grammar_mask_chunk(B, V);
  if (chunk < kGroup || chunk % kGroup) return hipErrorInvalidValue;
  const long nslots = ((long)V + 7 + 7) >> 3;  // the most a misaligned row covers
  const long nchunks = (nslots + chunk - 1) / chunk;
  if ((long)B * nchunks > 0x7fffffffL) return hipErrorInvalidValue;
  MaskArgs a;
  a.logits = (bf16_t*)logits;
  a.row_stride = row_stride;
  a.table = (const short*)table;
  a.state = state;
  a.rows = rows;
  a.active = active;
  a.extra = extra;
  a.n_extra = n_extra;
  a.V = V;
  a.N = N;
  a.Vt = Vt;
  a.R = R;
  a.W = W;
  a.chunk = chunk;
  a.nchunks = (int)nchunks;
  hipLaunchKernelGGL(grammar_mask_kernel, dim3((unsigned)(B * nchunks)), dim3(kThreads), 0, st, a);
  return hipGetLastError();
}

// grammar_advance_kernel: one thread per context row, in place.
RA_EXPORT int ra_grammar_advance(int* state, int* pos, const long long* out, const int* n_out,
                                 const void* table, int R, int cap, int N, int Vt, int max_steps,
                                 hipStream_t st) {
  if (R <= 0 || cap <= 0 || N <= 0 || N > kMaxStates || Vt <= 0 || max_steps < 0)
    return hipErrorInvalidValue;
  if (!state || !pos || !out || !n_out || !table) return hipErrorInvalidValue;
  AdvanceArgs a;
  a.state = state;
  a.pos = pos;
  a.out = out;
  a.n_out = n_out;
  a.table = (const short*)table;
  a.R = R;
  a.cap = cap;
  a.N = N;
  a.Vt = Vt;
  a.max_steps = max_steps;
  hipLaunchKernelGGL(grammar_advance_kernel, dim3((R + kThreads - 1) / kThreads), dim3(kThreads),
                     0, st, a);
  return hipGetLastError();
}
