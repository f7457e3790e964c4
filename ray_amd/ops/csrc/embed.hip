// Token + position embedding backward straight into the flat fp32 gradient sinks.
//
//   wte_grad[idx[n], :] += dx[n, :]          n = 0 .. B*T-1   (scatter-add)
//   wpe_grad[t, :]      += sum_b dx[b, t, :]                   (column reduction)
//
// Replaces torch's `index_add_(0, idx, dx.to(fp32))` (a bf16 -> fp32 copy of dx, then an
// atomic index kernel) and `add_(dx.float().sum(0))` (another fp32 copy and a reduce):
// dx is read twice as bf16 and nothing else is materialised.
//
// No float atomics: every sum runs in a fixed order, so the same batch gives the same
// gradient bits every run. The caller sorts the token ids (stable) and passes the sorted
// ids with the row each came from. The sorted positions are cut into chunks at every
// multiple of kChunk and at every change of token, so a chunk has at most kChunk rows of
// one token. Launch 1: the wave at the first position of a chunk sums the chunk's rows in
// order; a token that lies in one chunk goes straight into its sink row (its only writer),
// a chunk of a longer token writes its partial sum to the workspace (two slots per window
// of kChunk positions: the chunk that enters the window from the left, and the chunk that
// leaves it to the right). The same launch reduces the positions on the workgroups after
// the scatter ones. Launch 2: for each token that spans several chunks, the wave of its
// first window adds the partial sums from left to right and adds the total to the sink
// row. A token that fills 5 % of a 65536-row batch is ~100 chunks summed by ~100 waves and
// one ~100-term combine, not one wave walking 3000 rows.
// Reference: the embedding gradient of torch.nn.functional.embedding that the reference's
// GPT-2 benchmark runs through DDP
// (release/air_tests/air_benchmarks/workloads/torch_benchmark.py).
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 32;   // sorted positions per window
constexpr int kColTile = 16;  // 64-column groups a lane accumulates at once (1024 columns)

// acc[i] += row[c0 + i * 64 + lane] for the lane's columns of one column tile
__device__ __forceinline__ void add_row_bf16(float (&acc)[kColTile], const bf16_t* row, int c0,
                                             int C, int lane) {
#pragma unroll
  for (int i = 0; i < kColTile; ++i) {
    const int c = c0 + i * 64 + lane;
    if (c < C) acc[i] += bf2f(row[c]);
  }
}

__device__ __forceinline__ void add_row_f32(float (&acc)[kColTile], const float* row, int c0,
                                            int C, int lane) {
#pragma unroll
  for (int i = 0; i < kColTile; ++i) {
    const int c = c0 + i * 64 + lane;
    if (c < C) acc[i] += row[c];
  }
}

// dst[c] = acc (STORE) or dst[c] += acc
template <bool STORE>
__device__ __forceinline__ void put_row(const float (&acc)[kColTile], float* dst, int c0, int C,
                                        int lane) {
#pragma unroll
  for (int i = 0; i < kColTile; ++i) {
    const int c = c0 + i * 64 + lane;
    if (c < C) dst[c] = STORE ? acc[i] : dst[c] + acc[i];
  }
}

__global__ __launch_bounds__(kThreads) void embed_bwd_kernel(
    const bf16_t* __restrict__ dx, const long* __restrict__ sid, const long* __restrict__ perm,
    float* __restrict__ work, float* __restrict__ wte_g, float* __restrict__ wpe_g, int B, int T,
    int C, int V, int scatter_blocks) {
  const int C8 = C >> 3;
  if ((int)blockIdx.x < scatter_blocks) {
    const long rows = (long)B * T;
    const long n = (long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (n >= rows) return;
    const long tok = sid[n];
    if (tok < 0 || tok >= V) return;
    const bool is_start = n == 0 || sid[n - 1] != tok;
    if (!is_start && n % kChunk != 0) return;  // not the first position of a chunk
    const int lane = threadIdx.x & 63;
    // the chunk ends at the window's end, at the last row, or where the token changes: lane
    // l looks at position n + 1 + l, the first lane that sees the end gives the row count
    const long wend = (n / kChunk + 1) * kChunk < rows ? (n / kChunk + 1) * kChunk : rows;
    const long pos = n + 1 + lane;
    const unsigned long long same = __ballot(pos < wend && sid[pos] == tok);
    const int cnt = ~same ? __ffsll(~same) : 64;  // 1 + lanes that still see the token
    const long end = n + cnt;
    const bool continues = end < rows && sid[end] == tok;  // then end % kChunk == 0
    const bool whole = is_start && !continues;             // the token lies in this chunk
    // the chunk's rows of dx, one per lane, handed round below: the row loads of different
    // j do not wait for one another (the adds keep their order)
    const long my_row = lane < cnt ? perm[n + lane] : -1;
    float* dst = whole ? wte_g + tok * C : work + (2 * (n / kChunk) + (is_start ? 1 : 0)) * C;
    for (int c0 = 0; c0 < C; c0 += kColTile * 64) {
      float acc[kColTile];
#pragma unroll
      for (int i = 0; i < kColTile; ++i) acc[i] = 0.f;
#pragma unroll 4
      for (int j = 0; j < cnt; ++j) {
        const long r = __shfl(my_row, j);
        if (r >= 0 && r < rows) add_row_bf16(acc, dx + r * C, c0, C, lane);
      }
      if (whole) put_row<false>(acc, dst, c0, C, lane);
      else put_row<true>(acc, dst, c0, C, lane);
    }
    return;
  }
  const long item = (long)(blockIdx.x - scatter_blocks) * kThreads + threadIdx.x;
  const long t = item / C8;
  if (t >= T) return;
  const int c8 = (int)(item - t * C8);
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int b = 0; b < B; ++b) {
    float v[8];
    unpack8(reinterpret_cast<const uint4*>(dx + ((long)b * T + t) * C)[c8], v);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += v[j];
  }
  float4* g = reinterpret_cast<float4*>(wpe_g + t * C + c8 * 8);
  float4 a = g[0], b2 = g[1];
  a.x += acc[0], a.y += acc[1], a.z += acc[2], a.w += acc[3];
  b2.x += acc[4], b2.y += acc[5], b2.z += acc[6], b2.w += acc[7];
  g[0] = a;
  g[1] = b2;
}

// One wave per window w: if the token at the window's last position started inside this
// window and goes on into the next one, add its chunks' partial sums from left to right.
__global__ __launch_bounds__(kThreads) void embed_combine_kernel(
    const long* __restrict__ sid, const float* __restrict__ work, float* __restrict__ wte_g,
    long rows, int C, int V) {
  const long w = (long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  const long first = w * kChunk, next = first + kChunk;
  if (next >= rows) return;  // the last window has nothing to its right
  const long tok = sid[next - 1];
  if (tok < 0 || tok >= V || sid[next] != tok) return;                  // ends in this window
  if (sid[first] == tok && first > 0 && sid[first - 1] == tok) return;  // started before it
  const int lane = threadIdx.x & 63;
  // where the token ends: the first position after `next` with a larger id (binary search,
  // the ids are sorted); its windows are w + 1 .. vlast, each with a partial sum in slot 0
  long lo = next, hi = rows;
  while (lo < hi) {
    const long mid = lo + (hi - lo) / 2;
    if (sid[mid] <= tok) lo = mid + 1;
    else hi = mid;
  }
  const long vlast = (lo - 1) / kChunk;
  for (int c0 = 0; c0 < C; c0 += kColTile * 64) {
    float acc[kColTile];
#pragma unroll
    for (int i = 0; i < kColTile; ++i) acc[i] = 0.f;
    add_row_f32(acc, work + (2 * w + 1) * C, c0, C, lane);
#pragma unroll 4
    for (long v = w + 1; v <= vlast; ++v) add_row_f32(acc, work + (2 * v) * C, c0, C, lane);
    put_row<false>(acc, wte_g + tok * C, c0, C, lane);
  }
}

}  // namespace

// fp32 workspace (floats) of ra_embed_bwd: two partial rows per window of kChunk positions
RA_EXPORT long ra_embed_bwd_work(int B, int T, int C) {
  return 2 * (((long)B * T + kChunk - 1) / kChunk) * (long)C;
}

// dx: [B*T, C] bf16 contiguous (C % 8 == 0); sorted_idx: [B*T] int64 token ids in ascending
// order and perm: [B*T] the row of dx of each (torch.sort(idx, stable=True)); work:
// ra_embed_bwd_work(B, T, C) floats; wte_g: fp32 [V, C] sink (accumulated); wpe_g: fp32
// [>= T, C] sink (rows 0..T-1 accumulated).
RA_EXPORT int ra_embed_bwd(const void* dx, const long* sorted_idx, const long* perm, float* work,
                           float* wte_g, float* wpe_g, int B, int T, int C, int V,
                           hipStream_t st) {
  if (B <= 0 || T <= 0 || C <= 0 || C % 8 || V <= 0) return hipErrorInvalidValue;
  const long rows = (long)B * T;
  const long reduce_items = (long)T * (C / 8);
  const int sb = (int)((rows + kThreads / 64 - 1) / (kThreads / 64));
  const int rb = (int)((reduce_items + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(embed_bwd_kernel, dim3(sb + rb), dim3(kThreads), 0, st, (const bf16_t*)dx,
                     sorted_idx, perm, work, wte_g, wpe_g, B, T, C, V, sb);
  const long windows = (rows + kChunk - 1) / kChunk;
  const int cb = (int)((windows + kThreads / 64 - 1) / (kThreads / 64));
  hipLaunchKernelGGL(embed_combine_kernel, dim3(cb), dim3(kThreads), 0, st, sorted_idx,
                     (const float*)work, wte_g, rows, C, V);
  return hipGetLastError();
}
