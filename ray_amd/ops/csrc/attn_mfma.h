// Building blocks shared by the head_dim-64 MFMA attention kernels (attn.hip,
// attn_extend.hip): the 32x32x16 bf16 MFMA and its fragment helpers, the swizzled LDS image
// of a [rows][64] bf16 tile and its lane-constant read offsets, the forward's 64-key tile
// (fwd_tile), tile registers and the wave-private LDS ordering of the epilogues. See
// attn.hip's header for the orientation and the bank-conflict argument.
#pragma once
#include "common.h"

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
typedef short s16x4_t __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ f32x16 mfma32(bf16x8_t a, bf16x8_t b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ bf16x8_t ld8(const bf16_t* p) {
  return *reinterpret_cast<const bf16x8_t*>(p);
}

__device__ __forceinline__ bf16x4_t tr4(const bf16_t* p) {
  typedef __attribute__((address_space(3))) s16x4_t lds_s16x4;
  s16x4_t v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)const_cast<bf16_t*>(p));
  return __builtin_bit_cast(bf16x4_t, v);
}

__device__ __forceinline__ bf16x8_t cat44(bf16x4_t a, bf16x4_t b) {
  return bf16x8_t{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

// registers 8s..8s+7 of an accumulator → bf16 fragment (k-step s of a following MFMA)
__device__ __forceinline__ bf16x8_t acc_frag(const f32x16& x, int s) {
  bf16x8_t r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = (__bf16)x[8 * s + j];
  return r;
}

// value of x in the other 32-lane half (lane ^ 32)
__device__ __forceinline__ float half_max(float x) {
  auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float half_sum(float x) {
  auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// row index (within a 32x32 C tile) of accumulator register i for lane half hh
__device__ __forceinline__ int crow(int i, int hh) { return (i & 3) + 8 * (i >> 2) + 4 * hh; }

// ---------------------------------------------------------------- swizzled LDS image
__device__ __forceinline__ int swz(int row) {
  const int u = (row >> 1) & 7;
  return ((u & 1) << 2) | (u & 2) | (u >> 2);  // bit0 <-> bit2 of (row>>1)&7
}
// element offset of 16-B chunk `ch` (0..7) of row `row`
__device__ __forceinline__ int img_off(int row, int ch) { return row * 64 + ((ch ^ swz(row)) << 3); }

// Lane-constant offsets. Row read of a 32-row operand block starting at row 32x:
// lane (r, hh) reads row 32x + r, chunk 2kk + hh → offset 2048x + rowoff[kk].
// Transposed read (k rows kb + 4hh + 8e + q, columns 32dt + 16(g&1) + 4p) for a
// k-block starting at kb (multiple of 16): offset 64*kb + troff[e][dt].
struct LaneOffs {
  int row[4];
  int tr[2][2];
  __device__ __forceinline__ LaneOffs(int lane) {
    const int r = lane & 31, hh = lane >> 5, g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) row[kk] = img_off(r, 2 * kk + hh);
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        const int col = 32 * dt + 16 * (g & 1) + 4 * p;
        tr[e][dt] = img_off(4 * hh + 8 * e + q, col >> 3) + (col & 7);
      }
  }
};

// operand fragment with k down the image's rows: k = kb + {4hh+0..3, 8+4hh+0..3}
// (the acc_frag k order), column 32dt + (lane&31)
__device__ __forceinline__ bf16x8_t tr_frag(const bf16_t* img, const LaneOffs& lo, int kb, int dt) {
  return cat44(tr4(img + 64 * kb + lo.tr[0][dt]), tr4(img + 64 * kb + lo.tr[1][dt]));
}

// ---------------------------------------------------------------- the forward's tile
// One 64-key tile of the forward (attn_fwd_kernel, attn_extend_kernel) for a wave's 32
// queries: S^T = K.Q^T from the K image `Ks`, the online softmax in the log2 domain, then
// O^T += V^T.P^T from the V image `Vs`. `qf`: the lane's Q fragments; `kv0`: the tile's first
// key; `qpos`: the last key this lane's query attends to (read on a kDiag tile only, which
// masks the keys past it with a select, never an add); `o`, `m_run`, `l_run`: the lane's
// running output, max and sum.
template <bool kDiag>
__device__ __forceinline__ void fwd_tile(const bf16_t* Ks, const bf16_t* Vs, const LaneOffs& lo,
                                         const bf16x8_t (&qf)[4], int kv0, int qpos, int hh,
                                         float sc_log2, f32x16 (&o)[2], float& m_run,
                                         float& l_run) {
  f32x16 st[2];
#pragma unroll
  for (int kt = 0; kt < 2; ++kt) {
    st[kt] = f32x16{};
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
      st[kt] = mfma32(ld8(Ks + 2048 * kt + lo.row[kk]), qf[kk], st[kt]);
  }
  if (kDiag) {
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (kv0 + 32 * kt + crow(i, hh) > qpos) st[kt][i] = -INFINITY;
  }
  float mt = st[0][0];
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int i = 0; i < 16; ++i) mt = fmaxf(mt, st[kt][i]);
  mt = half_max(mt) * sc_log2;
  // Lazy rescaling: the running max moves (and O / l are rescaled) only when some query's
  // tile max exceeds it by more than 8 (log2 units). Otherwise the stale max stays,
  // p <= 2^8 — exact in fp32, and the final O / l is unchanged: the common tile skips the 32
  // multiplies of the O rescale and the exp of alpha. A wave-uniform branch (the first tile
  // always takes it: m_run = -inf).
  if (__builtin_amdgcn_ballot_w64(mt > m_run + 8.f)) {
    const float m_new = fmaxf(m_run, mt);
    const float alpha = fast_exp2(m_run - m_new);
    l_run *= alpha;
    m_run = m_new;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int i = 0; i < 16; ++i) o[dt][i] *= alpha;
  }
  float ls = 0.f;
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float p = fast_exp2(fmaf(st[kt][i], sc_log2, -m_run));
      st[kt][i] = p;
      ls += p;
    }
  l_run += half_sum(ls);
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
        o[dt] = mfma32(tr_frag(Vs, lo, 32 * kt + 16 * s, dt), acc_frag(st[kt], s), o[dt]);
}

// ---------------------------------------------------------------- tile staging
// [64 rows][64] bf16 tile; 256 threads x 2 chunks
// native vector type: HIP's uint4 is a struct, whose copies lower to memcpy through a
// stack slot (scratch) that SROA cannot promote
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
struct TileRegs {
  u32x4 v0, v1;
};
struct KV {
  TileRegs k, v;
};

// member-wise (a struct assignment may lower to memcpy, see u32x4 above)
__device__ __forceinline__ void kv_move(KV& d, const KV& s) {
  d.k.v0 = s.k.v0;
  d.k.v1 = s.k.v1;
  d.v.v0 = s.v.v0;
  d.v.v1 = s.v.v1;
}

__device__ __forceinline__ void tile_store(const TileRegs& r, bf16_t* img) {
  const int c = threadIdx.x;
  *reinterpret_cast<u32x4*>(img + img_off(c >> 3, c & 7)) = r.v0;
  *reinterpret_cast<u32x4*>(img + img_off((c + 256) >> 3, c & 7)) = r.v1;
}

// The epilogues' staging regions are wave-private: LDS operations of one wave execute in
// order, so only the compiler has to be kept from moving the reads above the writes — no
// workgroup barrier.
__device__ __forceinline__ void wave_lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
