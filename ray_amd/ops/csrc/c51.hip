// Fused C51 (categorical DQN, Bellemare et al. 2017) projection loss for the Rainbow
// learner: one launch reads the three network outputs of a DQN update and writes the
// per-row cross-entropy, its gradient wrt the online logits, the selected next action
// and (optionally) the projected target distribution.
//
// Reference semantics: rllib/algorithms/dqn/torch/dqn_torch_learner.py (num_atoms > 1)
// and ray_amd.ops.reference.c51_loss (floor/ceil + scatter_add form).
//
// Layout: one wave per batch row, lane k = atom k (2 <= K <= 64), four rows per
// 256-thread block. Per row:
//   1) for every action a: softmax over atoms of the selecting net (online net at
//      next_obs for double-Q, else the target net) and its expected value
//      sum_k z_k p_k; keep the argmax (lowest index on ties, as torch.argmax);
//   2) p = softmax(next_target[b, a*]);
//   3) b_j = (clamp(r + disc (1 - term) z_j, v_min, v_max) - v_min) / dz;
//   4) projection as a GATHER: m_i = sum_j p_j max(0, 1 - |b_j - i|). Lane i loops
//      over j with (b_j, p_j) broadcast from lane j: the same hat-function weights as
//      the floor/ceil scatter, but no write conflicts, no float atomics, and an integer
//      b_j (l == u) needs no special case;
//   5) ce = -sum_i m_i log_softmax(logits[b, a_b])_i and
//      dlogits[b, a_b] = w_b / B (softmax - m), exactly 0 on the other A - 1 rows.
// The scalar loss sum_b w_b ce_b / B is formed by a one-block second kernel that adds
// in a fixed order: the same inputs give the same bits every run (no float atomics in
// this file).
#include "common.h"

struct C51Args {
  const float* logits;       // [B,A,K] online net at obs
  const long* actions;       // [B]
  const float* next_online;  // [B,A,K] online net at next_obs; null: select with next_target
  const float* next_target;  // [B,A,K] target net at next_obs
  const float* rewards;      // [B]
  const float* discounts;    // [B] gamma or gamma^n
  const float* terminateds;  // [B]
  const float* weights;      // [B] importance weights; null = 1
  float* ce;                 // [B]
  float* dlogits;            // [B,A,K]
  int* next_action;          // [B]
  float* target_dist;        // [B,K]; null skips it
  int B, A, K;
  float v_min, v_max;
};

// softmax over the K atoms held one per lane (x = -inf on lanes >= K): returns p, and
// the log of the normaliser through *lse (log_softmax = x - *lse)
__device__ __forceinline__ float atom_softmax(float x, bool on, float* lse) {
  const float mx = wave_max(x);
  const float e = on ? __expf(x - mx) : 0.f;
  const float s = wave_sum(e);
  *lse = mx + __logf(s);
  return e / s;
}

__global__ __launch_bounds__(256) void c51_loss_kernel(C51Args p) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= p.B) return;  // whole waves leave together; the kernel has no block barrier
  const int A = p.A, K = p.K;
  const bool on = lane < K;
  const float dz = (p.v_max - p.v_min) / (float)(K - 1);
  const float z = p.v_min + dz * (float)lane;
  const long row = (long)b * A * K;

  // 1) greedy next action under the selecting net's expected values
  const float* sel = p.next_online ? p.next_online : p.next_target;
  float best = -INFINITY, lse;
  int na = 0;
  for (int a = 0; a < A; ++a) {
    const float x = on ? sel[row + (long)a * K + lane] : -INFINITY;
    const float pr = atom_softmax(x, on, &lse);
    const float q = wave_sum(on ? pr * z : 0.f);  // identical on every lane (xor butterfly)
    if (q > best) {
      best = q;
      na = a;
    }
  }
  // 2) target net's distribution of that action
  const float xt = on ? p.next_target[row + (long)na * K + lane] : -INFINITY;
  const float pt = atom_softmax(xt, on, &lse);
  // 3) Bellman-shifted atom positions in units of dz
  const float r = p.rewards[b];
  const float g = p.discounts[b] * (1.f - p.terminateds[b]);
  const float tz = fminf(fmaxf(r + g * z, p.v_min), p.v_max);
  const float bj = fminf(fmaxf((tz - p.v_min) / dz, 0.f), (float)(K - 1));
  // 4) gather projection
  float m = 0.f;
  const float fi = (float)lane;
  for (int j = 0; j < K; ++j) {
    const float pj = __shfl(pt, j, 64);
    const float bb = __shfl(bj, j, 64);
    m += pj * fmaxf(0.f, 1.f - fabsf(bb - fi));
  }
  if (!on) m = 0.f;
  // 5) cross-entropy against the taken action's logits, and its gradient
  const long act = p.actions[b];
  const bool ok = act >= 0 && act < A;  // a bad action index reads nothing: ce = NaN
  const float xa = (on && ok) ? p.logits[row + act * K + lane] : -INFINITY;
  const float pa = atom_softmax(xa, on && ok, &lse);
  const float ce = -wave_sum(on && ok ? m * (xa - lse) : 0.f);
  const float w = (p.weights ? p.weights[b] : 1.f) / (float)p.B;
  if (on) {
    for (int a = 0; a < A; ++a)
      p.dlogits[row + (long)a * K + lane] = (a == act) ? w * (pa - m) : 0.f;
    if (p.target_dist) p.target_dist[(long)b * K + lane] = m;
  }
  if (lane == 0) {
    p.ce[b] = ok ? ce : NAN;
    p.next_action[b] = na;
  }
}

// loss[0] = sum_b w_b ce_b / B: thread t adds rows t, t + 256, ... in order, then one
// block reduction (fixed order: deterministic)
__global__ __launch_bounds__(256) void c51_mean_kernel(const float* __restrict__ ce,
                                                       const float* __restrict__ weights, int B,
                                                       float* __restrict__ loss) {
  __shared__ float red[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < B; i += 256) s += ce[i] * (weights ? weights[i] : 1.f);
  const float t = block_sum<4>(s, red);
  if (threadIdx.x == 0) loss[0] = t / (float)B;
}

// loss may be null (no scalar reduction). Runs on the caller's stream; no host
// synchronisation, no allocation.
RA_EXPORT int ra_c51_loss(const float* logits, const long* actions, const float* next_online,
                          const float* next_target, const float* rewards,
                          const float* discounts, const float* terminateds,
                          const float* weights, float* ce, float* dlogits, int* next_action,
                          float* target_dist, float* loss, int B, int A, int K, float v_min,
                          float v_max, hipStream_t st) {
  if (B <= 0 || A <= 0 || K < 2 || K > 64 || !(v_min < v_max)) return hipErrorInvalidValue;
  C51Args p{logits, actions, next_online, next_target, rewards, discounts, terminateds, weights,
            ce, dlogits, next_action, target_dist, B, A, K, v_min, v_max};
  hipLaunchKernelGGL(c51_loss_kernel, dim3((B + 3) / 4), dim3(256), 0, st, p);
  if (loss) hipLaunchKernelGGL(c51_mean_kernel, dim3(1), dim3(256), 0, st, ce, weights, B, loss);
  return hipGetLastError();
}
