// attn_stream_tile.h -- the frame shared by the two streamed-softmax attention kernels, hubert_attn_fwd_kernel (hubert.hip)
// and rel_attn_stream_fwd_kernel (attention_stream.hip), as plain functions over the arrays those kernels declare.
//
// A block is one head and 128 queries: each of its 4 waves owns 32 queries for the whole launch and the block streams the
// keys / values in TILES OF 32 KEYS through LDS; nothing of size T x T exists.  A head is D rows of T floats, T contiguous.
// Both contractions run on v_mfma_f32_32x32x2_f32 (exact fp32 products, whatever the compute mode):
//   S^T[s][t] = sum_d K[d][s] Q[d][t]   A = K tile from LDS, B = this lane's query column (pre-scaled) in registers;
//   O[d][t]  += sum_s V[d][s] P^T[s][t]  A = V tile from LDS, B = the S^T accumulator itself.
// Layout: a lane is a query, col = lane & 31, and a half, hf = lane >> 5.  S^T leaves the matrix pipe with 16 of the tile's
// 32 keys in the lane's registers (the other 16 in lane ^ 32): register r is key acc_row(r, hf) = (r&3) + 8*(r>>2) + 4*hf
// (common.h).  So the running max / sum of a query is a loop over registers plus one exchange with lane ^ 32, and register
// r is already the B operand of the k-pair {acc_row(r, 0), acc_row(r, 1)} of the second product: no LDS round trip for P.
// The same map gives the channel of register r of an output tile o[j]: j * 32 + acc_row(r, hf).
// LDS: Ks[D * 32] is [d][key]; Vs is [d][TILE_VS] with TILE_VS = 33, because the A fragments of the second product walk d
// across the 32 lanes of a half at one key: a stride of 32 would put them all in one bank, 33 gives each its own.
#pragma once
#include "common.h"
#include <math.h>

constexpr int TILE_VS = 33;  // row stride of the value tile

// qr[i] = scale * q[2i + hf][t], the lane's B operand of every score product; 0 where the query does not exist.  One
// branch around all the loads: a select per element makes the compiler carry qr as one wide value through D / 2 branches.
template <int D>
__device__ __forceinline__ void tile_load_q(float (&qr)[D / 2], const float* __restrict__ q, size_t base, int T, int t, int hf,
                                            float scale, bool ok) {
#pragma unroll
  for (int i = 0; i < D / 2; ++i) qr[i] = 0.f;
  if (ok)
#pragma unroll
    for (int i = 0; i < D / 2; ++i) qr[i] = q[base + (size_t)(2 * i + hf) * T + t] * scale;
}

// keys / values s0 .. s0 + 31 of the head at `base` into Ks / Vs by all 256 threads; keys at or past n are staged as 0 by a
// select and never read from memory.  The caller puts the block's barriers around it.
template <int D>
__device__ __forceinline__ void tile_stage_kv(float* Ks, float* Vs, const float* __restrict__ k, const float* __restrict__ v,
                                              size_t base, int T, int s0, int n, int tid) {
  const int sd = tid >> 5, sc = tid & 31;
  const int s = s0 + sc;
  const bool sok = s < n;
#pragma unroll
  for (int i = 0; i < D / 8; ++i) {
    const int d = sd + 8 * i;
    const size_t g = base + (size_t)d * T + (sok ? s : 0);
    Ks[d * 32 + sc] = sok ? k[g] : 0.f;
    Vs[d * TILE_VS + sc] = sok ? v[g] : 0.f;
  }
}

template <int D>
__device__ __forceinline__ f32x16 tile_scores(const float* Ks, const float (&qr)[D / 2], int col, int hf) {
  f32x16 S = {};
#pragma unroll
  for (int i = 0; i < D / 2; ++i) S = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[(2 * i + hf) * 32 + col], qr[i], S, 0, 0, 0);
  return S;
}

// One step of the streamed softmax: S becomes exp(S - new max) in place, m / l are updated, and the factor alpha that
// rescales everything accumulated under the old max is returned.  The new max must be finite (key 0 exists and the callers
// fill with -inf only behind the last key).  FAST_EXP is the one place where the two kernels differ inside the frame:
// false is expf (the library's exponential, HuBERT), true is __expf (the v_exp_f32 intrinsic, as in the fused kernels of
// attention.hip that the rel-pos kernel is routed against).  Each kernel's parity figures and bit checks were taken with
// its own choice, so it is the caller's to make and changing it changes that kernel's bits.
template <bool FAST_EXP>
__device__ __forceinline__ float tile_softmax_step(f32x16& S, float& m, float& l) {
  float mx = -INFINITY;
#pragma unroll
  for (int r = 0; r < 16; ++r) mx = fmaxf(mx, S[r]);
  mx = fmaxf(mx, __shfl_xor(mx, 32));
  const float mn = fmaxf(m, mx);
  const float alpha = FAST_EXP ? __expf(m - mn) : expf(m - mn);
  float rs = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    S[r] = FAST_EXP ? __expf(S[r] - mn) : expf(S[r] - mn);
    rs += S[r];
  }
  rs += __shfl_xor(rs, 32);
  l = l * alpha + rs;
  m = mn;
  return alpha;
}

// o = o * alpha + V P^T for the tile in Vs (DT * 32 rows) and the probabilities in S
template <int DT>
__device__ __forceinline__ void tile_pv(f32x16 (&o)[DT], const float* Vs, const f32x16& S, float alpha, int col, int hf) {
#pragma unroll
  for (int j = 0; j < DT; ++j) o[j] *= alpha;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int sr = acc_row(r, hf);
#pragma unroll
    for (int j = 0; j < DT; ++j)
      o[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[(j * 32 + col) * TILE_VS + sr], S[r], o[j], 0, 0, 0);
  }
}

// out[d][t] = o / l for the channels d < D of the head at `obase`; exact 0 by a select where the query is not `live`
template <int D, int DT>
__device__ __forceinline__ void tile_store(float* __restrict__ out, size_t obase, int T, int t, const f32x16 (&o)[DT], float l,
                                           int hf, bool live) {
  const float inv = 1.f / l;
#pragma unroll
  for (int j = 0; j < DT; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int d = j * 32 + acc_row(r, hf);
      if (d < D) out[obase + (size_t)d * T + t] = live ? o[j][r] * inv : 0.f;
    }
}
