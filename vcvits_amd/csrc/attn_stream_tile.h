// attn_stream_tile.h -- the frame shared by the streamed-softmax attention kernels: the HuBERT forward (hubert.hip), the
// relative-position forward (attention_stream.hip), its training form (attention_stream_grad.hip) and the bf16-operand forms
// of the first two (attention_stream_bf16.hip).  This file holds the tile primitives, as plain functions over the arrays of
// a kernel, and the two OPERAND POLICIES TileF32 / TileBF16 (end of file) that group them; attn_stream_fwd.h, beside it,
// holds the two forward bodies, each written once over a policy, and their launchers.
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
//
// The bf16-operand form of the same frame is the second half of this file: the *_bf16 functions replace the three that
// touch operands, everything else above is shared as it is.  Its LDS images and their strides are described there.
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

// =====================================================================================================================
// bf16 operands (attention_stream_bf16.hip): the same block, tiles, lane layout and streamed softmax, with both
// contractions on v_mfma_f32_32x32x16_bf16.  K, V and Q are rounded to bf16 (nearest even) on the way in, the probabilities
// on the way into the second product; scores, max, sum, alpha and the output accumulate in fp32 as above.
//   S^T = K Q: D / 16 MFMAs.  A = 8 channels 16 * step + 8 * hf + e of key lane & 31, B = the same 8 channels of the lane's
//   query, packed bf16 and UNSCALED (D / 4 registers); the scale multiplies the fp32 score, so bf16 inputs give the exact
//   products whatever the scale.
//   O += V P^T: the C/D layout is the fp32 one, so registers 8 m .. 8 m + 7 of S, cast to bf16, are the B fragment of MFMA
//   m (m = 0, 1) of each 32-channel output tile: reduction element 8 * hf + e of MFMA m is key acc_row(8 m + e, hf), i.e. the
//   two 4-key runs 16 m + 4 hf .. + 3 and 16 m + 8 + 4 hf .. + 3, which is what the A fragment reads from the value tile.
// LDS: Ks is [key][TILE_KS(D)] bf16, channel innermost, so an A fragment of the scores is one 16-byte read.  TILE_KS = D + 8:
// ds_read_b128 serves 16 lanes per cycle (keys that are distinct mod 16, one half), each 4 dwords wide; the row stride is
// D / 2 + 4 dwords, which is 4 mod 8 for D = 32, 64, 80, so key * stride walks the 16 four-dword bank groups of the 64 banks
// once: conflict-free, and rows stay 16-byte aligned.  An unpadded D / 2 would put every key of D = 64 on the same banks.
// Vs is [channel][TILE_VSB] bf16, key innermost, so an A fragment of the second product is two 8-byte reads.  TILE_VSB = 36:
// ds_read_b64 serves the 32 channels of a half per cycle at one key offset, 2 dwords each; the stride of 18 dwords is 2 mod
// 4, so channel * 18 walks the 32 two-dword bank pairs once (16 dwords, the unpadded tile, would hit each pair twice over).
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

constexpr int TILE_VSB = 36;                                   // row stride of the bf16 value tile, in elements
constexpr int tile_ks(int D) { return D + 8; }                 // row stride of the bf16 key tile, in elements

// qf[8 i + e] = q[16 i + 8 hf + e][t] in fp32 and unscaled: the channels of the lane's B fragments; 0 where the query does
// not exist (one branch around all the loads, as tile_load_q)
template <int D>
__device__ __forceinline__ void tile_load_q_bf16(float (&qf)[D / 2], const float* __restrict__ q, size_t base, int T, int t,
                                                 int hf, bool ok) {
#pragma unroll
  for (int i = 0; i < D / 2; ++i) qf[i] = 0.f;
  if (ok)
#pragma unroll
    for (int i = 0; i < D / 2; ++i) qf[i] = q[base + (size_t)(16 * (i >> 3) + 8 * hf + (i & 7)) * T + t];
}

// the lane's B operands of every score product: qf rounded to bf16, D / 4 registers
template <int D>
__device__ __forceinline__ void tile_pack_q_bf16(bf16x8 (&qb)[D / 16], const float (&qf)[D / 2]) {
#pragma unroll
  for (int i = 0; i < D / 16; ++i)
#pragma unroll
    for (int e = 0; e < 8; ++e) qb[i][e] = (__bf16)qf[8 * i + e];
}

// keys / values s0 .. s0 + 31 of the head at `base`, rounded to bf16, into Ks ([key][channel]) / Vs ([channel][key]) by
// all 256 threads: a thread is one key and D / 8 adjacent channels, so its keys leave as one packed run.  Keys at or past n
// are staged as 0 by a select and never read from memory.  The caller puts the block's barriers around it.
template <int D>
__device__ __forceinline__ void tile_stage_kv_bf16(__bf16* Ks, __bf16* Vs, const float* __restrict__ k,
                                                   const float* __restrict__ v, size_t base, int T, int s0, int n, int tid) {
  constexpr int CH = D / 8, KS = tile_ks(D);
  const int sc = tid & 31, c0 = (tid >> 5) * CH;
  const int s = s0 + sc;
  const bool sok = s < n;
  __bf16 kk[CH];
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    const size_t g = base + (size_t)(c0 + i) * T + (sok ? s : 0);
    kk[i] = (__bf16)(sok ? k[g] : 0.f);
    Vs[(c0 + i) * TILE_VSB + sc] = (__bf16)(sok ? v[g] : 0.f);
  }
  __bf16* kd = Ks + sc * KS + c0;
  if constexpr (CH == 8) {
    bf16x8 w;
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = kk[i];
    *reinterpret_cast<bf16x8*>(kd) = w;  // 16 * (9 sc + sd) bytes into the tile
  } else if constexpr (CH == 4) {
    bf16x4 w = {kk[0], kk[1], kk[2], kk[3]};
    *reinterpret_cast<bf16x4*>(kd) = w;  // 8 * (10 sc + sd) bytes
  } else {
#pragma unroll
    for (int i = 0; i < CH; i += 2) {
      bf16x2 w = {kk[i], kk[i + 1]};
      *reinterpret_cast<bf16x2*>(kd + i) = w;  // CH is even: 4-byte aligned
    }
  }
}

// S^T = scale * (K Q) for the tile in Ks
template <int D>
__device__ __forceinline__ f32x16 tile_scores_bf16(const __bf16* Ks, const bf16x8 (&qb)[D / 16], float scale, int col, int hf) {
  f32x16 S = {};
#pragma unroll
  for (int i = 0; i < D / 16; ++i) {
    const bf16x8 a = *reinterpret_cast<const bf16x8*>(Ks + col * tile_ks(D) + 16 * i + 8 * hf);
    S = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, qb[i], S, 0, 0, 0);
  }
  return S * scale;
}

// o = o * alpha + V P^T for the tile in Vs (DT * 32 rows) and the probabilities in S, rounded to bf16 here and only here
template <int DT>
__device__ __forceinline__ void tile_pv_bf16(f32x16 (&o)[DT], const __bf16* Vs, const f32x16& S, float alpha, int col, int hf) {
#pragma unroll
  for (int j = 0; j < DT; ++j) o[j] *= alpha;
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    bf16x8 b;
#pragma unroll
    for (int e = 0; e < 8; ++e) b[e] = (__bf16)S[8 * m + e];
#pragma unroll
    for (int j = 0; j < DT; ++j) {
      const __bf16* vr = Vs + (j * 32 + col) * TILE_VSB + 16 * m + 4 * hf;  // key acc_row(8 m, hf)
      const bf16x4 lo = *reinterpret_cast<const bf16x4*>(vr), hi = *reinterpret_cast<const bf16x4*>(vr + 8);
      const bf16x8 a = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      o[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, o[j], 0, 0, 0);
    }
  }
}

// =====================================================================================================================
// Operand policies: what a forward body (attn_stream_fwd.h) takes as its template argument.  A policy is the LDS element type
// and the shapes of the two tiles, the lane's score operand, the three functions that touch operands, which channel element i
// of the lane's fp32 query view qf[D / 2] holds, and where the scale goes.  The functions above are the policies'
// implementations: a forward body reaches them through its policy only (tile_load_q is the column loader of the backward
// kernels of attention_stream_grad.hip as well).  Where the scale goes is part of each kernel's bits:
//   TileF32   qf = q * scale on load; a band term rel[r] is the sum of qf . embk[r] as it is; the scores take no further scale.
//   TileBF16  qf = q; rel[r] = (sum of qf . embk[r]) * scale, from the fp32 qf before it is packed; the fp32 score is
//             multiplied by the scale after the MFMAs.
template <int D_>
struct TileF32 {
  static constexpr int D = D_;
  typedef float elem;
  static constexpr int ALIGN = 4, KN = D * 32, VS = TILE_VS;  // of both tiles, in bytes; elements of Ks; row stride of Vs
  typedef float qop[D / 2];
  static __device__ __forceinline__ int chan(int i, int hf) { return 2 * i + hf; }
  static __device__ __forceinline__ void load_q(float (&qf)[D / 2], const float* __restrict__ q, size_t base, int T, int t, int hf,
                                                float scale, bool ok) {
    tile_load_q<D>(qf, q, base, T, t, hf, scale, ok);
  }
  static __device__ __forceinline__ float rel_term(float sum, float) { return sum; }
  static __device__ __forceinline__ void pack_q(qop& qo, const float (&qf)[D / 2]) {
#pragma unroll
    for (int i = 0; i < D / 2; ++i) qo[i] = qf[i];
  }
  static __device__ __forceinline__ void stage_kv(elem* Ks, elem* Vs, const float* __restrict__ k, const float* __restrict__ v,
                                                  size_t base, int T, int s0, int n, int tid) {
    tile_stage_kv<D>(Ks, Vs, k, v, base, T, s0, n, tid);
  }
  static __device__ __forceinline__ f32x16 scores(const elem* Ks, const qop& qo, float, int col, int hf) {
    return tile_scores<D>(Ks, qo, col, hf);
  }
  template <int DT>
  static __device__ __forceinline__ void pv(f32x16 (&o)[DT], const elem* Vs, const f32x16& S, float alpha, int col, int hf) {
    tile_pv(o, Vs, S, alpha, col, hf);
  }
};

template <int D_>
struct TileBF16 {
  static constexpr int D = D_;
  typedef __bf16 elem;
  static constexpr int ALIGN = 16, KN = 32 * tile_ks(D), VS = TILE_VSB;
  typedef bf16x8 qop[D / 16];
  static __device__ __forceinline__ int chan(int i, int hf) { return 16 * (i >> 3) + 8 * hf + (i & 7); }
  static __device__ __forceinline__ void load_q(float (&qf)[D / 2], const float* __restrict__ q, size_t base, int T, int t, int hf,
                                                float, bool ok) {
    tile_load_q_bf16<D>(qf, q, base, T, t, hf, ok);
  }
  static __device__ __forceinline__ float rel_term(float sum, float scale) { return sum * scale; }
  static __device__ __forceinline__ void pack_q(qop& qo, const float (&qf)[D / 2]) { tile_pack_q_bf16<D>(qo, qf); }
  static __device__ __forceinline__ void stage_kv(elem* Ks, elem* Vs, const float* __restrict__ k, const float* __restrict__ v,
                                                  size_t base, int T, int s0, int n, int tid) {
    tile_stage_kv_bf16<D>(Ks, Vs, k, v, base, T, s0, n, tid);
  }
  static __device__ __forceinline__ f32x16 scores(const elem* Ks, const qop& qo, float scale, int col, int hf) {
    return tile_scores_bf16<D>(Ks, qo, scale, col, hf);
  }
  template <int DT>
  static __device__ __forceinline__ void pv(f32x16 (&o)[DT], const elem* Vs, const f32x16& S, float alpha, int col, int hf) {
    tile_pv_bf16(o, Vs, S, alpha, col, hf);
  }
};
