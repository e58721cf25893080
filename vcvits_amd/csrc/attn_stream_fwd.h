// attn_stream_fwd.h -- the two streamed forward passes on the frame of attn_stream_tile.h, each written ONCE over an operand
// policy (TileF32 / TileBF16 there), and the launchers of their kernels.  The __global__ kernels in attention_stream.hip,
// attention_stream_bf16.hip, attention_stream_grad.hip and hubert.hip are one call of a body each; a further operand type is
// a policy and an instantiation, a further per-tile step of the rel-pos forward is a hook.
//   rel_attn_stream_fwd_body<P, Hook>  relative-position attention: the fill, the banded relative keys and values
//     (attention_stream.hip describes them).  Hook is the training kernel's dropout and stats; inference passes NoHook.
//   hubert_attn_fwd_body<P, LEN>       plain softmax attention with optional per-row lengths (hubert.hip describes them).
// The LDS arrays live in the bodies: a kernel's static LDS is that of the body it calls.
#pragma once
#include "attn_stream_tile.h"

constexpr int RELS = 16;  // relative positions at most (2w + 1 <= 16, as the fused kernels)
constexpr int RS = 18;    // row stride of the band tables: lane l reads offset c - l, so l * (RS - 1) walks the banks

// The hook of the rel-pos body that does nothing.  tile(): after the softmax step of the key tile at s0 (the row sum l has
// taken the exponentials already), before the carries and the band store, with S the lane's exp(s - m) and i its query (0
// for a lane without one).  done(): after the store, for the lanes whose query t exists, with the final max and sum.
struct NoHook {
  __device__ __forceinline__ void tile(f32x16&, int, int, int) const {}
  __device__ __forceinline__ void done(int, int, float, float) const {}
};

template <class P, class Hook>
__device__ __forceinline__ void rel_attn_stream_fwd_body(const float* __restrict__ q, const float* __restrict__ k,
                                                         const float* __restrict__ v, const float* __restrict__ embk,
                                                         const float* __restrict__ embv, const float* __restrict__ mask,
                                                         float* __restrict__ out, int H, int T, int w, float qscale,
                                                         const Hook& hook) {
  constexpr int D = P::D, DT = D / 32;  // output tiles of 32 channels
  __shared__ __attribute__((aligned(P::ALIGN))) typename P::elem Ks[P::KN];
  __shared__ __attribute__((aligned(P::ALIGN))) typename P::elem Vs[D * P::VS];
  __shared__ __attribute__((aligned(16))) float Ms[32];
  __shared__ float Ek[RELS * D];
  __shared__ float Ev[RELS * D];
  __shared__ float Rl[128 * RS];  // rel[r] of the block's queries
  __shared__ float Pb[128 * RS];  // un-normalised band probabilities (after the hook)
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int col = lane & 31, hf = lane >> 5;
  const int nr = 2 * w + 1;
  const size_t base = (size_t)blockIdx.y * D * T;
  const size_t mbase = (size_t)(blockIdx.y / H) * T;
  const int t0 = blockIdx.x * 128 + wv * 32;  // first query of the wave
  const int t = t0 + col;
  const bool tok = t < T;
  const int row = (wv * 32 + col) * RS;

  float qf[D / 2];  // the lane's fp32 query view: the band terms are formed from it
  typename P::qop qo;  // the score operand; for fp32 operands pack_q copies, and qo and qf are the same registers
  P::load_q(qf, q, base, T, t, hf, qscale, tok);
  P::pack_q(qo, qf);
  const float mi = tok ? mask[mbase + t] : 0.f;
  for (int i = tid; i < RELS * D; i += 256) {
    Ek[i] = i < nr * D ? embk[i] : 0.f;
    Ev[i] = i < nr * D ? embv[i] : 0.f;
  }
  for (int i = tid; i < 128 * RS; i += 256) Pb[i] = 0.f;
  __syncthreads();
  // rel[r] = q_i . embk[r] from the fp32 q: each lane sums its channels, the two halves of a query meet through lane ^ 32
  for (int r = 0; r < nr; ++r) {
    float a = 0.f;
#pragma unroll
    for (int i = 0; i < D / 2; ++i) a += qf[i] * Ek[r * D + P::chan(i, hf)];
    a += __shfl_xor(a, 32);
    if (hf == 0) Rl[row + r] = P::rel_term(a, qscale);
  }

  f32x16 o[DT] = {};
  float m = -INFINITY, l = 0.f;
  float c0 = 0.f, c1 = 0.f, c2 = 0.f;  // rescale carried by the band entries of the tiles at t0 - 32, t0, t0 + 32

  for (int s0 = 0; s0 < T; s0 += 32) {
    __syncthreads();  // the previous tile has been read (first pass: Rl is written)
    P::stage_kv(Ks, Vs, k, v, base, T, s0, T, tid);
    if (tid < 32) Ms[tid] = s0 + tid < T ? mask[mbase + s0 + tid] : 0.f;
    __syncthreads();
    f32x16 S = P::scores(Ks, qo, qscale, col, hf);

    const int ds = s0 - t0;
    const bool band = ds >= -32 && ds <= 32;  // wave-uniform
    if (band) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int off = ds + acc_row(r, hf) - col + w;  // key - query + w
        const bool inb = off >= 0 && off < nr;
        const float rel = Rl[row + (inb ? off : 0)];
        S[r] += inb ? rel : 0.f;
      }
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 mj = *reinterpret_cast<const float4*>(&Ms[8 * g + 4 * hf]);
      S[4 * g + 0] = mi * mj.x == 0.f ? -1e4f : S[4 * g + 0];
      S[4 * g + 1] = mi * mj.y == 0.f ? -1e4f : S[4 * g + 1];
      S[4 * g + 2] = mi * mj.z == 0.f ? -1e4f : S[4 * g + 2];
      S[4 * g + 3] = mi * mj.w == 0.f ? -1e4f : S[4 * g + 3];
    }
    if (s0 + 32 > T) {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (s0 + acc_row(r, hf) >= T) S[r] = -INFINITY;
    }
    // the new max is finite from the first tile on: key 0 exists and is -1e4 at the least
    const float alpha = tile_softmax_step<true>(S, m, l);
    hook.tile(S, s0, tok ? t : 0, hf);
    c0 *= alpha, c1 *= alpha, c2 *= alpha;
    if (band) {
      if (ds < 0) c0 = 1.f;
      else if (ds == 0) c1 = 1.f;
      else c2 = 1.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int sr = acc_row(r, hf);
        const int off = ds + sr - col + w;
        if (off >= 0 && off < nr && s0 + sr < T) Pb[row + off] = S[r];
      }
    }
    P::pv(o, Vs, S, alpha, col, hf);
  }

  __syncthreads();  // both lanes of a query read the band entries either of them wrote
  if (!tok) return;
  // relative values: entry r belongs to key t + r - w, i.e. to the tile at t0 - 32, t0 or t0 + 32
  for (int r = 0; r < nr; ++r) {
    const int rel = col + r - w;  // key - t0
    const float p = Pb[row + r] * (rel < 0 ? c0 : rel < 32 ? c1 : c2);
#pragma unroll
    for (int j = 0; j < DT; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) o[j][e] += p * Ev[r * D + j * 32 + acc_row(e, hf)];
  }
  tile_store<D>(out, base, T, t, o, l, hf, true);
  hook.done(t, hf, m, l);
}

template <class P, bool LEN>
__device__ __forceinline__ void hubert_attn_fwd_body(const float* __restrict__ q, const float* __restrict__ k,
                                                     const float* __restrict__ v, float* __restrict__ out, int H, int T,
                                                     size_t ldb, float scale, const int* __restrict__ frames) {
  constexpr int D = P::D, DT = (D + 31) / 32;  // output tiles of 32 channels
  __shared__ __attribute__((aligned(P::ALIGN))) typename P::elem Ks[P::KN];
  __shared__ __attribute__((aligned(P::ALIGN))) typename P::elem Vs[DT * 32 * P::VS];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int col = lane & 31, hf = lane >> 5;
  const size_t base = (size_t)(blockIdx.y / H) * ldb + (size_t)(blockIdx.y % H) * D * T;
  const size_t obase = (size_t)blockIdx.y * D * T;
  const int t = blockIdx.x * 128 + wv * 32 + col;
  const bool tok = t < T;
  int n = T;  // keys (and queries) that exist
  if (LEN) {
    n = min(max(frames[blockIdx.y / H], 1), T);
    if ((int)blockIdx.x * 128 >= n) {
      if (tok)
#pragma unroll
        for (int i = 0; i < D / 2; ++i) out[obase + (size_t)(2 * i + hf) * T + t] = 0.f;
      return;
    }
  }
  const bool qok = t < n;

  typename P::qop qo;
  {
    float qf[D / 2];
    P::load_q(qf, q, base, T, t, hf, scale, qok);
    P::pack_q(qo, qf);
  }
  for (int i = D * P::VS + tid; i < DT * 32 * P::VS; i += 256) Vs[i] = (typename P::elem)0.f;
  f32x16 o[DT] = {};
  float m = -INFINITY, l = 0.f;

  for (int s0 = 0; s0 < n; s0 += 32) {
    __syncthreads();  // the previous tile has been read
    P::stage_kv(Ks, Vs, k, v, base, T, s0, n, tid);
    __syncthreads();
    f32x16 S = P::scores(Ks, qo, scale, col, hf);
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if (s0 + acc_row(r, hf) >= n) S[r] = -INFINITY;
    const float alpha = tile_softmax_step<false>(S, m, l);
    P::pv(o, Vs, S, alpha, col, hf);
  }

  if (tok) tile_store<D>(out, obase, T, t, o, l, hf, !LEN || qok);
}

// The launchers, over a kernel family F: a struct whose kernel<D>() (rel-pos) or kernel<D, LEN>() (HuBERT) returns the
// __global__ instance, so the fp32 and the bf16 entry points share their refusals and their grid.
template <class F>
static int rel_attn_stream_launch(const float* q, const float* k, const float* v, const float* embk, const float* embv,
                                  const float* mask, float* out, int B, int H, int dk, int T, int w, float qscale, void* stream) {
  if (!q || !k || !v || !embk || !embv || !mask || !out || vcv_rel_attn_stream_supported(B, H, dk, T, w) != 0) return VCV_EINVAL;
  const auto kernel = dk == 64 ? F::template kernel<64>() : F::template kernel<32>();
  kernel<<<dim3(vcv_cdiv(T, 128), B * H), 256, 0, (hipStream_t)stream>>>(q, k, v, embk, embv, mask, out, H, T, w, qscale);
  return vcv_check_launch();
}

// frames: null launches the kernel without lengths
template <class F>
static int hubert_attn_launch(const float* q, const float* k, const float* v, float* out, int B, int H, int dk, int T, int64_t ldb,
                              float scale, const int* frames, void* stream) {
  if (!q || !k || !v || !out || vcv_hubert_attn_supported(B, H, dk, T) != 0 || ldb < (int64_t)H * dk * T) return VCV_EINVAL;
  const auto kernel = dk == 64 ? (frames ? F::template kernel<64, true>() : F::template kernel<64, false>())
                               : (frames ? F::template kernel<80, true>() : F::template kernel<80, false>());
  kernel<<<dim3(vcv_cdiv(T, 128), B * H), 256, 0, (hipStream_t)stream>>>(q, k, v, out, H, T, (size_t)ldb, scale, frames);
  return vcv_check_launch();
}
