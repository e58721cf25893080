// attention_stream.hip -- relative-position self-attention of the content encoder with the keys and values STREAMED
// (vits/model/transformer/relative_attention_transformer.py:150-182), forward only, no dropout, no probability output:
// what long-form inference runs.  Nothing of size T x T exists, so memory is linear in T and T is not bounded by LDS.
//
// The frame -- block, tiles of 32 keys, the two MFMA contractions, which key a lane's register holds -- is the one of
// attn_stream_tile.h, shared with hubert_attn_fwd_kernel (hubert.hip); this kernel takes it with __expf.  What is this
// kernel's own, following tests/attention_f64.py points 1, 2, 4:
//   * fill: a score is -1e4 by SELECT where mask_i * mask_j == 0 (the tile's 32 mask values are staged beside the keys).
//     A masked query is uniform over all T keys; a wholly masked first tile starts the running max at -1e4 and the first
//     real score rescales it away (alpha = exp(-1e4 - max) = 0).  No tile is skipped.  Keys at or past T are -inf.
//   * banded relative keys: rel[r] = (q_i / sqrt(dk)) . embk[r] is formed once per query before the loop and kept in LDS
//     ([128][RS]); only the key tiles that meet the band of the wave's 32 queries -- the wave's own tile and its two
//     neighbours, 2w + 1 <= 16 < 32 -- take the path that adds it (a wave-uniform branch).
//   * banded relative values: in those same tiles the un-normalised band probabilities exp(s - m) go to LDS ([128][RS],
//     each (query, offset) written once, by the lane that holds that key).  A tile's entries are relative to the running
//     max of that tile, so one register per band tile (3) carries the product of the later rescale factors alpha, exactly
//     as the output accumulator is rescaled; at the end out += sum_r pb[r] * carry * embv[r] and everything is scaled by 1 / l.
// Every index that scales with T is size_t.  Grid (ceil(T / 128), B * H), 256 threads.
//
// Resources (hipcc -O3, gfx950, from the code object's metadata; tests/test_attention_stream_cpu.py holds them):
//   dk = 32: 168 registers (16 of them accumulation registers), 57 SGPR, 30,976 B LDS, 0 B scratch, no spills;
//   dk = 64: 244 registers (32 of them accumulation registers), 57 SGPR, 43,392 B LDS, 0 B scratch, no spills.
// So two (dk = 64) or three (dk = 32) workgroups share a CU; 168 is the last register count at which three do.
#include "attn_stream_tile.h"

namespace {

constexpr int RELS = 16;  // relative positions at most (2w + 1 <= 16, as the fused kernels)
constexpr int RS = 18;    // row stride of the two band tables: lane l reads offset c - l, so l * (RS - 1) walks the banks

template <int D>
__global__ void __launch_bounds__(256)
rel_attn_stream_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                           const float* __restrict__ embk, const float* __restrict__ embv, const float* __restrict__ mask,
                           float* __restrict__ out, int H, int T, int w, float qscale) {
  constexpr int DT = D / 32;  // output tiles of 32 channels
  __shared__ float Ks[D * 32];
  __shared__ float Vs[D * TILE_VS];
  __shared__ __attribute__((aligned(16))) float Ms[32];
  __shared__ float Ek[RELS * D];
  __shared__ float Ev[RELS * D];
  __shared__ float Rl[128 * RS];  // rel[r] of the block's queries
  __shared__ float Pb[128 * RS];  // un-normalised band probabilities
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int col = lane & 31, hf = lane >> 5;
  const int nr = 2 * w + 1;
  const size_t base = (size_t)blockIdx.y * D * T;
  const size_t mbase = (size_t)(blockIdx.y / H) * T;
  const int t0 = blockIdx.x * 128 + wv * 32;  // first query of the wave
  const int t = t0 + col;
  const bool tok = t < T;
  const int row = (wv * 32 + col) * RS;

  float qr[D / 2];
  tile_load_q<D>(qr, q, base, T, t, hf, qscale, tok);
  const float mi = tok ? mask[mbase + t] : 0.f;
  for (int i = tid; i < RELS * D; i += 256) {
    Ek[i] = i < nr * D ? embk[i] : 0.f;
    Ev[i] = i < nr * D ? embv[i] : 0.f;
  }
  for (int i = tid; i < 128 * RS; i += 256) Pb[i] = 0.f;
  __syncthreads();
  // rel[r] = q_i . embk[r]: each lane sums its half of the channels, the two halves of a query meet through lane ^ 32
  for (int r = 0; r < nr; ++r) {
    float a = 0.f;
#pragma unroll
    for (int i = 0; i < D / 2; ++i) a += qr[i] * Ek[r * D + 2 * i + hf];
    a += __shfl_xor(a, 32);
    if (hf == 0) Rl[row + r] = a;
  }

  f32x16 o[DT] = {};
  float m = -INFINITY, l = 0.f;
  float c0 = 0.f, c1 = 0.f, c2 = 0.f;  // rescale carried by the band entries of the tiles at t0 - 32, t0, t0 + 32

  for (int s0 = 0; s0 < T; s0 += 32) {
    __syncthreads();  // the previous tile has been read (first pass: Rl is written)
    tile_stage_kv<D>(Ks, Vs, k, v, base, T, s0, T, tid);
    if (tid < 32) Ms[tid] = s0 + tid < T ? mask[mbase + s0 + tid] : 0.f;
    __syncthreads();
    f32x16 S = tile_scores<D>(Ks, qr, col, hf);

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
    tile_pv(o, Vs, S, alpha, col, hf);
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
}

}  // namespace

// 0: the streamed kernel takes this shape (dk 32 or 64, 2w + 1 <= 16, B * H within the grid's y limit, any T >= 1)
extern "C" int vcv_rel_attn_stream_supported(int B, int H, int dk, int T, int w) {
  if (B <= 0 || H <= 0 || T <= 0 || w < 0 || 2 * w + 1 > RELS || (long long)B * H > 65535) return VCV_EINVAL;
  return (dk == 32 || dk == 64) ? 0 : VCV_EINVAL;
}

// out [B, H*dk, T] = attention(q, k, v) with relative keys / values embk, embv [2w+1, dk] and mask [B, T]; no dropout
extern "C" int vcv_rel_attn_stream_fwd(const float* q, const float* k, const float* v, const float* embk, const float* embv,
                                       const float* mask, float* out, int B, int H, int dk, int T, int w, float qscale,
                                       void* stream) {
  if (!q || !k || !v || !embk || !embv || !mask || !out || vcv_rel_attn_stream_supported(B, H, dk, T, w) != 0) return VCV_EINVAL;
  const dim3 grid(vcv_cdiv(T, 128), B * H);
  if (dk == 64)
    rel_attn_stream_fwd_kernel<64><<<grid, 256, 0, (hipStream_t)stream>>>(q, k, v, embk, embv, mask, out, H, T, w, qscale);
  else
    rel_attn_stream_fwd_kernel<32><<<grid, 256, 0, (hipStream_t)stream>>>(q, k, v, embk, embv, mask, out, H, T, w, qscale);
  return vcv_check_launch();
}
