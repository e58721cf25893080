// attention_stream_bf16.hip -- the two streamed-softmax attention kernels with bf16 OPERANDS on v_mfma_f32_32x32x16_bf16:
// rel_attn_stream_fwd_bf16_kernel (the twin of attention_stream.hip's kernel) and hubert_attn_fwd_bf16_kernel (the twin of
// hubert.hip's).  What bf16 compute mode runs when VCVITS_ATTN_STREAM_BF16 = 1; the fp32 kernels are untouched.
//
// The frame is attn_stream_tile.h: tile_softmax_step and tile_store as they are, and the *_bf16 functions for staging, the
// scores and P V.  K, V and Q are rounded to bf16 (nearest even) on the way in, Q unscaled; the scale multiplies the fp32
// score.  The probabilities are rounded to bf16 only as the operand of the second product: the row sum l is formed from
// the fp32 values.  Everything that is a kernel's own stays fp32 arithmetic on unrounded values:
//   * rel-pos: rel[r] = qscale * (q_i . embk[r]) from the fp32 q before it is packed, the -1e4 fill by select, -inf behind
//     T, the band probabilities Pb with their three carries, out += sum pb * carry * embv, __expf;
//   * HuBERT: expf, keys s < frames[b] only with LEN, exact 0 behind; D = 80 is 5 score steps and 3 output tiles whose
//     channels >= 80 are zero rows of the value tile and are never stored.
// Grid (ceil(T / 128), B * H), 256 threads, every index that scales with T size_t, as the fp32 kernels.
//
// Resources (hipcc -O3, gfx950, from the code object's metadata; tests/test_attention_stream_bf16_cpu.py holds them):
//   rel-pos dk = 32: 156 registers, 27,520 B LDS (fp32 twin: 168, 30,976);   dk = 64: 212 registers, 35,968 B LDS (244, 43,392);
//   HuBERT  dk = 64: 156 registers,  9,216 B LDS (fp32 twin: 192, 16,640);   dk = 80: 204 registers, 12,544 B LDS (248, 22,912),
//   with and without lengths alike;
// 0 B scratch and no spills in all six instances.  The occupancy classes are those of the fp32 twins: three workgroups per
// CU for rel-pos dk = 32 (<= 168 registers), two for the others (169 .. 256), HuBERT dk = 64 now three as well.
#include "attn_stream_tile.h"

namespace {

constexpr int RELS = 16;  // relative positions at most (2w + 1 <= 16, as attention_stream.hip)
constexpr int RS = 18;    // row stride of the two band tables (attention_stream.hip)

template <int D>
__global__ void __launch_bounds__(256)
rel_attn_stream_fwd_bf16_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                const float* __restrict__ embk, const float* __restrict__ embv, const float* __restrict__ mask,
                                float* __restrict__ out, int H, int T, int w, float qscale) {
  constexpr int DT = D / 32;  // output tiles of 32 channels
  __shared__ __attribute__((aligned(16))) __bf16 Ks[32 * tile_ks(D)];
  __shared__ __attribute__((aligned(16))) __bf16 Vs[D * TILE_VSB];
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

  bf16x8 qb[D / 16];
  const float mi = tok ? mask[mbase + t] : 0.f;
  for (int i = tid; i < RELS * D; i += 256) {
    Ek[i] = i < nr * D ? embk[i] : 0.f;
    Ev[i] = i < nr * D ? embv[i] : 0.f;
  }
  for (int i = tid; i < 128 * RS; i += 256) Pb[i] = 0.f;
  __syncthreads();
  {
    // rel[r] = qscale * (q_i . embk[r]) from the fp32 q: each lane sums its channels, the two halves meet through lane ^ 32
    float qf[D / 2];
    tile_load_q_bf16<D>(qf, q, base, T, t, hf, tok);
    for (int r = 0; r < nr; ++r) {
      float a = 0.f;
#pragma unroll
      for (int i = 0; i < D / 2; ++i) a += qf[i] * Ek[r * D + 16 * (i >> 3) + 8 * hf + (i & 7)];
      a += __shfl_xor(a, 32);
      if (hf == 0) Rl[row + r] = a * qscale;
    }
    tile_pack_q_bf16<D>(qb, qf);
  }

  f32x16 o[DT] = {};
  float m = -INFINITY, l = 0.f;
  float c0 = 0.f, c1 = 0.f, c2 = 0.f;  // rescale carried by the band entries of the tiles at t0 - 32, t0, t0 + 32

  for (int s0 = 0; s0 < T; s0 += 32) {
    __syncthreads();  // the previous tile has been read (first pass: Rl is written)
    tile_stage_kv_bf16<D>(Ks, Vs, k, v, base, T, s0, T, tid);
    if (tid < 32) Ms[tid] = s0 + tid < T ? mask[mbase + s0 + tid] : 0.f;
    __syncthreads();
    f32x16 S = tile_scores_bf16<D>(Ks, qb, qscale, col, hf);

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
    tile_pv_bf16(o, Vs, S, alpha, col, hf);
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

// the bf16-operand twin of hubert_attn_fwd_kernel (hubert.hip): same arguments, same LEN semantics
template <int D, bool LEN>
__global__ void __launch_bounds__(256)
hubert_attn_fwd_bf16_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                            float* __restrict__ out, int H, int T, size_t ldb, float scale, const int* __restrict__ frames) {
  constexpr int DT = (D + 31) / 32;  // output tiles of 32 channels
  __shared__ __attribute__((aligned(16))) __bf16 Ks[32 * tile_ks(D)];
  __shared__ __attribute__((aligned(16))) __bf16 Vs[DT * 32 * TILE_VSB];
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

  bf16x8 qb[D / 16];
  {
    float qf[D / 2];
    tile_load_q_bf16<D>(qf, q, base, T, t, hf, qok);
    tile_pack_q_bf16<D>(qb, qf);
  }
  for (int i = D * TILE_VSB + tid; i < DT * 32 * TILE_VSB; i += 256) Vs[i] = (__bf16)0.f;
  f32x16 o[DT] = {};
  float m = -INFINITY, l = 0.f;

  for (int s0 = 0; s0 < n; s0 += 32) {
    __syncthreads();  // the previous tile has been read
    tile_stage_kv_bf16<D>(Ks, Vs, k, v, base, T, s0, n, tid);
    __syncthreads();
    f32x16 S = tile_scores_bf16<D>(Ks, qb, scale, col, hf);
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if (s0 + acc_row(r, hf) >= n) S[r] = -INFINITY;
    const float alpha = tile_softmax_step<false>(S, m, l);
    tile_pv_bf16(o, Vs, S, alpha, col, hf);
  }

  if (tok) tile_store<D>(out, obase, T, t, o, l, hf, !LEN || qok);
}

// frames: null launches the kernel without lengths
int hubert_bf16_launch(const float* q, const float* k, const float* v, float* out, int B, int H, int dk, int T, int64_t ldb,
                       float scale, const int* frames, void* stream) {
  if (!q || !k || !v || !out || vcv_hubert_attn_supported(B, H, dk, T) != 0 || ldb < (int64_t)H * dk * T) return VCV_EINVAL;
  const auto kernel = dk == 64 ? (frames ? hubert_attn_fwd_bf16_kernel<64, true> : hubert_attn_fwd_bf16_kernel<64, false>)
                               : (frames ? hubert_attn_fwd_bf16_kernel<80, true> : hubert_attn_fwd_bf16_kernel<80, false>);
  kernel<<<dim3(vcv_cdiv(T, 128), B * H), 256, 0, (hipStream_t)stream>>>(q, k, v, out, H, T, (size_t)ldb, scale, frames);
  return vcv_check_launch();
}

}  // namespace

// vcv_rel_attn_stream_fwd with bf16 operands: the same arguments, shapes (vcv_rel_attn_stream_supported) and refusals
extern "C" int vcv_rel_attn_stream_fwd_bf16(const float* q, const float* k, const float* v, const float* embk,
                                            const float* embv, const float* mask, float* out, int B, int H, int dk, int T, int w,
                                            float qscale, void* stream) {
  if (!q || !k || !v || !embk || !embv || !mask || !out || vcv_rel_attn_stream_supported(B, H, dk, T, w) != 0) return VCV_EINVAL;
  const dim3 grid(vcv_cdiv(T, 128), B * H);
  if (dk == 64)
    rel_attn_stream_fwd_bf16_kernel<64><<<grid, 256, 0, (hipStream_t)stream>>>(q, k, v, embk, embv, mask, out, H, T, w, qscale);
  else
    rel_attn_stream_fwd_bf16_kernel<32><<<grid, 256, 0, (hipStream_t)stream>>>(q, k, v, embk, embv, mask, out, H, T, w, qscale);
  return vcv_check_launch();
}

// vcv_hubert_attn_fwd / vcv_hubert_attn_fwd_len with bf16 operands: the same arguments, shapes (vcv_hubert_attn_supported)
// and refusals
extern "C" int vcv_hubert_attn_fwd_bf16(const float* q, const float* k, const float* v, float* out, int B, int H, int dk, int T,
                                        int64_t ldb, float scale, void* stream) {
  return hubert_bf16_launch(q, k, v, out, B, H, dk, T, ldb, scale, nullptr, stream);
}

extern "C" int vcv_hubert_attn_fwd_len_bf16(const float* q, const float* k, const float* v, float* out, int B, int H, int dk,
                                            int T, int64_t ldb, float scale, const int* frames, void* stream) {
  return frames ? hubert_bf16_launch(q, k, v, out, B, H, dk, T, ldb, scale, frames, stream) : VCV_EINVAL;
}
