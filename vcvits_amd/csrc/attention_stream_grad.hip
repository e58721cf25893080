// attention_stream_grad.hip -- TRAINING through the streamed relative-position self-attention of the content encoder
// (vits/model/transformer/relative_attention_transformer.py:150-182 and its autograd): a forward with dropout that leaves
// two floats per query behind, and a backward pass that recomputes the probabilities from them tile by tile.  Nothing of
// size T x T exists in either direction, so the memory of a training step is linear in T.
//
// The frame is the one of attn_stream_tile.h (block = one head x 128 lanes-as-columns, tiles of 32 rows through LDS, both
// contractions on v_mfma_f32_32x32x2_f32, __expf); the maths is tests/attention_f64.py points 1-5.
//
//   rel_attn_stream_train_fwd_kernel<D>  the streamed forward of attention_stream.hip -- the same body,
//   rel_attn_stream_fwd_body of attn_stream_fwd.h, not a copy of it -- with TrainHook (below) for
//     * dropout: the running sum l takes exp(s - m) as it is, the value product and the band entries take it times
//       drop_scale(seed, (g*T + i)*T + j): the generator and the flat index of attention.hip, so the fused kernels, the
//       unfused path and tests/attention_f64.keep_mask all draw the same mask.  p = 0 is one uniform branch;
//     * stats [B*H, T, 2] = (final running max m_i, final sum l_i).  The PAIR, not m + log l: a masked query row has every
//       score at -1e4, and -1e4 + log T has an ulp of 1e-3 in fp32, while exp(s - m) / l is exact there (m = -1e4, l = T).
//
//   The backward pass is TWO passes with one writer per output element: no float atomics, no workgroup waiting on another,
//   so all five gradients are bit-reproducible in every mode.  It costs two more score-type products than the single-pass
//   form (14 G T^2 dk FLOP instead of 10).  Both passes recompute, per (query i, key j):
//       P   = exp(s - m_i) / l_i          s: the filled score (band term added, -1e4 by select where mask_i * mask_j == 0)
//       dPd = dO_i . v_j + [band] dO_i . embv[j - i + w]
//       dS  = P (c dPd - delta_i)         c: the dropout factor, delta_i = sum_d dO[d,i] out[d,i] (= sum_j dPd Pd)
//     and dS is exactly 0 where the score was filled (the fill passes no gradient).
//
//   rel_attn_stream_bwd_q_kernel<D>   lane = query, K / V tiles of 32 keys streamed.  dq_i = qscale (sum_j dS_ij k_j +
//     sum_r dS_{i,i+r-w} embk[r]), the first sum on the matrix cores with the dS accumulator as B operand.  The band entries
//     of dS and Pd are kept per query in LDS ([128][RS], each written once by the lane that holds that key); from them the
//     block forms its partial tables dembk_part[r] = qscale sum_i dS_{i,i+r-w} q_i and dembv_part[r] = sum_i Pd_{i,i+r-w} dO_i.
//     To the workspace: delta, the band dot products q_i . embk[r] and dO_i . embv[r] (the key pass needs them for the
//     queries of a tile), and the partial tables, one slot per (head, query block).
//   rel_attn_stream_bwd_kv_kernel<D>  the mirror image: lane = key, tiles of 32 queries streamed (q pre-scaled, dO, and
//     per query m, 1 / l, delta, mask).  dv_j = sum_i Pd_ij dO_i and dk_j = qscale sum_i dS_ij q_i stay in the wave's
//     accumulators for the whole launch.  Only the three query tiles that meet the wave's band read the band terms.
//   rel_attn_stream_demb_reduce_kernel  dembk / dembv = the partial tables summed in index order.
//
// Workspace (floats): delta [G*T] | q.embk [G*T*(2w+1)] | dO.embv [G*T*(2w+1)] | partial tables [G*ceil(T/128)*2*(2w+1)*dk].
// Every index that scales with T is size_t.  Grids (ceil(T / 128), B * H), 256 threads.
//
// Resources (hipcc -O3, gfx950, from the code object's metadata; tests/test_attention_stream_grad_cpu.py reads them):
//   kernel, dk            registers (vector + accumulation, unified)   SGPR   static LDS
//   train_fwd  32 / 64    220 / 288                                    100    30,976 / 43,392 B
//   bwd_q      32 / 64    216 / 291                                    88/89  49,536 / 62,080 B
//   bwd_kv     32 / 64    276 / 348                                    52     8,960 / 17,408 B
//   demb_reduce           12                                           20     4,160 B
// 0 B scratch and no spills in any of them.  Past 256 registers a SIMD holds one wave, i.e. one workgroup per CU: these
// kernels were written for memory, and their occupancy has not been worked on (profiles/attn_stream_grad_bench.txt).
// What keeps the scalar registers from spilling, and is easy to undo by accident: 16 selects in a row hold 16 lane masks
// (32 scalar registers) between the compares and their uses.  So the dropout factor is applied as a bit mask and not as a
// select (drop_mix), and the query pass does not test `key < T` per element (see there).
#include "attn_stream_fwd.h"

namespace {

constexpr int LS = 33;    // row stride of a tile that is read both along and across its rows

// The dropout mask of attention.hip / vits_blocks.hip: same stream, same masks.  There the factor of element idx is
// drop_scale(seed, idx): splitmix64 of z = seed + idx * DROP_STEP (mod 2^64), 24 bits of it against p.  Here the kernels walk
// the 16 elements of an accumulator by ADDING to z (the next key is + DROP_STEP, the next query + T * DROP_STEP): one 64-bit
// index multiply per tile instead of one per element, and no table of 16 64-bit constants in scalar registers.
constexpr unsigned long long DROP_STEP = 0x9E3779B97F4A7C15ull;
// keep iff u = (z >> 40) * 2^-24 >= p, i.e. (z >> 40) >= thr = ceil(p * 2^24) (both sides of that are exact: u has 24 bits and
// p * 2^24 is p with another exponent).  Compared as integers and applied as a bit mask, so that 16 of these in a row
// hold no 16 lane masks in scalar registers.
__device__ __forceinline__ float drop_mix(unsigned long long z, int thr, float inv_keep) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  const int below = ((int)(z >> 40) - thr) >> 31;  // all ones where dropped
  return __int_as_float(__float_as_int(inv_keep) & ~below);
}
// c[r] = the factor of the element at flat index idx0 + acc_row(r, 0) * stride, r = 0 .. 15 (idx0 holds the lane half's
// 4 * hf * stride)
__device__ __forceinline__ void drop_tile(float (&c)[16], unsigned long long seed, unsigned long long idx0, unsigned long long stride,
                                          float p, float inv_keep) {
  unsigned long long z = seed + idx0 * DROP_STEP;
  const unsigned long long dz = stride * DROP_STEP;
  const int thr = (int)ceilf(p * 16777216.0f);
#pragma unroll
  for (int g = 0; g < 4; ++g) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      c[4 * g + e] = drop_mix(z, thr, inv_keep);
      z += dz;
    }
    z += 4 * dz;  // rows 8 g + 4 .. 8 g + 7 are the other lane half's
  }
}

// columns c0 .. c0 + 31 of the heads a and b at `base` into As / Bs as [d][LS], scaled; columns at or past T are 0 by a
// select and never read.  The caller puts the block's barriers around it.
template <int D>
__device__ __forceinline__ void stage_pair(float* As, float* Bs, const float* __restrict__ a, const float* __restrict__ b,
                                           size_t base, int T, int c0, int tid, float sa) {
  const int sd = tid >> 5, sc = tid & 31;
  const int c = c0 + sc;
  const bool ok = c < T;
#pragma unroll
  for (int i = 0; i < D / 8; ++i) {
    const int d = sd + 8 * i;
    const size_t g = base + (size_t)d * T + (ok ? c : 0);
    As[d * LS + sc] = ok ? a[g] * sa : 0.f;
    Bs[d * LS + sc] = ok ? b[g] : 0.f;
  }
}

// C[row][lane's column] = sum_d X[d][row] xr[d]: X a [d][LS] tile, xr the lane's column (element 2i + hf in xr[i])
template <int D>
__device__ __forceinline__ f32x16 dot_tile(const float* Xs, const float (&xr)[D / 2], int col, int hf) {
  f32x16 S = {};
#pragma unroll
  for (int i = 0; i < D / 2; ++i) S = __builtin_amdgcn_mfma_f32_32x32x2f32(Xs[(2 * i + hf) * LS + col], xr[i], S, 0, 0, 0);
  return S;
}

// o[d][lane's column] += sum_row X[d][row] W[row][lane's column]: X a [d][LS] tile, W a dot_tile result
template <int DT>
__device__ __forceinline__ void acc_tile(f32x16 (&o)[DT], const float* Xs, const f32x16& W, int col, int hf) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int sr = acc_row(r, hf);
#pragma unroll
    for (int j = 0; j < DT; ++j)
      o[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(Xs[(j * 32 + col) * LS + sr], W[r], o[j], 0, 0, 0);
  }
}

// The training forward's two additions to rel_attn_stream_fwd_body (attn_stream_fwd.h): dropout on the probabilities of a
// tile -- the row sum l has taken exp(s - m) as it is, the band entries and the value product take it dropped -- and the
// stats pair of a query at the end.  p = 0 is one uniform branch, and then the bits are the plain streamed forward's.
struct TrainHook {
  float* __restrict__ stats;
  int T;
  float pdrop, inv_keep;
  unsigned long long seed;
  __device__ __forceinline__ void tile(f32x16& S, int s0, int i, int hf) const {
    if (pdrop > 0.f) {
      const size_t drow = ((size_t)blockIdx.y * T + i) * T;  // flat index of this query's first probability
      float c[16];
      drop_tile(c, seed, drow + (size_t)(s0 + 4 * hf), 1ull, pdrop, inv_keep);
#pragma unroll
      for (int r = 0; r < 16; ++r) S[r] *= c[r];
    }
  }
  __device__ __forceinline__ void done(int t, int hf, float m, float l) const {
    if (hf == 0) {
      const size_t si = ((size_t)blockIdx.y * T + t) * 2;
      stats[si] = m;
      stats[si + 1] = l;
    }
  }
};

template <int D>
__global__ void __launch_bounds__(256)
rel_attn_stream_train_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                 const float* __restrict__ embk, const float* __restrict__ embv, const float* __restrict__ mask,
                                 float* __restrict__ out, float* __restrict__ stats, int H, int T, int w, float qscale,
                                 float pdrop, unsigned long long seed, const unsigned long long* __restrict__ seed_off) {
  if (seed_off) seed += *seed_off;
  rel_attn_stream_fwd_body<TileF32<D>>(q, k, v, embk, embv, mask, out, H, T, w, qscale,
                                       TrainHook{stats, T, pdrop, 1.f / (1.f - pdrop), seed});
}

// Query pass.
template <int D>
__global__ void __launch_bounds__(256)
rel_attn_stream_bwd_q_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                             const float* __restrict__ embk, const float* __restrict__ embv, const float* __restrict__ mask,
                             const float* __restrict__ out, const float* __restrict__ stats, const float* __restrict__ dO,
                             float* __restrict__ ws, float* __restrict__ dq, int H, int T, int w, float qscale,
                             float pdrop, unsigned long long seed, const unsigned long long* __restrict__ seed_off) {
  constexpr int DT = D / 32;
  constexpr int NE = RELS * D / 256;  // table elements per thread
  __shared__ float Ks[D * LS];
  __shared__ float Vs[D * LS];
  __shared__ __attribute__((aligned(16))) float Ms[32];
  __shared__ float Ek[RELS * D];
  __shared__ float Ev[RELS * D];
  __shared__ float Rk[128 * RS];   // q_i . embk[r] (q pre-scaled)
  __shared__ float Rv[128 * RS];   // dO_i . embv[r]
  __shared__ float dSb[128 * RS];  // dS_{i, i + r - w}
  __shared__ float Pdb[128 * RS];  // Pd_{i, i + r - w}
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int col = lane & 31, hf = lane >> 5;
  const int nr = 2 * w + 1;
  const size_t gT = (size_t)blockIdx.y * T;
  const size_t base = gT * D;
  const size_t mbase = (size_t)(blockIdx.y / H) * T;
  const int t0 = blockIdx.x * 128 + wv * 32;
  const int t = t0 + col;
  const bool tok = t < T;
  const int row = (wv * 32 + col) * RS;
  const float inv_keep = 1.f / (1.f - pdrop);
  if (seed_off) seed += *seed_off;
  const size_t drow = (gT + (tok ? t : 0)) * T;
  const size_t GT = (size_t)gridDim.y * T;  // the workspace sections (file header) start at multiples of it
  float* const ws_delta = ws;
  float* const ws_rk = ws + GT;
  float* const ws_rv = ws + GT * (1 + nr);

  float qr[D / 2], dor[D / 2];
  tile_load_q<D>(qr, q, base, T, t, hf, qscale, tok);
  tile_load_q<D>(dor, dO, base, T, t, hf, 1.f, tok);
  const float mi = tok ? mask[mbase + t] : 0.f;
  const float mrow = tok ? stats[(gT + t) * 2] : 0.f;
  const float invl = tok ? 1.f / stats[(gT + t) * 2 + 1] : 0.f;  // a query that does not exist has P = 0
  float delta = 0.f;
  if (tok) {
#pragma unroll
    for (int i = 0; i < D / 2; ++i) delta += dor[i] * out[base + (size_t)(2 * i + hf) * T + t];
  }
  delta += __shfl_xor(delta, 32);
  if (tok && hf == 0) ws_delta[gT + t] = delta;

  for (int i = tid; i < RELS * D; i += 256) {
    Ek[i] = i < nr * D ? embk[i] : 0.f;
    Ev[i] = i < nr * D ? embv[i] : 0.f;
  }
  for (int i = tid; i < 128 * RS; i += 256) dSb[i] = 0.f, Pdb[i] = 0.f;
  __syncthreads();
  for (int r = 0; r < nr; ++r) {
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int i = 0; i < D / 2; ++i) {
      a += qr[i] * Ek[r * D + 2 * i + hf];
      b += dor[i] * Ev[r * D + 2 * i + hf];
    }
    a += __shfl_xor(a, 32);
    b += __shfl_xor(b, 32);
    if (hf == 0) {
      Rk[row + r] = a;
      Rv[row + r] = b;
      if (tok) {
        ws_rk[(gT + t) * nr + r] = a;
        ws_rv[(gT + t) * nr + r] = b;
      }
    }
  }

  f32x16 o[DT] = {};
  for (int s0 = 0; s0 < T; s0 += 32) {
    __syncthreads();  // the previous tile has been read (first pass: Rk / Rv are written)
    stage_pair<D>(Ks, Vs, k, v, base, T, s0, tid, 1.f);
    if (tid < 32) Ms[tid] = s0 + tid < T ? mask[mbase + s0 + tid] : 0.f;
    __syncthreads();
    f32x16 S = dot_tile<D>(Ks, qr, col, hf);
    f32x16 dP = dot_tile<D>(Vs, dor, col, hf);

    const int ds = s0 - t0;
    const bool band = ds >= -32 && ds <= 32;  // wave-uniform
    if (band) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int off = ds + acc_row(r, hf) - col + w;  // key - query + w
        const bool inb = off >= 0 && off < nr;
        const float rk = Rk[row + (inb ? off : 0)], rv = Rv[row + (inb ? off : 0)];
        S[r] += inb ? rk : 0.f;
        dP[r] += inb ? rv : 0.f;
      }
    }
    float c[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) c[r] = 1.f;
    if (pdrop > 0.f) drop_tile(c, seed, drow + (size_t)(s0 + 4 * hf), 1ull, pdrop, inv_keep);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int sr = acc_row(r, hf);
      const bool fill = mi * Ms[sr] == 0.f;
      const float p = __expf((fill ? -1e4f : S[r]) - mrow) * invl;
      S[r] = p * c[r];
      dP[r] = fill ? 0.f : p * (c[r] * dP[r] - delta);
    }
    // (a key at or past T is staged as masked, so its dS is 0; its Pd is not, for a masked query, and is never used: the
    // band entries below are written for existing keys only)
    if (band) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int sr = acc_row(r, hf);
        const int off = ds + sr - col + w;
        if (off >= 0 && off < nr && s0 + sr < T) {
          Pdb[row + off] = S[r];
          dSb[row + off] = dP[r];
        }
      }
    }
    acc_tile(o, Ks, dP, col, hf);
  }
  __syncthreads();  // both lanes of a query read the band entries either of them wrote

  if (tok) {
    for (int r = 0; r < nr; ++r) {
      const float d = dSb[row + r];
#pragma unroll
      for (int j = 0; j < DT; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[j][e] += d * Ek[r * D + j * 32 + acc_row(e, hf)];
    }
#pragma unroll
    for (int j = 0; j < DT; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) dq[base + (size_t)(j * 32 + acc_row(e, hf)) * T + t] = o[j][e] * qscale;
  }

  // the block's partial tables: its 128 queries go through Ks (q) / Vs (dO) 32 at a time; thread -> NE (r, d) elements
  float ak[NE] = {}, av[NE] = {};
  for (int ch = 0; ch < 4; ++ch) {
    __syncthreads();
    stage_pair<D>(Ks, Vs, q, dO, base, T, blockIdx.x * 128 + ch * 32, tid, 1.f);
    __syncthreads();
#pragma unroll
    for (int n = 0; n < NE; ++n) {
      const int e = tid + 256 * n, d = e % D, r = e / D;
      for (int i = 0; i < 32; ++i) {
        ak[n] += dSb[(ch * 32 + i) * RS + r] * Ks[d * LS + i];
        av[n] += Pdb[(ch * 32 + i) * RS + r] * Vs[d * LS + i];
      }
    }
  }
  const size_t ne = (size_t)nr * D;
  float* part = ws + GT * (1 + 2 * nr) + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2 * ne;
#pragma unroll
  for (int n = 0; n < NE; ++n) {
    const int e = tid + 256 * n;
    if (e < nr * D) {
      part[e] = ak[n] * qscale;
      part[ne + e] = av[n];
    }
  }
}

// Key pass.
template <int D>
__global__ void __launch_bounds__(256)
rel_attn_stream_bwd_kv_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                              const float* __restrict__ mask, const float* __restrict__ stats, const float* __restrict__ dO,
                              const float* __restrict__ ws_delta, const float* __restrict__ ws_rk,
                              const float* __restrict__ ws_rv, float* __restrict__ dk_, float* __restrict__ dv, int H, int T,
                              int w, float qscale, float pdrop, unsigned long long seed,
                              const unsigned long long* __restrict__ seed_off) {
  constexpr int DT = D / 32;
  __shared__ float Qs[D * LS];  // q * qscale
  __shared__ float Os[D * LS];  // dO
  __shared__ float Mx[32], Il[32], Dl[32], Mq[32];  // of the tile's queries: running max, 1 / sum, delta, mask
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int col = lane & 31, hf = lane >> 5;
  const int nr = 2 * w + 1;
  const size_t gT = (size_t)blockIdx.y * T;
  const size_t base = gT * D;
  const size_t mbase = (size_t)(blockIdx.y / H) * T;
  const int j0 = blockIdx.x * 128 + wv * 32;  // first key of the wave
  const int j = j0 + col;
  const bool jok = j < T;
  const float inv_keep = 1.f / (1.f - pdrop);
  if (seed_off) seed += *seed_off;

  float kr[D / 2], vr[D / 2];
  tile_load_q<D>(kr, k, base, T, j, hf, 1.f, jok);
  tile_load_q<D>(vr, v, base, T, j, hf, 1.f, jok);
  const float mj = jok ? mask[mbase + j] : 0.f;

  f32x16 ak[DT] = {}, av[DT] = {};
  for (int i0 = 0; i0 < T; i0 += 32) {
    __syncthreads();  // the previous tile has been read
    stage_pair<D>(Qs, Os, q, dO, base, T, i0, tid, qscale);
    if (tid < 32) {
      const int i = i0 + tid;
      const bool ok = i < T;
      Mx[tid] = ok ? stats[(gT + i) * 2] : 0.f;
      Il[tid] = ok ? 1.f / stats[(gT + i) * 2 + 1] : 0.f;  // a query that does not exist has P = 0
      Dl[tid] = ok ? ws_delta[gT + i] : 0.f;
      Mq[tid] = ok ? mask[mbase + i] : 0.f;
    }
    __syncthreads();
    f32x16 S = dot_tile<D>(Qs, kr, col, hf);
    f32x16 dP = dot_tile<D>(Os, vr, col, hf);

    const int ds = i0 - j0;
    if (ds >= -32 && ds <= 32) {  // wave-uniform: the band of the wave's keys meets this query tile
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = i0 + acc_row(r, hf);
        const int off = j - i + w;  // key - query + w
        if (off >= 0 && off < nr && i < T) {
          S[r] += ws_rk[(gT + i) * nr + off];
          dP[r] += ws_rv[(gT + i) * nr + off];
        }
      }
    }
    float c[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) c[r] = 1.f;
    if (pdrop > 0.f) drop_tile(c, seed, (gT + (size_t)(i0 + 4 * hf)) * T + j, (unsigned long long)T, pdrop, inv_keep);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int sr = acc_row(r, hf);
      const bool fill = Mq[sr] * mj == 0.f;
      const float p = __expf((fill ? -1e4f : S[r]) - Mx[sr]) * Il[sr];
      S[r] = p * c[r];
      dP[r] = fill ? 0.f : p * (c[r] * dP[r] - Dl[sr]);
    }
    acc_tile(av, Os, S, col, hf);
    acc_tile(ak, Qs, dP, col, hf);
  }
  if (!jok) return;
#pragma unroll
  for (int jt = 0; jt < DT; ++jt)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const size_t o = base + (size_t)(jt * 32 + acc_row(e, hf)) * T + j;
      dv[o] = av[jt][e];
      dk_[o] = ak[jt][e];  // (Qs holds q * qscale)
    }
}

// dembk / dembv [ne] = sum over the npart partial tables ([dembk | dembv], 2 * ne floats each), in index order.  Block = 64
// table elements x 16 slices of the partial range; the slices meet in LDS (rel_attn_demb_reduce_kernel, attention.hip).
__global__ void __launch_bounds__(1024) rel_attn_stream_demb_reduce_kernel(const float* __restrict__ part, float* __restrict__ dembk,
                                                                          float* __restrict__ dembv, int npart, int ne) {
  __shared__ float red[16][65];
  const int x = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const int el = blockIdx.x * 64 + x;
  float a = 0.f;
  if (el < 2 * ne) {
    const int per = (npart + 15) / 16;
    const int p0 = sl * per, p1 = p0 + per < npart ? p0 + per : npart;
    for (int p = p0; p < p1; ++p) a += part[(size_t)p * 2 * ne + el];
  }
  red[sl][x] = a;
  __syncthreads();
  if (sl == 0 && el < 2 * ne) {
    float t = red[0][x];
#pragma unroll
    for (int s = 1; s < 16; ++s) t += red[s][x];
    if (el < ne) dembk[el] = t; else dembv[el - ne] = t;
  }
}

bool ok_call(int B, int H, int dk, int T, int w, float pdrop) {
  return vcv_rel_attn_stream_supported(B, H, dk, T, w) == 0 && pdrop >= 0.f && pdrop < 1.f &&
         (long long)B * H * vcv_cdiv(T, 128) <= 0x7fffffffLL;  // (the reduce kernel counts the partial tables in an int)
}

}  // namespace

// out [B, H*dk, T] and stats [B*H, T, 2] = (running max, sum) of the attention with dropout (pdrop, seed)
extern "C" int vcv_rel_attn_stream_train_fwd(const float* q, const float* k, const float* v, const float* embk, const float* embv,
                                             const float* mask, float* out, float* stats, int B, int H, int dk, int T, int w,
                                             float qscale, float pdrop, uint64_t seed, void* stream) {
  if (!q || !k || !v || !embk || !embv || !mask || !out || !stats || !ok_call(B, H, dk, T, w, pdrop)) return VCV_EINVAL;
  const unsigned long long* so = (const unsigned long long*)vcv_get_seed_offset_ptr();
  const dim3 grid(vcv_cdiv(T, 128), B * H);
  if (dk == 64)
    rel_attn_stream_train_fwd_kernel<64><<<grid, 256, 0, (hipStream_t)stream>>>(q, k, v, embk, embv, mask, out, stats, H, T, w,
                                                                                  qscale, pdrop, seed, so);
  else
    rel_attn_stream_train_fwd_kernel<32><<<grid, 256, 0, (hipStream_t)stream>>>(q, k, v, embk, embv, mask, out, stats, H, T, w,
                                                                                  qscale, pdrop, seed, so);
  return vcv_check_launch();
}

// floats of workspace the backward pass needs (linear in T); < 0 for a shape it does not take
extern "C" long long vcv_rel_attn_stream_bwd_workspace(int B, int H, int dk, int T, int w) {
  if (vcv_rel_attn_stream_supported(B, H, dk, T, w) != 0) return -1;
  const long long G = (long long)B * H, nr = 2 * w + 1;
  return G * T * (1 + 2 * nr) + G * vcv_cdiv(T, 128) * 2 * nr * dk;
}

extern "C" int vcv_rel_attn_stream_bwd(const float* q, const float* k, const float* v, const float* embk, const float* embv,
                                       const float* mask, const float* out, const float* stats, const float* dO, float* ws,
                                       float* dq, float* dk_out, float* dv, float* dembk, float* dembv, int B, int H, int dk, int T,
                                       int w, float qscale, float pdrop, uint64_t seed, void* stream) {
  if (!q || !k || !v || !embk || !embv || !mask || !out || !stats || !dO || !ws || !dq || !dk_out || !dv || !dembk || !dembv ||
      !ok_call(B, H, dk, T, w, pdrop))
    return VCV_EINVAL;
  const unsigned long long* so = (const unsigned long long*)vcv_get_seed_offset_ptr();  // the same offset as the forward
  const hipStream_t st = (hipStream_t)stream;
  const size_t GT = (size_t)B * H * T;
  const int nr = 2 * w + 1, nqb = vcv_cdiv(T, 128);
  float *ws_delta = ws, *ws_rk = ws + GT, *ws_rv = ws_rk + GT * nr, *ws_part = ws_rv + GT * nr;
  const dim3 grid(nqb, B * H);
  if (dk == 64) {
    rel_attn_stream_bwd_q_kernel<64><<<grid, 256, 0, st>>>(q, k, v, embk, embv, mask, out, stats, dO, ws, dq, H, T, w, qscale, pdrop, seed, so);
    rel_attn_stream_bwd_kv_kernel<64><<<grid, 256, 0, st>>>(q, k, v, mask, stats, dO, ws_delta, ws_rk, ws_rv, dk_out, dv, H, T, w,
                                                            qscale, pdrop, seed, so);
  } else {
    rel_attn_stream_bwd_q_kernel<32><<<grid, 256, 0, st>>>(q, k, v, embk, embv, mask, out, stats, dO, ws, dq, H, T, w, qscale, pdrop, seed, so);
    rel_attn_stream_bwd_kv_kernel<32><<<grid, 256, 0, st>>>(q, k, v, mask, stats, dO, ws_delta, ws_rk, ws_rv, dk_out, dv, H, T, w,
                                                            qscale, pdrop, seed, so);
  }
  const int ne = nr * dk;
  rel_attn_stream_demb_reduce_kernel<<<vcv_cdiv(2 * ne, 64), 1024, 0, st>>>(ws_part, dembk, dembv, B * H * nqb, ne);
  return vcv_check_launch();
}
