// attention_stream.hip -- relative-position self-attention of the content encoder with the keys and values STREAMED
// (vits/model/transformer/relative_attention_transformer.py:150-182), forward only, no dropout, no probability output:
// what long-form inference runs.  Nothing of size T x T exists, so memory is linear in T and T is not bounded by LDS.
//
// The frame -- block, tiles of 32 keys, the two MFMA contractions, which key a lane's register holds -- is the one of
// attn_stream_tile.h, shared with hubert_attn_fwd_kernel (hubert.hip).  The kernel is rel_attn_stream_fwd_body of
// attn_stream_fwd.h with fp32 operands (TileF32) and no hook; the bf16-operand kernel (attention_stream_bf16.hip) and the
// training forward (attention_stream_grad.hip) are the same body.  What that body adds to the frame, following
// tests/attention_f64.py points 1, 2, 4, with __expf:
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
#include "attn_stream_fwd.h"

namespace {

template <int D>
__global__ void __launch_bounds__(256)
rel_attn_stream_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                           const float* __restrict__ embk, const float* __restrict__ embv, const float* __restrict__ mask,
                           float* __restrict__ out, int H, int T, int w, float qscale) {
  rel_attn_stream_fwd_body<TileF32<D>>(q, k, v, embk, embv, mask, out, H, T, w, qscale, NoHook());
}

struct RelFwdF32 {
  template <int D>
  static auto kernel() { return rel_attn_stream_fwd_kernel<D>; }
};

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
  return rel_attn_stream_launch<RelFwdF32>(q, k, v, embk, embv, mask, out, B, H, dk, T, w, qscale, stream);
}
