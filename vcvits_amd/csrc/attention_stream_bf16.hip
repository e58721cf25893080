// attention_stream_bf16.hip -- the two streamed-softmax attention kernels with bf16 OPERANDS on v_mfma_f32_32x32x16_bf16:
// rel_attn_stream_fwd_bf16_kernel (the twin of attention_stream.hip's kernel) and hubert_attn_fwd_bf16_kernel (the twin of
// hubert.hip's).  What bf16 compute mode runs when VCVITS_ATTN_STREAM_BF16 = 1; the fp32 kernels are untouched.
//
// Both are the bodies of attn_stream_fwd.h, the ones the fp32 kernels call, instantiated with the operand policy TileBF16 of
// attn_stream_tile.h: the *_bf16 functions for staging, the scores and P V.  K, V and Q are rounded to bf16 (nearest even)
// on the way in, Q unscaled; the scale multiplies the fp32 score.  The probabilities are rounded to bf16 only as the operand
// of the second product: the row sum l is formed from the fp32 values.  Everything that is a body's own stays fp32
// arithmetic on unrounded values:
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
#include "attn_stream_fwd.h"

namespace {

template <int D>
__global__ void __launch_bounds__(256)
rel_attn_stream_fwd_bf16_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                const float* __restrict__ embk, const float* __restrict__ embv, const float* __restrict__ mask,
                                float* __restrict__ out, int H, int T, int w, float qscale) {
  rel_attn_stream_fwd_body<TileBF16<D>>(q, k, v, embk, embv, mask, out, H, T, w, qscale, NoHook());
}

template <int D, bool LEN>
__global__ void __launch_bounds__(256)
hubert_attn_fwd_bf16_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                            float* __restrict__ out, int H, int T, size_t ldb, float scale, const int* __restrict__ frames) {
  hubert_attn_fwd_body<TileBF16<D>, LEN>(q, k, v, out, H, T, ldb, scale, frames);
}

struct RelFwdBF16 {
  template <int D>
  static auto kernel() { return rel_attn_stream_fwd_bf16_kernel<D>; }
};
struct HubertFwdBF16 {
  template <int D, bool LEN>
  static auto kernel() { return hubert_attn_fwd_bf16_kernel<D, LEN>; }
};

}  // namespace

// vcv_rel_attn_stream_fwd with bf16 operands: the same arguments, shapes (vcv_rel_attn_stream_supported) and refusals
extern "C" int vcv_rel_attn_stream_fwd_bf16(const float* q, const float* k, const float* v, const float* embk,
                                            const float* embv, const float* mask, float* out, int B, int H, int dk, int T, int w,
                                            float qscale, void* stream) {
  return rel_attn_stream_launch<RelFwdBF16>(q, k, v, embk, embv, mask, out, B, H, dk, T, w, qscale, stream);
}

// vcv_hubert_attn_fwd / vcv_hubert_attn_fwd_len with bf16 operands: the same arguments, shapes (vcv_hubert_attn_supported)
// and refusals
extern "C" int vcv_hubert_attn_fwd_bf16(const float* q, const float* k, const float* v, float* out, int B, int H, int dk, int T,
                                        int64_t ldb, float scale, void* stream) {
  return hubert_attn_launch<HubertFwdBF16>(q, k, v, out, B, H, dk, T, ldb, scale, nullptr, stream);
}

extern "C" int vcv_hubert_attn_fwd_len_bf16(const float* q, const float* k, const float* v, float* out, int B, int H, int dk,
                                            int T, int64_t ldb, float scale, const int* frames, void* stream) {
  return frames ? hubert_attn_launch<HubertFwdBF16>(q, k, v, out, B, H, dk, T, ldb, scale, frames, stream) : VCV_EINVAL;
}
