// hubert.hip -- what HuBERT inference (vcvits_amd/model/hubert.py) needs beyond the conv family and layernorm_c:
//   * softmax self-attention, forward only, keys / values streamed in tiles (no [T, T] tensor in memory), on the frame of
//     attn_stream_tile.h that the streamed relative-position kernels share; the kernel is hubert_attn_fwd_body of
//     attn_stream_fwd.h with fp32 operands, the body attention_stream_bf16.hip instantiates with bf16 ones;
//   * GroupNorm(C, C) over time fused with GELU (layer 0 of the base model's conv front end);
//   * LayerNorm over channels fused with GELU (every layer of the large models' front end);
//   * bias + exact GELU (+ residual) as one streaming pass.
// Everything is [B, C, T] float32 with T contiguous, as in the rest of the library.
//
// Rows of unequal length in one padded batch (extract_features(lengths=)): the features of a row are those of the row
// computed alone.  Three entry points carry a device array of one int per batch row for that, and everything else of the
// model is per frame already (frames past a row's end may hold anything there: nothing valid reads them):
//   * vcv_hubert_groupnorm_gelu_len  statistics over the first counts[b] samples of a row, exact 0 written behind them;
//   * vcv_hubert_mask_frames         y = t < frames[b] ? x : 0, on the input of the position conv (a row alone sees zero
//                                    padding there) and on the final features;
//   * vcv_hubert_attn_fwd_len        keys s < frames[b] only, exact 0 for the queries behind them.
// All three select, never multiply: NaN or Inf behind a row's end does not reach a valid frame.  The entry points without
// lengths are the same kernels instantiated without the array, with the instructions they had before it existed.
#include "attn_stream_fwd.h"

namespace {

__device__ __forceinline__ float hubert_gelu(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752440f)); }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// ---- y[r, t] = res[r, t] + gelu(x[r, t] + bias[r % C]) for t < T; rows of x are Tin >= T floats apart (the position
// conv yields T + 1 frames and fairseq drops the last), rows of res / y T apart; bias / res may be null -----------------
__global__ void __launch_bounds__(256)
hubert_bias_gelu_kernel(const float* x, const float* __restrict__ bias, const float* res,
                        float* y, int C, int Tin, int T, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const size_t r = i / (size_t)T;
  const int t = (int)(i - r * (size_t)T);
  float v = x[r * (size_t)Tin + t];
  if (bias) v += bias[(int)(r % (size_t)C)];
  v = hubert_gelu(v);
  if (res) v += res[i];
  y[i] = v;
}

// ---- y[b, c, t] = t < frames[b] ? x[b, c, t] : 0 (a select: whatever lies behind a row's end becomes exact 0, NaN
// included); one streaming pass, y may be x ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
hubert_mask_frames_kernel(const float* x, float* y, int C, int T, const int* __restrict__ frames, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const size_t r = i / (size_t)T;
  const int t = (int)(i - r * (size_t)T);
  float v = 0.f;
  if (t < frames[r / (size_t)C]) v = x[i];
  y[i] = v;
}

// ---- GroupNorm(C, C) + GELU: one block per (b, c) row of T samples.  Pass 1 sums x and x^2 in float64 (a row of the base
// model's first layer has 1e5 - 1e6 samples, and a float32 sum of squares loses the variance as soon as the row has an
// offset); pass 2 re-reads the row (from L2 while it fits), subtracts the mean as a two-float value, and writes once.
// y may be x.  LEN: the statistics and the normalised output cover the first n = counts[b] samples of the row (clamped to
// [1, T]; samples behind them are never read), and y[n .. T) is written as exact 0.  n = 1 has variance 0 and yields
// gelu(beta).  Without LEN n is T and the code is what it was. -----------------------------------------------------------
template <bool LEN>
__global__ void __launch_bounds__(256)
hubert_groupnorm_gelu_kernel(const float* x, const float* __restrict__ gamma, const float* __restrict__ beta, float* y,
                             int C, int Trow, float eps, const int* __restrict__ counts) {
  __shared__ double red[2][4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const size_t row = blockIdx.x;
  const float* xr = x + row * (size_t)Trow;
  float* yr = y + row * (size_t)Trow;
  int T = Trow;  // the samples that count
  if (LEN) T = min(max(counts[row / (size_t)C], 1), Trow);
  // 16-byte loads over the aligned middle of the row when x and y rows are misaligned alike, scalars around it
  int head = (int)((4 - (((uintptr_t)xr >> 2) & 3)) & 3);
  if ((((uintptr_t)xr ^ (uintptr_t)yr) & 15) != 0 || head > T) head = T;
  const int n4 = (T - head) >> 2, tail0 = head + 4 * n4;
  const float4* x4 = (const float4*)(xr + head);
  float4* y4 = (float4*)(yr + head);
  double s = 0.0, q = 0.0;
  for (int i = tid; i < head; i += 256) { const double a = xr[i]; s += a; q += a * a; }
  for (int i = tid; i < n4; i += 256) {
    const float4 v = x4[i];
    const double a = v.x, b = v.y, c = v.z, d = v.w;
    s += (a + b) + (c + d);
    q += (a * a + b * b) + (c * c + d * d);
  }
  for (int i = tail0 + tid; i < T; i += 256) { const double a = xr[i]; s += a; q += a * a; }
  s = wave_sum(s);
  q = wave_sum(q);
  if (lane == 0) { red[0][wv] = s; red[1][wv] = q; }
  __syncthreads();
  s = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
  q = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  const double mean = s / T;
  double var = q / T - mean * mean;
  var = var > 0.0 ? var : 0.0;
  const float mhi = (float)mean, mlo = (float)(mean - (double)mhi);
  const int ch = (int)(row % (size_t)C);
  const float g = (float)(1.0 / sqrt(var + (double)eps)) * gamma[ch], bt = beta[ch];
  for (int i = tid; i < head; i += 256) yr[i] = hubert_gelu(((xr[i] - mhi) - mlo) * g + bt);
  for (int i = tid; i < n4; i += 256) {
    float4 v = x4[i];
    v.x = hubert_gelu(((v.x - mhi) - mlo) * g + bt);
    v.y = hubert_gelu(((v.y - mhi) - mlo) * g + bt);
    v.z = hubert_gelu(((v.z - mhi) - mlo) * g + bt);
    v.w = hubert_gelu(((v.w - mhi) - mlo) * g + bt);
    y4[i] = v;
  }
  for (int i = tail0 + tid; i < T; i += 256) yr[i] = hubert_gelu(((xr[i] - mhi) - mlo) * g + bt);
  if (LEN)
    for (int i = T + tid; i < Trow; i += 256) yr[i] = 0.f;
}

// ---- LayerNorm over C + GELU for [B, C, T]: a block is 64 consecutive t (lanes) x 4 channel groups (waves); one pass
// of float64 sums, one pass that normalises, activates and writes (two reads, one write).  y may be x. --------------------
__global__ void __launch_bounds__(256)
hubert_layernorm_c_gelu_kernel(const float* x, const float* __restrict__ gamma, const float* __restrict__ beta, float* y,
                               int C, int T, float eps) {
  __shared__ double red[2][4][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int b = blockIdx.y, t = blockIdx.x * 64 + lane;
  const bool ok = t < T;
  const size_t base = (size_t)b * C * T + (ok ? t : 0);
  double s = 0.0, q = 0.0;
#pragma unroll 4
  for (int c = wv; c < C; c += 4) {
    const double a = x[base + (size_t)c * T];
    s += a;
    q += a * a;
  }
  red[0][wv][lane] = s;
  red[1][wv][lane] = q;
  __syncthreads();
  s = (red[0][0][lane] + red[0][1][lane]) + (red[0][2][lane] + red[0][3][lane]);
  q = (red[1][0][lane] + red[1][1][lane]) + (red[1][2][lane] + red[1][3][lane]);
  const double mean = s / C;
  double var = q / C - mean * mean;
  var = var > 0.0 ? var : 0.0;
  const float mhi = (float)mean, mlo = (float)(mean - (double)mhi);
  const float rs = (float)(1.0 / sqrt(var + (double)eps));
  if (!ok) return;
#pragma unroll 4
  for (int c = wv; c < C; c += 4) {
    const size_t o = base + (size_t)c * T;
    y[o] = hubert_gelu(((x[o] - mhi) - mlo) * rs * gamma[c] + beta[c]);
  }
}

// ---- softmax((q * scale)^T k) v per head, forward only, on the streamed frame of attn_stream_tile.h (layout, tiles and
// the two MFMA contractions are described there), with expf: hubert_attn_fwd_body<TileF32<D>, LEN> (attn_stream_fwd.h), which
// the following describes.  q / k / v / out: [B, H * D, T]; batch rows of q / k / v are
// `ldb` floats apart (H * D * T, or 3 * H * D * T when the three are slices of one fused projection).  Grid
// (ceil(T / 128), B * H), 256 threads.  D = 80 pads the value tile to 96 rows of zeros (3 output tiles of 32 channels).
// LEN: a head of batch row b sees the keys s < n = frames[b] only (precondition 1 <= frames[b] <= T, so key 0 exists; the
// value is clamped into that range, so a bad one cannot read out of bounds).  The key loop ends at n, keys / values and
// queries at or behind n are staged as 0 by a select (whatever is stored there, NaN included, is never used), their scores
// are -inf, and the output of the queries t >= n is exact 0.  A block whose 128 queries all lie behind n writes its zeros
// and leaves before the first barrier (n is uniform over the block).  Without LEN n is T and the code is what it was.
// Resources (hipcc -O3, gfx950, from the code object's metadata; tests/test_attention_stream_cpu.py holds them): D = 64: 192
// registers, 51 / 55 SGPR without / with LEN, 16,640 B LDS; D = 80: 248 registers, 52 / 55 SGPR, 22,912 B LDS; 0 B scratch,
// no spills. ------
template <int D, bool LEN>
__global__ void __launch_bounds__(256)
hubert_attn_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                       float* __restrict__ out, int H, int T, size_t ldb, float scale, const int* __restrict__ frames) {
  hubert_attn_fwd_body<TileF32<D>, LEN>(q, k, v, out, H, T, ldb, scale, frames);
}

struct HubertFwdF32 {
  template <int D, bool LEN>
  static auto kernel() { return hubert_attn_fwd_kernel<D, LEN>; }
};

}  // namespace

extern "C" int vcv_hubert_bias_gelu(const float* x, const float* bias, const float* res, float* y, int R, int C, int Tin,
                                    int T, void* stream) {
  if (!x || !y || R <= 0 || C <= 0 || T <= 0 || Tin < T) return VCV_EINVAL;
  const size_t n = (size_t)R * T;
  const size_t blocks = (n + 255) / 256;
  if (blocks > 0x7fffffffULL) return VCV_EINVAL;
  hubert_bias_gelu_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(x, bias, res, y, C, Tin, T, n);
  return vcv_check_launch();
}

// counts: null launches the kernel without lengths
static int groupnorm_gelu_launch(const float* x, const float* gamma, const float* beta, float* y, int B, int C, int T,
                                 const int* counts, float eps, void* stream) {
  if (!x || !gamma || !beta || !y || B <= 0 || C <= 0 || T <= 0) return VCV_EINVAL;
  const long long rows = (long long)B * C;
  if (rows > 0x7fffffffLL) return VCV_EINVAL;
  const auto kernel = counts ? hubert_groupnorm_gelu_kernel<true> : hubert_groupnorm_gelu_kernel<false>;
  kernel<<<(unsigned)rows, 256, 0, (hipStream_t)stream>>>(x, gamma, beta, y, C, T, eps, counts);
  return vcv_check_launch();
}

extern "C" int vcv_hubert_groupnorm_gelu(const float* x, const float* gamma, const float* beta, float* y, int B, int C, int T,
                                         float eps, void* stream) {
  return groupnorm_gelu_launch(x, gamma, beta, y, B, C, T, nullptr, eps, stream);
}

extern "C" int vcv_hubert_groupnorm_gelu_len(const float* x, const float* gamma, const float* beta, float* y, int B, int C,
                                             int T, const int* counts, float eps, void* stream) {
  return counts ? groupnorm_gelu_launch(x, gamma, beta, y, B, C, T, counts, eps, stream) : VCV_EINVAL;
}

extern "C" int vcv_hubert_mask_frames(const float* x, float* y, int B, int C, int T, const int* frames, void* stream) {
  if (!x || !y || !frames || B <= 0 || C <= 0 || T <= 0) return VCV_EINVAL;
  const size_t n = (size_t)B * C * T;
  const size_t blocks = (n + 255) / 256;
  if (blocks > 0x7fffffffULL) return VCV_EINVAL;
  hubert_mask_frames_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(x, y, C, T, frames, n);
  return vcv_check_launch();
}

extern "C" int vcv_hubert_layernorm_c_gelu(const float* x, const float* gamma, const float* beta, float* y, int B, int C,
                                           int T, float eps, void* stream) {
  if (!x || !gamma || !beta || !y || B <= 0 || B > 65535 || C <= 0 || T <= 0) return VCV_EINVAL;
  hubert_layernorm_c_gelu_kernel<<<dim3(vcv_cdiv(T, 64), B), 256, 0, (hipStream_t)stream>>>(x, gamma, beta, y, C, T, eps);
  return vcv_check_launch();
}

extern "C" int vcv_hubert_attn_supported(int B, int H, int dk, int T) {
  if (B <= 0 || H <= 0 || T <= 0 || (long long)B * H > 65535) return 1;
  return (dk == 64 || dk == 80) ? 0 : 1;
}

extern "C" int vcv_hubert_attn_fwd(const float* q, const float* k, const float* v, float* out, int B, int H, int dk, int T,
                                   int64_t ldb, float scale, void* stream) {
  return hubert_attn_launch<HubertFwdF32>(q, k, v, out, B, H, dk, T, ldb, scale, nullptr, stream);
}

extern "C" int vcv_hubert_attn_fwd_len(const float* q, const float* k, const float* v, float* out, int B, int H, int dk, int T,
                                       int64_t ldb, float scale, const int* frames, void* stream) {
  return frames ? hubert_attn_launch<HubertFwdF32>(q, k, v, out, B, H, dk, T, ldb, scale, frames, stream) : VCV_EINVAL;
}
