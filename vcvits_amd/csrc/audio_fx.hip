// audio_fx.hip -- the front of the audio path: band-limited sinc resampling (torchaudio.transforms.Resample with its
// defaults, vits/data/audio.py:158-172), the phase vocoder and the ordered inverse STFT of torchaudio.functional.pitch_shift
// (vits/data/audio.py:174-180, infer.py:45-46).  Each kernel is testable on its own against tests/audio_fx_f64.py; the
// arithmetic contract is DESIGN 3.1, unpinned #6.
//   resample_table_kernel   per phase p: first tap inside the band and the W taps from there, float64 -> float32
//   resample_apply_kernel   y[b, i*n + p] = sum_w tap[w][p] * x[b, i*o + first[p] - width + w], input span staged in LDS
//   phase_vocoder_kernel    one wavefront per (b, bin) row, 64 frames per step, float64 phase with a cross-lane scan
//   istft_ordered_kernel    inverse STFT whose overlap-add sums the frames in ascending order (bit-reproducible)
#include "common.h"

// The table follows torch's separate float64 roundings; the one fused multiply-add is the apply kernel's explicit fmaf().
#pragma clang fp contract(off)

namespace {

constexpr int kRsThreads = 256;
constexpr int kIstThreads = 256;
constexpr double kPi = 3.14159265358979323846;
constexpr double kLpw = 6.0;  // lowpass_filter_width

// (-p / n as float32 + (k - width) / o) * base: torchaudio's tap position before clamping
__device__ __forceinline__ double tap_pos(double tp, int k, int width, int o, double base) {
  return (tp + (double)(k - width) / (double)o) * base;
}

}  // namespace

// ---- resample: table ------------------------------------------------------------------------------------------------
// One lane per phase.  first[p] = smallest k in [0, 2*width + o) with |t| < 6; taps[w * n + p] = float32 tap first[p] + w
// (0 past the bank's last tap), so lanes with consecutive p read consecutive words.
__global__ void __launch_bounds__(kRsThreads)
resample_table_kernel(int o, int n, int width, int W, double base, double scale, int* __restrict__ first,
                      float* __restrict__ taps) {
  const int p = blockIdx.x * kRsThreads + threadIdx.x;
  if (p >= n) return;
  const int K = 2 * width + o;
  // float32(-p) / float32(n) in float32; the double quotient rounded once is the same value (53 >= 2 * 24 + 2)
  const double tp = (double)(float)((double)(-p) / (double)n);
  int k = (int)floor((double)width + (double)o * (double)p / (double)n - kLpw * (double)o / base) - 2;
  k = min(max(k, 0), K);
  while (k > 0 && fabs(tap_pos(tp, k - 1, width, o, base)) < kLpw) --k;
  while (k < K && !(fabs(tap_pos(tp, k, width, o, base)) < kLpw)) ++k;
  first[p] = k;
  for (int w = 0; w < W; ++w) {
    float v = 0.f;
    if (k + w < K) {
      double t = tap_pos(tp, k + w, width, o, base);
      t = fmin(fmax(t, -kLpw), kLpw);
      double win = cos(t * kPi / kLpw / 2.0);
      win = win * win;
      t *= kPi;
      double s = t == 0.0 ? 1.0 : sin(t) / t;
      s *= win * scale;
      v = (float)s;
    }
    taps[(size_t)w * n + p] = v;
  }
}

// ---- resample: apply ------------------------------------------------------------------------------------------------
// grid (ceil(Tout / (256 * PER)), B).  The tile's input span [lo, lo + span) goes to LDS (16-byte loads when the rows are
// aligned), then thread t takes outputs j0 + t + 256 m: W fused multiply-adds in tap order, whatever the batch.  A tap
// window that is not inside the staged span (never, by the span's derivation in the launcher) reads global memory with
// bounds checks instead.
template <int PER>
__global__ void __launch_bounds__(kRsThreads)
resample_apply_kernel(const float* __restrict__ x, const int* __restrict__ lens, float* __restrict__ y, int T, int Tout,
                      int o, int n, int width, int W, const int* __restrict__ first, const float* __restrict__ taps,
                      int span, int vec) {
  extern __shared__ __attribute__((aligned(16))) float rs_xs[];
  const int b = blockIdx.y, t = threadIdx.x;
  const int len = lens ? min(lens[b], T) : T;
  const long long outlen = ((long long)n * len + o - 1) / o;
  const int j0 = blockIdx.x * (kRsThreads * PER);
  float* yb = y + (size_t)b * Tout;
  if (j0 >= outlen) {
    for (int m = 0; m < PER; ++m) {
      const int j = j0 + t + kRsThreads * m;
      if (j < Tout) yb[j] = 0.f;
    }
    return;
  }
  const float* xb = x + (size_t)b * T;
  long long lo = ((long long)j0 * o) / n - width - 2;
  lo -= ((lo % 4) + 4) % 4;
  if (vec) {
    for (int q = t * 4; q < span; q += kRsThreads * 4) {
      const long long g = lo + q;
      float4 v;
      if (g >= 0 && g + 3 < len) {
        v = *reinterpret_cast<const float4*>(xb + g);
      } else {
        v.x = (g >= 0 && g < len) ? xb[g] : 0.f;
        v.y = (g + 1 >= 0 && g + 1 < len) ? xb[g + 1] : 0.f;
        v.z = (g + 2 >= 0 && g + 2 < len) ? xb[g + 2] : 0.f;
        v.w = (g + 3 >= 0 && g + 3 < len) ? xb[g + 3] : 0.f;
      }
      *reinterpret_cast<float4*>(rs_xs + q) = v;
    }
  } else {
    for (int q = t; q < span; q += kRsThreads) {
      const long long g = lo + q;
      rs_xs[q] = (g >= 0 && g < len) ? xb[g] : 0.f;
    }
  }
  __syncthreads();
  for (int m = 0; m < PER; ++m) {
    const int j = j0 + t + kRsThreads * m;
    if (j >= Tout) continue;
    float acc = 0.f;
    if (j < outlen) {
      const int i = j / n, p = j - i * n;
      const long long s = (long long)i * o + first[p] - width;
      const float* tp = taps + p;
      const long long r = s - lo;
      if (r >= 0 && r + W <= span) {
        const float* xr = rs_xs + (int)r;
        for (int w = 0; w < W; ++w) acc = fmaf(tp[(size_t)w * n], xr[w], acc);
      } else {
        for (int w = 0; w < W; ++w) {
          const long long g = s + w;
          acc = fmaf(tp[(size_t)w * n], (g >= 0 && g < len) ? xb[g] : 0.f, acc);
        }
      }
    }
    yb[j] = acc;
  }
}

// ---- phase vocoder --------------------------------------------------------------------------------------------------
// 256 threads = four rows.  Lane l of a step holds output frame s = s0 + l: its magnitude from time step float32(s * rate),
// and term s of the summed sequence [angle(S[0]), inc_0, inc_1, ...] (inc_{s-1}, from time step s - 1).  Inclusive scan
// over the lanes plus the carry of the steps before; everything in float64, rounded once at the store.
namespace {

__device__ __forceinline__ float2 pv_frame(const float2* __restrict__ row, int i, int F) {
  return (i >= 0 && i < F) ? row[i] : make_float2(0.f, 0.f);
}

__device__ __forceinline__ double pv_angle(float2 v) { return atan2((double)v.y, (double)v.x); }

}  // namespace

__global__ void __launch_bounds__(256)
phase_vocoder_kernel(const float2* __restrict__ spec, float2* __restrict__ out, const float* __restrict__ adv, int rows,
                     int NF, int F, int Fo, double rate) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;  // a whole wavefront; no workgroup barrier below
  const float2* sr = spec + (size_t)row * F;
  float2* orow = out + (size_t)row * Fo;
  const double a = (double)adv[row % NF];
  const double two_pi = 2.0 * kPi;
  double carry = 0.0;
  for (int s0 = 0; s0 < Fo; s0 += 64) {
    const int s = s0 + lane;
    double term = 0.0, mag = 0.0;
    if (s < Fo) {
      const float ts = (float)((double)s * rate);
      const float2 v0 = pv_frame(sr, (int)ts, F), v1 = pv_frame(sr, (int)(ts + 1.0f), F);
      const double alpha = (double)(ts - truncf(ts));
      mag = alpha * hypot((double)v1.x, (double)v1.y) + (1.0 - alpha) * hypot((double)v0.x, (double)v0.y);
      if (s == 0) {
        term = pv_angle(sr[0]);
      } else {
        const float tq = (float)((double)(s - 1) * rate);
        const double a0 = pv_angle(pv_frame(sr, (int)tq, F)), a1 = pv_angle(pv_frame(sr, (int)(tq + 1.0f), F));
        double v = a1 - a0 - a;
        v = v - two_pi * rint(v / two_pi);
        term = v + a;
      }
    }
    for (int d = 1; d < 64; d <<= 1) {
      const double up = __shfl_up(term, d, 64);
      if (lane >= d) term += up;
    }
    const double phase = carry + term;
    carry += __shfl(term, 63, 64);
    if (s < Fo) orow[s] = make_float2((float)(mag * cos(phase)), (float)(mag * sin(phase)));
  }
}

// ---- ordered inverse STFT -------------------------------------------------------------------------------------------
// torch.istft(center=True, length=) for a power-of-two n_fft and hop = n_fft / 4.  A workgroup inverts G consecutive frames
// into LDS, four at a time, one per wavefront (conjugate-symmetric extension, radix-2 passes, real part / n_fft, times the
// window) and writes the G - 3 hop blocks they cover completely: each output sample sums its (up to) four frames in
// ascending frame order and divides by the window envelope summed in the same order.  No atomics: two runs, and a row alone or in a batch, give the same bits.
__global__ void __launch_bounds__(kIstThreads)
istft_ordered_kernel(const float2* __restrict__ spec, const float* __restrict__ window, const float2* __restrict__ tw,
                     float* __restrict__ out, int F, int n_fft, int logn, int G, int length) {
  extern __shared__ __attribute__((aligned(16))) float ist_smem[];
  float2* bufs = reinterpret_cast<float2*>(ist_smem);  // [4][n_fft]: one transform per wavefront
  float* fr = ist_smem + 8 * n_fft;                    // [G][n_fft]
  const int half = n_fft / 2, hop = n_fft / 4, nbin = half + 1;
  const int b = blockIdx.y, m0 = blockIdx.x * (G - 3), f_lo = m0 - 3;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float inv = 1.f / (float)n_fft;
  for (int q0 = 0; q0 < G; q0 += 4) {  // G is a multiple of 4; the barriers are reached by every wavefront
    const int q = q0 + wave, f = f_lo + q;
    const bool live = f >= 0 && f < F;
    float2* buf = bufs + (size_t)wave * n_fft;
    float* fq = fr + (size_t)q * n_fft;
    if (live) {
      const float2* sb = spec + (size_t)b * nbin * F + f;
      for (int k = lane; k < n_fft; k += 64) {
        float2 v;
        if (k <= half) {
          v = sb[(size_t)k * F];
          v.y = (k == 0 || k == half) ? 0.f : -v.y;
        } else {
          v = sb[(size_t)(n_fft - k) * F];
        }
        buf[__brev((unsigned)k) >> (32 - logn)] = v;
      }
    }
    __syncthreads();
    for (int st = 1; st <= logn; ++st) {
      const int hm = 1 << (st - 1), step = n_fft >> st;
      if (live) {
        for (int u = lane; u < half; u += 64) {
          const int pos = u & (hm - 1), i = ((u >> (st - 1)) << st) + pos, j = i + hm;
          const float2 w = tw[pos * step], c = buf[i], d = buf[j];
          const float2 e = make_float2(d.x * w.x - d.y * w.y, d.x * w.y + d.y * w.x);
          buf[i] = make_float2(c.x + e.x, c.y + e.y);
          buf[j] = make_float2(c.x - e.x, c.y - e.y);
        }
      }
      __syncthreads();
    }
    for (int i = lane; i < n_fft; i += 64) fq[i] = live ? buf[i].x * inv * window[i] : 0.f;
    __syncthreads();
  }
  float* ob = out + (size_t)b * length;
  for (int idx = threadIdx.x; idx < (G - 3) * hop; idx += kIstThreads) {
    const int m = m0 + idx / hop;
    const int i = m * hop + idx % hop;  // index into the untrimmed overlap-add
    const int tt = i - half;
    if (tt < 0 || tt >= length) continue;
    float sum = 0.f, env = 0.f;
    for (int f = m - 3; f <= m; ++f) {
      if (f < 0 || f >= F) continue;
      const int nn = i - f * hop;
      const float w = window[nn];
      sum += fr[(size_t)(f - f_lo) * n_fft + nn];
      env += w * w;
    }
    ob[tt] = env > 1e-11f ? sum / env : 0.f;
  }
}

// ---- C ABI ----------------------------------------------------------------------------------------------------------

extern "C" int vcv_resample_table(int o, int n, int width, int W, double base, int* first, float* taps, void* stream) {
  if (!first || !taps || o <= 0 || n <= 0 || width <= 0 || W <= 0 || !(base > 0.0)) return VCV_EINVAL;
  resample_table_kernel<<<vcv_cdiv(n, kRsThreads), kRsThreads, 0, (hipStream_t)stream>>>(o, n, width, W, base,
                                                                                           base / (double)o, first, taps);
  return vcv_check_launch();
}

extern "C" int vcv_resample_apply(const float* x, const int* lens, float* y, int B, int T, int Tout, int o, int n,
                                  int width, int W, const int* first, const float* taps, void* stream) {
  if (!x || !y || !first || !taps || B <= 0 || B > 65535 || T <= 0 || Tout <= 0 || o <= 0 || n <= 0 || width <= 0 ||
      W <= 0)
    return VCV_EINVAL;
  const int vec = ((uintptr_t)x % 16 == 0 && T % 4 == 0) ? 1 : 0;
  // a tile of TJ outputs reads inputs [floor(j0 o / n) - width - 2 - 3, floor((j0 + TJ - 1) o / n) + width + 2]: tap
  // first[p] sits in (j o / n - 6 o / base, that + 1] and W <= 12 o / base + 2 <= 2 width + 2
  auto span_of = [&](int tj) { return (((long long)tj * o + n - 1) / n + 2LL * width + 12 + 3) / 4 * 4; };
  const long long lds_max = 64 * 1024 / sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  if (span_of(4 * kRsThreads) <= lds_max) {
    const int span = (int)span_of(4 * kRsThreads);
    dim3 grid(vcv_cdiv(Tout, 4 * kRsThreads), B);
    resample_apply_kernel<4><<<grid, kRsThreads, sizeof(float) * span, st>>>(x, lens, y, T, Tout, o, n, width, W, first,
                                                                             taps, span, vec);
  } else if (span_of(kRsThreads) <= lds_max) {
    const int span = (int)span_of(kRsThreads);
    dim3 grid(vcv_cdiv(Tout, kRsThreads), B);
    resample_apply_kernel<1><<<grid, kRsThreads, sizeof(float) * span, st>>>(x, lens, y, T, Tout, o, n, width, W, first,
                                                                             taps, span, vec);
  } else {
    return VCV_EINVAL;  // decimation by more than about 59: the span of one tile does not fit in LDS
  }
  return vcv_check_launch();
}

extern "C" int vcv_phase_vocoder(const float* spec, float* out, const float* phase_advance, int B, int n_freq, int F,
                                 int F_out, double rate, void* stream) {
  if (!spec || !out || !phase_advance || B <= 0 || n_freq <= 0 || F <= 0 || F_out <= 0 || !(rate > 0.0)) return VCV_EINVAL;
  const long long rows = (long long)B * n_freq;
  if (rows > 0x7fffffffLL) return VCV_EINVAL;
  phase_vocoder_kernel<<<(unsigned)((rows + 3) / 4), 256, 0, (hipStream_t)stream>>>(
      (const float2*)spec, (float2*)out, phase_advance, (int)rows, n_freq, F, F_out, rate);
  return vcv_check_launch();
}

extern "C" int vcv_istft_ordered(const float* spec, const float* window, const float* twiddle, float* out, int B, int F,
                                 int n_fft, int length, void* stream) {
  if (!spec || !window || !twiddle || !out || B <= 0 || B > 65535 || F <= 0 || length <= 0) return VCV_EINVAL;
  if (n_fft < 64 || n_fft > 1024 || (n_fft & (n_fft - 1))) return VCV_EINVAL;
  int logn = 0;
  while ((1 << logn) < n_fft) ++logn;
  const int G = n_fft <= 512 ? 16 : 8, hop = n_fft / 4;
  const int blocks = vcv_cdiv(length + n_fft / 2, hop);  // hop blocks of the overlap-add that reach the output
  dim3 grid(vcv_cdiv(blocks, G - 3), B);
  const size_t lds = sizeof(float) * (size_t)n_fft * (8 + G);  // four transform buffers + G frames: at most 64 KB
  istft_ordered_kernel<<<grid, kIstThreads, lds, (hipStream_t)stream>>>((const float2*)spec, window, (const float2*)twiddle,
                                                                        out, F, n_fft, logn, G, length);
  return vcv_check_launch();
}
