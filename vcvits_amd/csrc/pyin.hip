// pyin.hip -- pYIN pitch tracking (librosa.pyin as vits/data/audio.py:24-63 calls it), batched over utterances of
// different lengths.  Three stages, each testable on its own against tests/pyin_f64.py; the numbers in the comments are
// the steps of the arithmetic contract (unpinned #5):
//   pyin_yin_kernel      1.-5. reflect padding + framing, fp64 autocorrelation, float32 energy, CMNDF, parabolic shifts
//   pyin_obs_kernel      6.    troughs, threshold priors, candidates -> log-observations [B, F, 2*NB] fp64
//   pyin_viterbi_kernel  7.-8. banded Viterbi (one workgroup per utterance), backtrace, f0 / voicing / pitch class
// Every value that must match numpy to the last bit (thresholds, beta / Boltzmann tables, log-transition band, log(tiny),
// bin frequencies, class table) comes from the host as a table.
#include "common.h"

// No contraction anywhere in this file: the float32 energy prefix and the CMNDF / shift arithmetic are numpy's separate
// roundings (the energy prefix needs an extra guard, see there).  The one fused multiply-add is the fp64 autocorrelation's
// explicit fma().
#pragma clang fp contract(off)

namespace {

constexpr int kFrame = 2048;     // frame_length (the kernels' LDS layout is sized for it)
constexpr int kWin = kFrame / 2; // pyin's internal win_length
constexpr int kYinFrames = 4;    // frames per yin workgroup (one wave each) + one energy wave
constexpr int kMaxHop = 1024;
constexpr int kMaxLag = 256;     // max_period < 256: four lags per lane
constexpr int kNB = 601;         // pitch bins (10 per semitone, C2..C7)
constexpr int kNS = 2 * kNB;     // HMM states: voiced block, then unvoiced block
constexpr int kHalfW = 45;       // transition band: +-45 bins
constexpr int kBand = 2 * kHalfW + 1;
constexpr int kMaxTroughs = 128; // at most 120 troughs in 239 lags (troughs are at least two lags apart)
constexpr int kVitThreads = 640; // ten waves: thread t owns local bin t of both blocks

struct Best {
  double v;
  int i;
};

// larger value wins; equal values: the smaller state index (numpy's first argmax)
__device__ __forceinline__ Best better(Best a, Best b) {
  return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}

__device__ __forceinline__ int reflect_index(int p, int n, int pad) {
  int q = p - pad;
  q = q < 0 ? -q : q;
  const int period = max(2 * (n - 1), 1);
  int r = q % period;
  return r >= n ? period - r : r;
}

}  // namespace

// ---- stage 1 ------------------------------------------------------------------------------------------------------------
// grid (ceil(Fmax / 4), B), 320 threads: waves 0..3 take the autocorrelation of frames 4*bx + w (lane l: lags l + 64k),
// wave 4 runs the four sequential float32 energy prefixes in lanes 0..3.  The block's frames sit in LDS once, as doubles.
__global__ void __launch_bounds__(64 * (kYinFrames + 1))
pyin_yin_kernel(const float* __restrict__ y, const int* __restrict__ n_samples, const int* __restrict__ n_frames,
                int T, int Fmax, int hop, int pad, int lo, int hi, double tiny, double* __restrict__ cmndf,
                double* __restrict__ shifts, int* __restrict__ nonfinite) {
  __shared__ double xs[(kYinFrames - 1) * kMaxHop + kFrame];
  __shared__ float cs_lo[kYinFrames][kMaxLag];
  __shared__ float cs_hi[kYinFrames][kMaxLag];
  __shared__ double dd[kYinFrames][kMaxLag];
  __shared__ double cum[kYinFrames][kMaxLag];
  __shared__ double yin[kYinFrames][kMaxLag];

  const int b = blockIdx.y;
  const int n = min(n_samples[b], T);  // the launchers validate; the clamps keep every access in bounds regardless
  const int nf = min(n_frames[b], Fmax);
  const int f0 = blockIdx.x * kYinFrames;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int nlag = hi - lo + 1;
  const float* yb = y + (size_t)b * T;

  // librosa's valid_audio: every sample of the utterance is finite (each block checks its share)
  {
    const int share = (n + gridDim.x - 1) / gridDim.x;
    const int s0 = blockIdx.x * share;
    const int s1 = min(n, s0 + share);
    int bad = 0;
    for (int i = s0 + tid; i < s1; i += blockDim.x) bad |= !isfinite(yb[i]);
    if (bad) atomicOr(nonfinite, 1);
  }
  if (f0 >= nf) {
    // frames past this utterance's end: zeros (the collate pads with zeros)
    for (int i = tid; i < kYinFrames * nlag; i += blockDim.x) {
      const int f = f0 + i / nlag;
      if (f < Fmax) {
        const size_t o = ((size_t)b * Fmax + f) * nlag + i % nlag;
        cmndf[o] = 0.0;
        shifts[o] = 0.0;
      }
    }
    return;
  }

  // 1. reflect padding is a copy: padded position p of this block's span reads sample reflect(p)
  const int span = (kYinFrames - 1) * hop + kFrame;
  const int p0 = f0 * hop;
  const int plen = n + 2 * pad;
  for (int i = tid; i < span; i += blockDim.x) {
    const int p = p0 + i;
    xs[i] = p < plen ? (double)yb[reflect_index(p, n, pad)] : 0.0;
  }
  __syncthreads();

  if (wave == kYinFrames) {
    // 3. energy: float32 squares, sequential float32 prefix (np.cumsum), one lane per frame
    if (lane < kYinFrames && f0 + lane < nf) {
      const double* x = xs + lane * hop;
      float acc = 0.f;
      for (int i = 0; i <= kWin + hi; ++i) {
        const float v = (float)x[i];
        float sq = v * v;
        // the square must reach the add rounded to float32 (numpy's y**2, then cumsum); the backend fuses
        // v * v + acc into one FMA even under contract(off) and through __fmul_rn / __fadd_rn, so pin sq in a register
        __asm__ volatile("" : "+v"(sq));
        acc = acc + sq;
        if (i <= hi) cs_lo[lane][i] = acc;
        if (i >= kWin) cs_hi[lane][i - kWin] = acc;
      }
    }
  } else if (f0 + wave < nf) {
    // 2. autocorrelation acf[tau] = sum_{m=1..1024} x[m] x[m+tau] in fp64
    const double* x = xs + wave * hop;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int m = 1; m <= kWin; ++m) {
      const double xm = x[m];
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k] = fma(xm, x[m + lane + 64 * k], acc[k]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double a = acc[k];
      dd[wave][lane + 64 * k] = fabs(a) < 1e-6 ? 0.0 : a;
    }
  }
  __syncthreads();
  if (wave == kYinFrames || f0 + wave >= Fmax) return;
  const size_t ob = ((size_t)b * Fmax + f0 + wave) * nlag;
  if (f0 + wave >= nf) {
    for (int k = lane; k < nlag; k += 64) {
      cmndf[ob + k] = 0.0;
      shifts[ob + k] = 0.0;
    }
    return;
  }

  // 4. difference function d[tau] = float64(e[0] + e[tau]) - 2 acf[tau] (energy differences in float32, zeroed below 1e-6)
  {
    const float e0r = __fsub_rn(cs_hi[wave][0], cs_lo[wave][0]);
    const float e0 = fabsf(e0r) < 1e-6f ? 0.f : e0r;
    for (int k = 0; k < 4; ++k) {
      const int tau = lane + 64 * k;
      if (tau > hi) break;
      const float er = __fsub_rn(cs_hi[wave][tau], cs_lo[wave][tau]);
      const float e = fabsf(er) < 1e-6f ? 0.f : er;
      dd[wave][tau] = (double)__fadd_rn(e0, e) - 2.0 * dd[wave][tau];
    }
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  if (lane == 0) {
    double c = 0.0;  // sequential fp64 cumulative sum of d[1..tau]
    for (int tau = 1; tau <= hi; ++tau) {
      c += dd[wave][tau];
      cum[wave][tau] = c;
    }
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  for (int k = lane; k < nlag; k += 64) {
    const int tau = lo + k;
    const double v = dd[wave][tau] / (cum[wave][tau] / (double)tau + tiny);
    yin[wave][k] = v;
    cmndf[ob + k] = v;
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  // 5. parabolic shifts; both end elements 0
  for (int k = lane; k < nlag; k += 64) {
    double s = 0.0;
    if (k > 0 && k < nlag - 1) {
      const double xl = yin[wave][k - 1], xc = yin[wave][k], xr = yin[wave][k + 1];
      const double a = xr + xl - 2.0 * xc;
      const double bb = (xr - xl) / 2.0;
      s = fabs(bb) >= fabs(a) ? 0.0 : -bb / a;
    }
    shifts[ob + k] = s;
  }
}

// ---- stage 2 ------------------------------------------------------------------------------------------------------------
// one wave per frame, four frames per 256-thread block; grid (ceil(Fmax / 4), B).
// thr[101] = linspace(0, 1, 101); beta[100]; gm_bonus[n] = 0.01 * sum(beta[:n]) (n = 0..100);
// pmf[count * pmf_ld + rank] = boltzmann.pmf(rank, 2, count).
__global__ void __launch_bounds__(256)
pyin_obs_kernel(const double* __restrict__ cmndf, const double* __restrict__ shifts, const int* __restrict__ n_frames,
                int Fmax, int nlag, int lo, const double* __restrict__ thr, const double* __restrict__ beta,
                const double* __restrict__ gm_bonus, const double* __restrict__ pmf, int pmf_ld, double sr, double fmin_hz,
                double tiny, double log_tiny, double* __restrict__ log_obs, double* __restrict__ voiced_prob) {
  __shared__ double xs[4][kMaxLag];
  __shared__ int tk[4][kMaxTroughs];
  __shared__ double cprob[4][kMaxTroughs];
  __shared__ int cbin[4][kMaxTroughs];
  __shared__ double obs[4][kNB + 1];
  __shared__ int order[4][kMaxTroughs];

  const int b = blockIdx.y;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int f = blockIdx.x * 4 + wave;
  if (f >= Fmax) return;
  const size_t fo = (size_t)b * Fmax + f;
  double* lob = log_obs + fo * kNS;
  if (f >= min(n_frames[b], Fmax)) {
    for (int j = lane; j < kNS; j += 64) lob[j] = 0.0;
    if (lane == 0) voiced_prob[fo] = 0.0;
    return;
  }
  const double* x = cmndf + fo * nlag;
  const double* sh = shifts + fo * nlag;
  double* X = xs[wave];
  for (int k = lane; k < nlag; k += 64) X[k] = x[k];
  for (int j = lane; j <= kNB; j += 64) obs[wave][j] = 0.0;
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");

  // troughs (localmin with edge padding; element 0: x[0] < x[1]), compacted in lag order
  const unsigned long long below_me = (1ull << lane) - 1ull;
  int J = 0;
  for (int c = 0; c * 64 < nlag; ++c) {
    const int k = c * 64 + lane;
    bool tr = false;
    if (k < nlag) {
      if (k == 0) tr = X[0] < X[1];
      else tr = X[k] < X[k - 1] && (k == nlag - 1 || X[k] <= X[k + 1]);
    }
    const unsigned long long m = __ballot(tr);
    if (tr) tk[wave][J + __popcll(m & below_me)] = k;
    J += __popcll(m);
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");

  double lv = 0.0;
  if (J > 0) {
    // trough slots ja = lane, jb = lane + 64; n_below = number of thresholds[1:] <= height
    const int ja = lane, jb = lane + 64;
    const bool va = ja < J, vb = jb < J;
    const double ha = va ? X[tk[wave][ja]] : 0.0;
    const double hb = vb ? X[tk[wave][jb]] : 0.0;
    int na = 0, nbl = 0;
    for (int t = 1; t <= 100; ++t) {
      const double th = thr[t];
      na += th <= ha;
      nbl += th <= hb;
    }
    // global minimum: first argmin of the trough heights
    Best g = {va ? -ha : -INFINITY, va ? ja : 1 << 20};
    if (vb) g = better(g, Best{-hb, jb});
    for (int o = 32; o > 0; o >>= 1) {
      Best h = {__shfl_xor(g.v, o, 64), __shfl_xor(g.i, o, 64)};
      g = better(g, h);
    }
    // threshold priors: rank of a trough among those below the threshold, in lag order
    double pa = 0.0, pb = 0.0;
    for (int t = 0; t < 100; ++t) {
      const bool ba = va && na <= t, bbl = vb && nbl <= t;
      const unsigned long long ma = __ballot(ba), mb = __ballot(bbl);
      const int ca = __popcll(ma);
      const int count = ca + __popcll(mb);
      if (ba) pa += pmf[count * pmf_ld + __popcll(ma & below_me)] * beta[t];
      if (bbl) pb += pmf[count * pmf_ld + ca + __popcll(mb & below_me)] * beta[t];
    }
    if (g.i == ja) pa += gm_bonus[na];
    if (g.i == jb) pb += gm_bonus[nbl];
    // candidates: period lo + k + shift[k] -> bin clip(rint(120 log2(sr / period / fmin)), 0, NB)
    if (va) {
      const int k = tk[wave][ja];
      const double per = (double)(lo + k) + sh[k];
      const double bi = 120.0 * log2((sr / per) / fmin_hz);
      cprob[wave][ja] = pa;
      cbin[wave][ja] = (int)fmin(fmax(rint(bi), 0.0), (double)kNB);
    }
    if (vb) {
      const int k = tk[wave][jb];
      const double per = (double)(lo + k) + sh[k];
      const double bi = 120.0 * log2((sr / per) / fmin_hz);
      cprob[wave][jb] = pb;
      cbin[wave][jb] = (int)fmin(fmax(rint(bi), 0.0), (double)kNB);
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    // a nonzero candidate wins its bin unless a later (larger-lag) nonzero candidate lands there too (numpy's last write);
    // bin NB is overwritten by the unvoiced fill.  order[]: the winners by ascending bin (numpy sums the rows in order)
    bool win[2] = {false, false};
    for (int s = 0; s < 2; ++s) {
      const int j = lane + 64 * s;
      if (j >= J) continue;
      const int bn = cbin[wave][j];
      bool w = cprob[wave][j] != 0.0 && bn < kNB;
      for (int q = j + 1; q < J && w; ++q) w = !(cprob[wave][q] != 0.0 && cbin[wave][q] == bn);
      win[s] = w;
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    for (int s = 0; s < 2; ++s) {
      const int j = lane + 64 * s;
      if (j < J && !win[s]) cbin[wave][j] = -1;
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    for (int s = 0; s < 2; ++s) {
      const int j = lane + 64 * s;
      if (!win[s]) continue;
      const int bn = cbin[wave][j];
      int rank = 0;
      for (int q = 0; q < J; ++q) {
        const int bq = cbin[wave][q];
        rank += bq >= 0 && bq < bn;
      }
      obs[wave][bn] = cprob[wave][j];
      order[wave][rank] = j;
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    if (lane == 0) {
      int nw = 0;
      for (int j = 0; j < J; ++j) nw += cbin[wave][j] >= 0;
      double s = 0.0;
      for (int r = 0; r < nw; ++r) s += cprob[wave][order[wave][r]];
      lv = s;
    }
  }
  lv = __shfl(lv, 0, 64);
  const double vp = fmin(fmax(lv, 0.0), 1.0);
  const double pu = (1.0 - vp) / (double)kNB;
  const double lu = pu == 0.0 ? log_tiny : log(pu + tiny);
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  for (int j = lane; j < kNB; j += 64) {
    const double p = obs[wave][j];
    lob[j] = p == 0.0 ? log_tiny : log(p + tiny);
  }
  for (int j = lane; j < kNB; j += 64) lob[kNB + j] = lu;
  if (lane == 0) voiced_prob[fo] = vp;
}

// ---- stage 3 ------------------------------------------------------------------------------------------------------------
// one workgroup per utterance (grid B), 640 threads; thread t < NB owns target bin t of both blocks.
// band[s][d][t] (s = 0: same voicing block, 0.99; s = 1: across, 0.01) = log_trans[t + d - 45 -> t]; every entry outside
// the band is log_tiny.  Out-of-band predecessors come from per-block prefix / suffix (value, first index) scans of
// fl(value[i] + log_tiny).
__global__ void __launch_bounds__(kVitThreads)
pyin_viterbi_kernel(const double* __restrict__ log_obs, const double* __restrict__ voiced_prob,
                    const int* __restrict__ n_frames, int Fmax, const double* __restrict__ log_p_init,
                    const double* __restrict__ band, double log_tiny, const float* __restrict__ f0_tab,
                    const float* __restrict__ class_tab, uint16_t* __restrict__ bptr, float* __restrict__ f0,
                    uint8_t* __restrict__ voiced, float* __restrict__ vprob, float* __restrict__ pclass,
                    uint16_t* __restrict__ states) {
  __shared__ double val[2][kNS];
  __shared__ double pre_v[2][kNB], suf_v[2][kNB];
  __shared__ int pre_i[2][kNB], suf_i[2][kNB];
  __shared__ double wtot_v[4][kVitThreads / 64];
  __shared__ int wtot_i[4][kVitThreads / 64];
  __shared__ double red_v[kVitThreads / 64];
  __shared__ int red_i[kVitThreads / 64];

  const int b = blockIdx.x;
  const int t = threadIdx.x;
  const int wave = t >> 6, lane = t & 63;
  const int nw = kVitThreads / 64;
  const int nf = min(n_frames[b], Fmax);
  const size_t row = (size_t)b * Fmax;
  const double* lob = log_obs + row * kNS;
  uint16_t* bp = bptr + row * kNS;

  // 8. frames past the utterance's end are 0
  for (int f = nf + t; f < Fmax; f += kVitThreads) {
    f0[row + f] = 0.f;
    voiced[row + f] = 0;
    vprob[row + f] = 0.f;
    pclass[row + f] = 0.f;
    if (states) states[row + f] = 0;
  }
  if (nf <= 0) return;

  for (int j = t; j < kNS; j += kVitThreads) val[0][j] = lob[j] + log_p_init[j];
  __syncthreads();

  const Best none = {-INFINITY, 1 << 20};
  const int lo = max(0, t - kHalfW), hi = min(kNB - 1, t + kHalfW);
  int cur = 0;
  for (int f = 1; f < nf; ++f) {
    const double* v = val[cur];
    // per-block inclusive prefix and suffix scans of (fl(value + log_tiny), index)
    {
      Best pr[2], su[2];
      for (int a = 0; a < 2; ++a) {
        const Best e = t < kNB ? Best{v[a * kNB + t] + log_tiny, a * kNB + t} : none;
        pr[a] = e;
        su[a] = e;
      }
      for (int o = 1; o < 64; o <<= 1) {
        for (int a = 0; a < 2; ++a) {
          const Best up = {__shfl_up(pr[a].v, o, 64), __shfl_up(pr[a].i, o, 64)};
          const Best dn = {__shfl_down(su[a].v, o, 64), __shfl_down(su[a].i, o, 64)};
          if (lane >= o) pr[a] = better(pr[a], up);
          if (lane + o < 64) su[a] = better(su[a], dn);
        }
      }
      if (lane == 63) {
        for (int a = 0; a < 2; ++a) { wtot_v[a][wave] = pr[a].v; wtot_i[a][wave] = pr[a].i; }
      }
      if (lane == 0) {
        for (int a = 0; a < 2; ++a) { wtot_v[2 + a][wave] = su[a].v; wtot_i[2 + a][wave] = su[a].i; }
      }
      __syncthreads();
      for (int w = 0; w < nw; ++w) {
        for (int a = 0; a < 2; ++a) {
          if (w < wave) pr[a] = better(pr[a], Best{wtot_v[a][w], wtot_i[a][w]});
          if (w > wave) su[a] = better(su[a], Best{wtot_v[2 + a][w], wtot_i[2 + a][w]});
        }
      }
      if (t < kNB) {
        for (int a = 0; a < 2; ++a) {
          pre_v[a][t] = pr[a].v; pre_i[a][t] = pr[a].i;
          suf_v[a][t] = su[a].v; suf_i[a][t] = su[a].i;
        }
      }
      __syncthreads();
    }
    if (t < kNB) {
      // in-band predecessors, ascending index: best[target block][source block]
      Best b00 = none, b01 = none, b10 = none, b11 = none;
      const double* same = band;
      const double* cross = band + (size_t)kBand * kNB;
      for (int i = lo; i <= hi; ++i) {
        const int d = i - t + kHalfW;
        const double v0 = v[i], v1 = v[kNB + i];
        const double cs = same[d * kNB + t], cx = cross[d * kNB + t];
        const double s00 = v0 + cs, s01 = v1 + cx;  // target in block 0 from block 0 / 1
        const double s10 = v0 + cx, s11 = v1 + cs;  // target in block 1 from block 0 / 1
        if (s00 > b00.v) b00 = Best{s00, i};
        if (s01 > b01.v) b01 = Best{s01, kNB + i};
        if (s10 > b10.v) b10 = Best{s10, i};
        if (s11 > b11.v) b11 = Best{s11, kNB + i};
      }
      // out-of-band: [0, lo) and (hi, NB) of each block
      Best out = none;
      for (int a = 0; a < 2; ++a) {
        if (lo > 0) out = better(out, Best{pre_v[a][lo - 1], pre_i[a][lo - 1]});
        if (hi + 1 < kNB) out = better(out, Best{suf_v[a][hi + 1], suf_i[a][hi + 1]});
      }
      const Best t0 = better(better(b00, b01), out);
      const Best t1 = better(better(b10, b11), out);
      const double* lf = lob + (size_t)f * kNS;
      val[cur ^ 1][t] = lf[t] + t0.v;
      val[cur ^ 1][kNB + t] = lf[kNB + t] + t1.v;
      bp[(size_t)f * kNS + t] = (uint16_t)t0.i;
      bp[(size_t)f * kNS + kNB + t] = (uint16_t)t1.i;
    }
    cur ^= 1;
    __syncthreads();
  }

  // final state: first argmax of the last frame's values
  Best m = none;
  for (int j = t; j < kNS; j += kVitThreads) m = better(m, Best{val[cur][j], j});
  for (int o = 32; o > 0; o >>= 1) m = better(m, Best{__shfl_xor(m.v, o, 64), __shfl_xor(m.i, o, 64)});
  if (lane == 0) { red_v[wave] = m.v; red_i[wave] = m.i; }
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < nw; ++w) m = better(m, Best{red_v[w], red_i[w]});
    // backtrace; 8. f0 = bin frequency (0 unvoiced), voiced = state < NB, class from the host's coarse_f0 table
    int s = min(m.i, kNS - 1);  // (NaN inputs: no state wins; keep the walk in bounds)
    for (int f = nf - 1; f >= 0; --f) {
      const int k = s < kNB ? s : kNB;
      f0[row + f] = f0_tab[k];
      voiced[row + f] = s < kNB;
      vprob[row + f] = (float)voiced_prob[row + f];
      pclass[row + f] = class_tab[k];
      if (states) states[row + f] = (uint16_t)s;
      if (f > 0) s = min((int)bp[(size_t)f * kNS + s], kNS - 1);
    }
  }
}

// ---- C ABI ----------------------------------------------------------------------------------------------------------------

extern "C" int vcv_pyin_yin(const float* y, const int* n_samples, const int* n_frames, int B, int T, int Fmax,
                            int frame_length, int hop, int pad, int min_period, int max_period, double tiny,
                            double* cmndf, double* shifts, int* nonfinite, void* stream) {
  if (B <= 0 || Fmax <= 0 || frame_length != kFrame || hop <= 0 || hop > kMaxHop || pad < 0 || min_period < 1 ||
      max_period >= kMaxLag || max_period < min_period + 2 || max_period > kFrame - kWin - 1)
    return VCV_EINVAL;
  dim3 grid(vcv_cdiv(Fmax, kYinFrames), B);
  pyin_yin_kernel<<<grid, 64 * (kYinFrames + 1), 0, (hipStream_t)stream>>>(
      y, n_samples, n_frames, T, Fmax, hop, pad, min_period, max_period, tiny, cmndf, shifts, nonfinite);
  return vcv_check_launch();
}

extern "C" int vcv_pyin_obs(const double* cmndf, const double* shifts, const int* n_frames, int B, int Fmax, int nlag,
                            int min_period, const double* thresholds, const double* beta_probs, const double* gm_bonus,
                            const double* pmf, int pmf_ld, double sr, double fmin, double tiny, double log_tiny,
                            double* log_obs, double* voiced_prob, void* stream) {
  if (B <= 0 || Fmax <= 0 || nlag < 3 || nlag > kMaxLag || pmf_ld <= (nlag + 1) / 2 || min_period < 1)
    return VCV_EINVAL;
  dim3 grid(vcv_cdiv(Fmax, 4), B);
  pyin_obs_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(cmndf, shifts, n_frames, Fmax, nlag, min_period, thresholds,
                                                           beta_probs, gm_bonus, pmf, pmf_ld, sr, fmin, tiny, log_tiny,
                                                           log_obs, voiced_prob);
  return vcv_check_launch();
}

extern "C" int vcv_pyin_viterbi(const double* log_obs, const double* voiced_prob, const int* n_frames, int B, int Fmax,
                                int n_states, const double* log_p_init, const double* band, int band_width,
                                double log_tiny, const float* f0_table, const float* class_table, uint16_t* backptr,
                                float* f0, uint8_t* voiced, float* vprob, float* pclass, uint16_t* states,
                                void* stream) {
  if (B <= 0 || Fmax <= 0 || n_states != kNS || band_width != kBand) return VCV_EINVAL;
  pyin_viterbi_kernel<<<B, kVitThreads, 0, (hipStream_t)stream>>>(log_obs, voiced_prob, n_frames, Fmax, log_p_init,
                                                                  band, log_tiny, f0_table, class_table, backptr, f0,
                                                                  voiced, vprob, pclass, states);
  return vcv_check_launch();
}
