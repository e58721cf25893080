// conv_plan.h -- the host side that the packed-weight convolution families share (conv_dma.hip, conv_pk_kernel.h with its
// fp32 / bf16 / 16-bit-activation instances, conv_x3.hip): which launches such a kernel can take at all, the span geometry of
// a tile, the occupancy figures the tile heuristics weigh, and everything a launcher does after its weight pack.
// The heuristics themselves -- every measured threshold -- stay in each family's choose().  Host-only.
#pragma once
#include <type_traits>
#include "common.h"
#include "prof.h"

namespace {

// One-group launches of the forward type (a_mode 0) or phased (transposed conv / strided data gradient, one residue per
// phase), input transform none or a leaky-ReLU with slope in [0, 1), at least 32 rows x 16 reduction channels, at most 16
// taps, tensors whose flattened rows index in 31 bits, out_tf none or one of DLEAKY / DRELU / DTANH with `oaux` given.  What
// the families differ in: s_le_3 (the family stages no span longer
// than stride 3's); io (the storage combination of the instance: VcvConvArgs.io must match it, and only io != 0 has the
// post-scale and the merged form, ms > 1: all output phases of a transposed conv as rows of one launch).
inline bool conv_eligible(const VcvConvArgs& a, bool s_le_3, int io = 0) {
  if (a.io != io || (io == 0 && a.post_scale != 0.f)) return false;
  // the epilogues act on these three derivative masks only, and read `oaux` for each of them
  const bool out_tf_ok = a.out_tf == VCV_TF_NONE ||
                         ((a.out_tf == VCV_TF_DLEAKY || a.out_tf == VCV_TF_DRELU || a.out_tf == VCV_TF_DTANH) && a.oaux);
  if (!out_tf_ok) return false;
  const bool fwd_type = a.a_mode == 0 && a.phases <= 1;
  const bool phased = a.a_mode == 1 && a.phases > 1 && a.s == 1 && a.dj == -1;
  // (16-bit activations only: the epilogue that interleaves the phases)
  const bool merged = io != 0 && a.a_mode == 1 && a.phases <= 1 && a.s == 1 && a.dj == -1 && a.os == a.ms && a.P == 1 &&
                      a.Mg % a.ms == 0 && !a.res && !a.mask && !a.accumulate;
  return (a.ms > 1 ? merged : (fwd_type || phased)) && a.G == 1 &&
         (a.in_tf == VCV_TF_NONE || (a.in_tf == VCV_TF_LEAKY && a.slope < 1.f && a.slope >= 0.f)) && a.Mg >= 32 &&
         a.Cg >= 16 && a.K <= 16 && a.s >= 1 && (!s_le_3 || a.s <= 3) && (long long)a.Tin * a.P * 4 < (1ll << 31) &&
         (long long)a.Mg * a.Tout * a.P < (1ll << 31);
}

inline int conv_phases(const VcvConvArgs& a) { return a.phases > 1 ? a.phases : 1; }

// Span geometry of a BM x BN tile into g (DmaGeom / BfGeom): residues, taps per residue, the staged input span per channel
// (a multiple of 64; `slack` = elements of round-down at its start, which the family's widest input load needs) and the
// tile counts.
template <class Geom>
void conv_span(const VcvConvArgs& a, int BM, int BN, int slack, Geom& g) {
  const int qspan = (BN - 1) / a.P + 1;
  const int adj = a.dj < 0 ? -a.dj : a.dj;
  g.phases = conv_phases(a);
  g.JA = vcv_cdiv(a.K, g.phases);
  const int rowmax = (qspan * a.s + (g.JA - 1) * adj + 1) * a.P;
  g.xw = (rowmax + slack + 63) & ~63;
  g.ntu = vcv_cdiv(a.Q * a.P, BN);
  g.nmt = vcv_cdiv(a.Mg, BM);
}

// workgroups of a launch tiled bm x bn (one per residue of a phased launch)
inline long long conv_blocks(const VcvConvArgs& a, int bm, int bn) {
  return (long long)a.B * vcv_cdiv(a.Q * a.P, bn) * vcv_cdiv(a.Mg, bm) * conv_phases(a);
}

// (useful columns of the position tiles) x (fill of the last round of 256 workgroups)
inline double conv_round_fill(const VcvConvArgs& a, int bm, int bn) {
  const int U = a.Q * a.P;
  const long long nb = conv_blocks(a, bm, bn);
  const long long rounds = (nb + 255) / 256;
  return ((double)U / ((double)vcv_cdiv(U, bn) * bn)) * ((double)nb / (double)(rounds * 256));
}

// ... x (useful rows of the m-tiles)
inline double conv_round_fill_rows(const VcvConvArgs& a, int bm, int bn) {
  const int U = a.Q * a.P;
  const long long nb = conv_blocks(a, bm, bn);
  const long long rounds = (nb + 255) / 256;
  return ((double)U / ((double)vcv_cdiv(U, bn) * bn)) * ((double)a.Mg / ((double)vcv_cdiv(a.Mg, bm) * bm)) *
         ((double)nb / (double)(rounds * 256));
}

// 16-byte epilogue through LDS (BfGeom.vec): output rows contiguous in the column index, room for a 32 x 40 float tile per
// MFMA wave.  It bounds a column by u < Q * P alone, so every q must be an output row (Q <= Tout): with more positions than
// rows the scalar epilogue, which tests the row, takes the launch
inline int conv_vec(const VcvConvArgs& a, int mfma_waves, size_t lds_bytes) {
  return vcv_tuning().pk_vec && conv_phases(a) == 1 && a.os == 1 && a.oo == 0 && a.Q <= a.Tout && (!a.mask || a.P == 1) &&
         (size_t)mfma_waves * 32 * 40 * 4 <= lds_bytes;
}

// XCD-aware tile order (BfGeom.xcd) for `sharers` workgroups per column tile.  Nothing to share when a column tile has one
// workgroup (measured: the re-deal alone costs the 64 x 10 s decode 11 %: eight XCDs walking eight far-apart regions of the
// tensor instead of one)
inline int conv_xcd(int sharers) { return vcv_tuning().xcd_remap && sharers > 1; }

// algorithmic bytes: input once, weights once, output once (+ the fused epilogue operands); esz = bytes per activation element
inline double conv_abytes(const VcvConvArgs& a, double esz, bool count_accumulate) {
  const int streams = 1 + (a.res ? 1 : 0) + (a.oaux ? 1 : 0) + (count_accumulate && a.accumulate ? 1 : 0);
  return esz * (double)a.B * a.Cg * a.Tin * a.P + 4.0 * (double)a.Mg * a.Cg * a.K +
         esz * (double)a.B * (a.ms > 1 ? a.Mg / a.ms : a.Mg) * a.Tout * a.P * streams;
}

typedef void (*ConvFinishFn)(const VcvConvArgs, const float*, int);

// What a launcher does after its weight pack: the dynamic-LDS attribute, the profiler record, the launch of `kern` over
// (a, g, wp, last) and -- when the reduction was split (g.ks > 1: `last` is the partial-sum slabs) -- the finishing pass,
// `finish4` (16-byte) where `vec` and the output allow it, else `finish`.
// tile: the profiler tag's element kind, BM * 1000 + BN and last word;  bf16_terms: bf16 MFMA products per multiply-add (0: none)
template <class Kern, class Geom, class Wp, class Last>
int conv_launch_tail(Kern kern, const VcvConvArgs& a, const Geom& g, dim3 grid, int threads, size_t lds_bytes, hipStream_t st,
                     const int (&tile)[3], double abytes, int bf16_terms, Wp wp, Last last, ConvFinishFn finish = nullptr,
                     ConvFinishFn finish4 = nullptr, bool vec = false) {
  if (lds_bytes > 64 * 1024 &&
      hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess)
    return VCV_EHIP;
  const double flops = 2.0 * a.B * a.Mg * a.Cg * a.K * a.P * (double)(g.phases > 1 ? a.Tin : a.Q);
  const int tag[12] = {a.B, tile[0], a.Cg, a.Mg, a.K, a.Q, a.P, a.s, g.phases, a.a_mode + 10 * g.ks, tile[1], tile[2]};
  hipEvent_t ev0, ev1;
  vcv_prof_events(VCV_PROF_CONV_DMA, flops, tag, 12, &ev0, &ev1, abytes, bf16_terms * flops / VCV_PEAK_BF16_MFMA);
  VCV_LAUNCH_EV(kern, grid, dim3(threads), (unsigned)lds_bytes, st, ev0, ev1, a, g, wp, last);
  if constexpr (std::is_pointer<Last>::value) {
    if (g.ks > 1) {
      const size_t n = (size_t)a.B * a.Mg * a.Q * a.P;
      if (finish4 && vec && !a.mask && n % 4 == 0 && a.Q == a.Tout && a.Q * a.P >= 4)
        hipLaunchKernelGGL(finish4, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, st, a, (const float*)last, g.ks);
      else
        hipLaunchKernelGGL(finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, (const float*)last, g.ks);
    }
  }
  return vcv_check_launch();
}

}  // namespace
