// conv_x3.hip -- fp32 convolutions on the bf16 matrix pipe by EXACT operand splitting (vcv_conv_x3_*): the same
// forward-type / phased launch family as conv_pk.hip, same epilogue, same results to fp32 rounding.
//
// Why: v_mfma_f32_32x32x2_f32 peaks at 157 TFLOP/s; v_mfma_f32_32x32x16_bf16 at 2.5 PFLOP/s -- sixteen times the
// multiply-accumulates per cycle.  An fp32 number is the exact sum of three bf16 numbers,
//     x = x0 + x1 + x2,   x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1)
// (8 + 8 + 8 significand bits; both subtractions are exact in fp32, and bf16 has fp32's exponent range), so an fp32
// product is the sum of nine bf16 products, each of which the matrix core forms exactly and adds in fp32:
//     a * b = sum_{i, j} a_i * b_j .
// NTERM = 9 evaluates all of them: the operands enter with all 24 bits, every partial product is exact, and the fp32
// accumulator is rounded nine times per sixteen reduction elements where the fp32 MFMA chain rounds it eight times --
// the same arithmetic class as an fmaf chain, in a different summation order.  NTERM = 6 leaves out a1*b2, a2*b1 and
// a2*b2 (each below 2^-24 of |a*b|: less than the rounding of the accumulator they would be added to).  Nine bf16
// MFMAs cost 9 x 32 cycles per 16 reduction elements against 8 x 64 for fp32 MFMAs: 1.78 x the fp32 matrix peak
// (2.67 x with six terms) at the same LDS read volume per product, with the HBM / L2 traffic of an fp32 kernel.
// (The reference's own fp32 path on its native hardware runs cuDNN convolutions with TF32 inputs -- 10 significand
// bits -- by default, torch.backends.cudnn.allow_tf32; this keeps all 24.)
//
// Pipeline (one workgroup = NW MFMA waves + 4 producer waves, one output tile of BM channels x BN positions):
//   * reduction step ("stage") = one 16-channel group x the taps of one weight-ring slot.  Weights are pre-split and packed in
//     HBM in LDS image order wp[phase][m-tile][group][tap][term][h][m][8 ch] (bf16): ONE producer wave copies a tap's slab with
//     global_load_lds, 1 KiB per instruction, into a ring up to three stages ahead: 4 slots of one or two taps (2 for the
//     256-row tile), or 2 .. 4 slots of PH taps in the merged-phase form.
//   * the input span of a channel group (all taps read the same span at shifted offsets) is staged by the other three
//     producer waves: 16-byte buffer loads of four consecutive positions x 8 channels per lane (range-checked descriptors:
//     zero padding, ragged tails and channel tails need no predicates), input leaky-ReLU, split into three bf16 terms, three
//     16-byte LDS writes per position; the loads of the task a wave converts in stage s + 1 are in flight during stage s (the
//     producers pass the barrier with `s_waitcnt lgkmcnt(0)` only).  Two span buffers: group g + 1 is staged during group g.
//   * MFMA waves: per tap TM x 3 + TN x 3 `ds_read_b128` fragment reads feed TM x TN x NTERM MFMAs, interleaved over
//     the wave's accumulator tiles so that consecutive MFMAs are independent; one barrier per stage.
//   * phased launches (strided data gradients, transposed-conv forwards) of 2 or 3 output residues take conv_x3_merged_kernel,
//     one workgroup for ALL residues (x3_merge_phases; more residues, and launches too small to fill the chip, do not).
#include <type_traits>

#include "common.h"
#include "prof.h"
#include "conv_tile.h"
#include "conv_plan.h"
#include "split_terms.h"

namespace {

typedef __attribute__((address_space(3))) void* lds_ptr;

// diagnostic build only (-DVCV_X3_STAMPS, tools/probes/x3_stamps.py): 100 MHz stamps of workgroup phases; the product build
// executes none of this
#ifdef VCV_X3_STAMPS
__device__ unsigned long long* g_x3_stamps;
#define VCV_X3_STAMP(k)                                                                                          \
  do {                                                                                                          \
    if (g_x3_stamps && lane == 0)                                                                               \
      g_x3_stamps[((size_t)(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z))) * 8 + (k)] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)
#else
#define VCV_X3_STAMP(k)
#endif

constexpr int NPROD = 4;  // producer waves: 1 weight-DMA wave + 3 input-staging waves
constexpr int NXW = 3;
constexpr int MAXT = 2;   // pipelined staging tasks per input wave and stage
constexpr int NRING_DEF = 4;  // weight-slab ring slots (a power of two: conv_x3_kernel masks the slot index; the 256-row tile takes 2)

// ---- weight pack: fp32 w -> split bf16 slabs wp[phase][m-tile][group][j][term][h][m][8] -----------------------------
// mode 0: w is [M, C, K] (forward);  mode 1: w is [C, M, K], A(m, c, j) = w[c, m, K-1-j] (stride-1 data gradient);
// mode 2: w is [C, M, K], residue r = phase keeps taps k = r + j*phases (ConvTranspose forward / strided dgrad)
__global__ void __launch_bounds__(256)
pack_x3_kernel(const float* __restrict__ w, bf16x8* __restrict__ wp, int M, int C, int K, int BM, int JA, int ngr, int nmt,
               int phases, int mode, size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  size_t t = i;
  const int ml = (int)(t % BM); t /= BM;
  const int hh = (int)(t & 1); t >>= 1;
  const int j = (int)(t % JA); t /= JA;
  const int g = (int)(t % ngr); t /= ngr;
  const int mt = (int)(t % nmt); t /= nmt;
  const int r = (int)t;
  const int m = mt * BM + ml;
  const int c0 = g * 16 + hh * 8;
  bf16x8 v0, v1, v2;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int c = c0 + e;
    float f = 0.f;
    if (m < M && c < C) {
      if (mode == 0) { if (j < K) f = w[((size_t)m * C + c) * K + j]; }
      else if (mode == 1) { if (j < K) f = w[((size_t)c * M + m) * K + (K - 1 - j)]; }
      else { const int k = r + j * phases; if (k < K) f = w[((size_t)c * M + m) * K + k]; }
    }
    __bf16 a, b, d;
    split3(f, a, b, d);
    v0[e] = a, v1[e] = b, v2[e] = d;
  }
  // slab (r, mt, g, j): [term][h][m][8]
  const size_t slab = (((size_t)r * nmt + mt) * ngr + g) * JA + j;
  bf16x8* o = wp + slab * (size_t)(3 * 2 * BM) + (size_t)hh * BM + ml;
  o[0] = v0;
  o[(size_t)2 * BM] = v1;
  o[(size_t)4 * BM] = v2;
}

__device__ __forceinline__ void barrier_lds() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// The body of an input staging wave (xi = 0 .. NXW - 1) of a workgroup whose reduction runs S stages, NSG per channel group,
// over the groups g_begin .. g_end - 1: one barrier after the prologue, one per stage.
template <bool LEAKY>
__device__ __forceinline__ void x3_stage_inputs(const VcvConvArgs& p, const BfGeom& tg, char* Xbuf, int xi, int lane, int b, int f0,
                                                int g_begin, int g_end, int NSG, int S) {
  const int XW = tg.xw, P = p.P, Cg = p.Cg;
  // ---- input staging waves.  A task = (half h of the 16-channel group, block of 256 positions): 8 channels x 4
  // consecutive positions per lane.  Wave xi owns tasks xi, xi + 3, ...; local task i of group g + 1 is converted in
  // stage (g, i mod NSG), and its loads are issued at the START of the stage before (two register sets), so they have a
  // whole stage to arrive.
  const int npb = (XW + 255) >> 8;
  const int ntask = 2 * npb;
  const int nt_w = ntask > xi ? (ntask - xi + NXW - 1) / NXW : 0;  // tasks of this wave per group
  const long long TinP = (long long)p.Tin * P;
  const float* xb = p.x + (size_t)b * Cg * (size_t)TinP;
  f32x4 xr[2][MAXT][8];
  auto loadT = [&](int g, int i, f32x4 (&dst)[8]) __attribute__((always_inline)) {
    const int task = xi + NXW * i;
    const int hh = task & 1, pb = task >> 1;
    unsigned voff = (unsigned)(f0 + pb * 256 + 4 * lane) * 4u;  // negative -> wraps -> out of range -> 0
    asm volatile("" : "+v"(voff));  // one register (see conv_pk.hip: immediate-offset folding of negative offsets)
    const int c0 = g * 16 + hh * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = c0 + e;
      const unsigned rec = c < Cg ? (unsigned)(TinP * 4) : 0u;
      __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(xb + (size_t)c * (size_t)TinP), 0, (int)rec, 0x00020000);
      dst[e] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, 0, 0));
    }
  };
  auto storeT = [&](int i, const f32x4 (&src)[8], int buf) __attribute__((always_inline)) {
    const int task = xi + NXW * i;
    const int hh = task & 1, pb = task >> 1;
    const int pos = pb * 256 + 4 * lane;
    if (pos >= XW) return;  // (XW is a multiple of 64: the four positions of a lane are inside or outside together)
    char* base = Xbuf + buf * tg.buf_bytes + ((size_t)hh * XW + pos) * 16;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      bf16x8 v0, v1, v2;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float f = src[e][jj];
        if (LEAKY) f = fmaxf(f, f * p.slope);  // slope in [0, 1)
        __bf16 a, bq, d;
        split3(f, a, bq, d);
        v0[e] = a, v1[e] = bq, v2[e] = d;
      }
      *reinterpret_cast<bf16x8*>(base + (size_t)jj * 16) = v0;
      *reinterpret_cast<bf16x8*>(base + ((size_t)2 * XW + jj) * 16) = v1;
      *reinterpret_cast<bf16x8*>(base + ((size_t)4 * XW + jj) * 16) = v2;
    }
  };
  // loads of the tasks converted in stage (g, j) -- they belong to group g + 1 -- into register set `par`
  auto load_stage = [&](auto par, int g, int j) __attribute__((always_inline)) {
    constexpr int PAR = decltype(par)::value;
    if (g + 1 >= g_end) return;
#pragma unroll
    for (int q = 0; q < MAXT; ++q)
      if (j + q * NSG < nt_w) loadT(g + 1, j + q * NSG, xr[PAR][q]);
  };
  auto store_stage = [&](auto par, int g, int j) __attribute__((always_inline)) {
    constexpr int PAR = decltype(par)::value;
    if (g + 1 >= g_end) return;
    const int nb = (g + 1 - g_begin) & 1;
#pragma unroll
    for (int q = 0; q < MAXT; ++q)
      if (j + q * NSG < nt_w) storeT(j + q * NSG, xr[PAR][q], nb);
    // (more tasks per stage than the pipelined slots hold: load and convert on the spot)
    for (int i = j + MAXT * NSG; i < nt_w; i += NSG) {
      loadT(g + 1, i, xr[PAR][0]);
      storeT(i, xr[PAR][0], nb);
    }
  };
  typedef std::integral_constant<int, 0> P0;
  typedef std::integral_constant<int, 1> P1;
  // prologue: the whole span of the first group, then the loads of stage 0's tasks
  for (int i = 0; i < nt_w; ++i) {
    loadT(g_begin, i, xr[0][0]);
    storeT(i, xr[0][0], 0);
  }
  int g = g_begin, j = 0;
  load_stage(P0(), g, j);
  if (xi == 0) VCV_X3_STAMP(6);
  barrier_lds();
  for (int s = 0; s < S; s += 2) {
    {  // even stage: its tasks sit in set 0; the next stage's loads go to set 1
      int g2 = g, j2 = j + 1;
      if (j2 == NSG) j2 = 0, ++g2;
      if (s + 1 < S) load_stage(P1(), g2, j2);
      store_stage(P0(), g, j);
      g = g2, j = j2;
      barrier_lds();
    }
    if (s + 1 < S) {  // odd stage
      int g2 = g, j2 = j + 1;
      if (j2 == NSG) j2 = 0, ++g2;
      if (s + 2 < S) load_stage(P0(), g2, j2);
      store_stage(P1(), g, j);
      g = g2, j = j2;
      barrier_lds();
    }
  }
}

// BfGeom fields as used here: nch = channel groups of 16, a_bytes = one weight slab (3 * 2 * BM * 16), buf_bytes = one
// span buffer (3 * 2 * xw * 16), JA / phases / ks / vec / ntu / nmt / xw as in conv_pk.hip; BKC = 16, ncg = 1.
// JS: taps per stage (1 or 2).  Two taps double the MFMA work between barriers (the 2 x 1-tile waves of the 128 x 128 tile
// have only 12 MFMAs per tap) at twice the weight-ring footprint; a group's last stage may hold one tap.
template <int NTERM, int TM, int TN, int WM, int WN, bool LEAKY, int NRING = NRING_DEF, int JS = 1>
__global__ void __launch_bounds__(64 * (WM * WN + NPROD))
conv_x3_kernel(const VcvConvArgs p, const BfGeom tg, const char* __restrict__ wp, float* __restrict__ part) {
  constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN, NW = WM * WN;
  constexpr int TAPB = 3 * 2 * BM * 16;  // bytes of one tap of a weight slab
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, h = lane >> 5;

  int bxk, mt, r;  // (column-tile, split) index, m-tile, output residue of a phased launch (0 otherwise)
  xcd_tile_id(bxk, mt, r, tg.xcd);
  const int kz = bxk % tg.ks;
  const int bx = bxk / tg.ks;
  const int b = bx / tg.ntu, ut = bx % tg.ntu;
  const int JA = tg.JA, P = p.P, U = p.Q * P, Cg = p.Cg;
  const int K = tg.phases > 1 ? (r < p.K ? (p.K - r + tg.phases - 1) / tg.phases : 0) : p.K;
  const int oo = p.oo + (tg.phases > 1 ? r : 0);
  const int u0 = ut * BN, m0 = mt * BM;
  const int qa = u0 / P;
  const int jspan = (JA - 1) * p.dj;
  const int jmin = jspan < 0 ? jspan : 0;
  const int f0r = (qa * p.s + p.off + jmin) * P;  // first input position the tile reads (flattened [row][P]); may be < 0
  const int f0 = f0r & ~3;                        // the image starts at a multiple of four floats of the channel row
  const int fsh = f0r - f0;
  const int XW = tg.xw;

  const int g_begin = (int)((long long)kz * tg.nch / tg.ks), g_end = (int)((long long)(kz + 1) * tg.nch / tg.ks);
  const int NSG = (K + JS - 1) / JS;      // stages per channel group
  const int S = (g_end - g_begin) * NSG;  // stages
  char* const Aring = smem;
  char* const Xbuf = smem + NRING * tg.a_bytes;

  if (wave >= NW) {
    // ================================================================================================ producers
    __builtin_amdgcn_s_setprio(3);
    if (S <= 0) return;
    const int pw = wave - NW;
    if (pw == 0) {
      VCV_X3_STAMP(4);
      // ---- weight DMA wave: the slab of stage s + NRING - 1 is issued while stage s is multiplied (NRING-slot ring); it
      // passes the barrier of stage s as soon as the slab of stage s + 1 has landed, with later slabs still in flight
      const char* wtile = wp + ((size_t)r * gridDim.y + mt) * (size_t)tg.nch * JA * TAPB;
      constexpr int nT = TAPB >> 10;  // 1 KiB wave-instructions per tap
      constexpr int nA = JS * nT;     // ... per slab: ALWAYS issued in full, so that the in-flight accounting below holds
      auto issue = [&](int g, int sj, int slot) {
        const int j0 = sj * JS;
        char* dst = Aring + slot * tg.a_bytes;
#pragma unroll
        for (int jj = 0; jj < JS; ++jj) {
          const int j = j0 + jj < K ? j0 + jj : j0;  // (a group's odd last tap: its partner slot re-loads the same tap, unread)
          const char* slab = wtile + ((size_t)g * JA + j) * TAPB;
#pragma unroll
          for (int i = 0; i < nT; ++i)
            __builtin_amdgcn_global_load_lds((const void*)(slab + i * 1024 + lane * 16), (lds_ptr)(dst + jj * TAPB + i * 1024), 16, 0, 0);
        }
      };
      int gn = g_begin, jn = 0, issued = 0;
      for (; issued < NRING - 1 && issued < S; ++issued) {
        issue(gn, jn, issued);
        if (++jn == NSG) jn = 0, ++gn;
      }
      // (prologue barrier: slab 0 must be there)
      if (issued >= 3) wait_vm<2 * nA>(); else if (issued == 2) wait_vm<nA>(); else wait_vm<0>();
      asm volatile("s_barrier" ::: "memory");
      for (int s = 0; s < S; ++s) {
        if (issued < S) {
          issue(gn, jn, issued & (NRING - 1));
          if (++jn == NSG) jn = 0, ++gn;
          ++issued;
        }
        // slabs <= s + 1 complete; `issued - (s + 2)` later ones may stay in flight
        const int fly = issued - (s + 2);
        if (fly >= 2) wait_vm<2 * nA>(); else if (fly == 1) wait_vm<nA>(); else wait_vm<0>();
        asm volatile("s_barrier" ::: "memory");
      }
      VCV_X3_STAMP(5);
      return;
    }
    x3_stage_inputs<LEAKY>(p, tg, Xbuf, pw - 1, lane, b, f0, g_begin, g_end, NSG, S);
    return;
  }

  // ==================================================================================================== MFMA waves
  if (wave == 0) VCV_X3_STAMP(0);
  const int wm = wave / WN, wn = wave % WN;
  int laneoff[TN];
#pragma unroll
  for (int tn = 0; tn < TN; ++tn) {
    int u = u0 + (wn * TN + tn) * 32 + l31;
    if (u > U - 1) u = U - 1;
    const int q = u / P, pc = u - q * P;
    laneoff[tn] = (((q - qa) * p.s - jmin) * P + pc + fsh + h * XW) * 16;  // byte offset in a span buffer (h plane included)
  }
  f32x16 acc[TM][TN];
#pragma unroll
  for (int tm = 0; tm < TM; ++tm)
#pragma unroll
    for (int tn = 0; tn < TN; ++tn)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[tm][tn][e] = 0.f;

  if (S > 0) {
    __syncthreads();
    if (wave == 0) VCV_X3_STAMP(1);
    const int aoff = (h * BM + wm * TM * 32 + l31) * 16;
    int g = g_begin, sj = 0;
    for (int s = 0; s < S; ++s) {
      const char* As0 = Aring + (s & (NRING - 1)) * tg.a_bytes + aoff;
      const int j0 = sj * JS;
#pragma unroll
      for (int jj = 0; jj < JS; ++jj) {
        if (j0 + jj < K) {
          const char* As = As0 + jj * TAPB;
          const char* Xs = Xbuf + ((g - g_begin) & 1) * tg.buf_bytes + (j0 + jj) * p.dj * P * 16;
          bf16x8 a[TM][3], bb[TN][3];
#pragma unroll
          for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
              a[tm][pl] = *reinterpret_cast<const bf16x8*>(As + ((size_t)pl * 2 * BM + tm * 32) * 16);
#pragma unroll
          for (int tn = 0; tn < TN; ++tn)
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
              bb[tn][pl] = *reinterpret_cast<const bf16x8*>(Xs + laneoff[tn] + (size_t)pl * 2 * XW * 16);
          mma_product<NTERM>(acc, a, bb);
        }
      }
      if (++sj == NSG) sj = 0, ++g;
      __syncthreads();  // publishes stage s + 1 (LDS writes + the weight DMA) and retires the reads of stage s
    }
  }
  if (wave == 0) VCV_X3_STAMP(2);
  conv_tile_epilogue<TM, TN>(p, tg, acc, smem, part, wave, wm, wn, lane, b, kz, u0, m0, oo, BM);
  if (wave == 0) VCV_X3_STAMP(3);
}

// ---- merged-phase form of a phased launch (PH = 2 or 3 output residues) --------------------------------------------------
// The residues of a phased launch read the SAME input span at the same tap offsets; only the weight slab differs (residue r
// keeps the taps k = r + j * PH).  In the kernel above each residue is a workgroup of its own (gridDim.z), so a span is staged
// and split PH times and multiplied by one or two taps each time.  Here ONE workgroup owns the (column tile, m-tile) for all
// residues: the staging waves stage each channel group once, an MFMA wave holds one accumulator set per residue, and a stage
// is one (group, tap j) for every residue that has the tap -- the span fragments of tap j are read once and multiplied by up
// to PH weight slabs (ring slot = PH taps; residues r >= nres(j) = min(PH, K - j * PH) have no tap j: nothing is loaded or
// multiplied for them, and a residue without any tap stores its epilogue over zeros).  Per output element the additions are
// those of the per-residue launch in the same order (groups outer, taps inner, small terms first): the results are
// bit-identical.  The weight pack is the one the per-residue launch reads, wp[phase][m-tile][group][tap].
template <int nT>
__device__ __forceinline__ void wait_vm_taps(int k) {
  // at most k taps (nT load instructions each) stay in flight; vmcnt has six bits, and a lower count only waits longer
  constexpr int CAP = 63 / nT;
  switch (k) {
    case 0: wait_vm<0>(); break;
    case 1: wait_vm<nT>(); break;
    case 2: wait_vm<(2 < CAP ? 2 : CAP) * nT>(); break;
    case 3: wait_vm<(3 < CAP ? 3 : CAP) * nT>(); break;
    case 4: wait_vm<(4 < CAP ? 4 : CAP) * nT>(); break;
    case 5: wait_vm<(5 < CAP ? 5 : CAP) * nT>(); break;
    default: wait_vm<(6 < CAP ? 6 : CAP) * nT>(); break;
  }
}

template <int NTERM, int PH, int TM, int TN, int WM, int WN, bool LEAKY>
__global__ void __launch_bounds__(64 * (WM * WN + NPROD))
conv_x3_merged_kernel(const VcvConvArgs p, const BfGeom tg, const char* __restrict__ wp, const int nring) {
  constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN, NW = WM * WN;
  constexpr int TAPB = 3 * 2 * BM * 16;  // bytes of one tap of a weight slab; a ring slot (tg.a_bytes) holds PH of them
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, h = lane >> 5;

  int bx, mt, rz;  // column tile, m-tile (gridDim.z == 1: rz is 0)
  xcd_tile_id(bx, mt, rz, tg.xcd);
  const int b = bx / tg.ntu, ut = bx % tg.ntu;
  const int JA = tg.JA, P = p.P, U = p.Q * P;
  const int u0 = ut * BN, m0 = mt * BM;
  const int qa = u0 / P;
  const int jspan = (JA - 1) * p.dj;
  const int jmin = jspan < 0 ? jspan : 0;
  const int f0r = (qa * p.s + p.off + jmin) * P;
  const int f0 = f0r & ~3;
  const int fsh = f0r - f0;
  const int XW = tg.xw;
  const int S = tg.nch * JA;  // stages: (group, tap)
  char* const Aring = smem;
  char* const Xbuf = smem + nring * tg.a_bytes;

  if (wave >= NW) {
    // ================================================================================================ producers
    __builtin_amdgcn_s_setprio(3);
    const int pw = wave - NW;
    if (pw == 0) {
      // ---- weight DMA wave: as above, the slab of stage s + nring - 1 is issued while stage s is multiplied.  A slab has
      // nres(j) taps, so the in-flight accounting counts taps: n1 / n2 are the taps of the last / last-but-one slab issued
      const char* wtile = wp + (size_t)mt * tg.nch * JA * TAPB;
      const size_t rstride = (size_t)gridDim.y * tg.nch * JA * TAPB;  // residue r + 1 of the pack
      constexpr int nT = TAPB >> 10;  // 1 KiB wave-instructions per tap
      auto issue = [&](int g, int j, int slot) {
        const int nres = p.K - j * PH < PH ? p.K - j * PH : PH;
        const char* slab = wtile + ((size_t)g * JA + j) * TAPB + lane * 16;
        char* dst = Aring + slot * tg.a_bytes;
#pragma unroll
        for (int r = 0; r < PH; ++r) {
          if (r < nres) {
#pragma unroll
            for (int i = 0; i < nT; ++i)
              __builtin_amdgcn_global_load_lds((const void*)(slab + r * rstride + i * 1024), (lds_ptr)(dst + r * TAPB + i * 1024), 16, 0, 0);
          }
        }
        return nres;
      };
      int gn = 0, jn = 0, issued = 0, slot = 0, n1 = 0, n2 = 0;
      for (; issued < nring - 1 && issued < S; ++issued) {
        n2 = n1, n1 = issue(gn, jn, slot);
        if (++jn == JA) jn = 0, ++gn;
        if (++slot == nring) slot = 0;
      }
      // (prologue barrier: slab 0 must be there; the ring has at most four slots)
      wait_vm_taps<nT>(issued >= 3 ? n1 + n2 : issued == 2 ? n1 : 0);
      asm volatile("s_barrier" ::: "memory");
      for (int s = 0; s < S; ++s) {
        if (issued < S) {
          n2 = n1, n1 = issue(gn, jn, slot);
          if (++jn == JA) jn = 0, ++gn;
          if (++slot == nring) slot = 0;
          ++issued;
        }
        // slabs <= s + 1 complete; `issued - (s + 2)` later ones may stay in flight
        const int fly = issued - (s + 2);
        wait_vm_taps<nT>(fly >= 2 ? n1 + n2 : fly == 1 ? n1 : 0);
        asm volatile("s_barrier" ::: "memory");
      }
      return;
    }
    x3_stage_inputs<LEAKY>(p, tg, Xbuf, pw - 1, lane, b, f0, 0, tg.nch, JA, S);
    return;
  }

  // ==================================================================================================== MFMA waves
  const int wm = wave / WN, wn = wave % WN;
  int laneoff[TN];
#pragma unroll
  for (int tn = 0; tn < TN; ++tn) {
    int u = u0 + (wn * TN + tn) * 32 + l31;
    if (u > U - 1) u = U - 1;
    const int q = u / P, pc = u - q * P;
    laneoff[tn] = (((q - qa) * p.s - jmin) * P + pc + fsh + h * XW) * 16;
  }
  f32x16 acc[PH][TM][TN];
#pragma unroll
  for (int r = 0; r < PH; ++r)
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
      for (int tn = 0; tn < TN; ++tn)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[r][tm][tn][e] = 0.f;

  __syncthreads();
  {
    const int aoff = (h * BM + wm * TM * 32 + l31) * 16;
    int g = 0, j = 0, slot = 0;
    for (int s = 0; s < S; ++s) {
      const char* As0 = Aring + slot * tg.a_bytes + aoff;
      const char* Xs = Xbuf + (g & 1) * tg.buf_bytes + j * p.dj * P * 16;
      const int nres = p.K - j * PH < PH ? p.K - j * PH : PH;
      bf16x8 bb[TN][3];
#pragma unroll
      for (int tn = 0; tn < TN; ++tn)
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
          bb[tn][pl] = *reinterpret_cast<const bf16x8*>(Xs + laneoff[tn] + (size_t)pl * 2 * XW * 16);
      // (literal residue indices: a loop the compiler leaves rolled would index the accumulator sets at run time)
      auto residue = [&](auto rc) __attribute__((always_inline)) {
        constexpr int r = decltype(rc)::value;
        if (r < nres) {
          bf16x8 a[TM][3];
#pragma unroll
          for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
              a[tm][pl] = *reinterpret_cast<const bf16x8*>(As0 + r * TAPB + ((size_t)pl * 2 * BM + tm * 32) * 16);
          mma_product<NTERM>(acc[r], a, bb);
        }
      };
      residue(std::integral_constant<int, 0>());
      residue(std::integral_constant<int, 1>());
      if constexpr (PH > 2) residue(std::integral_constant<int, 2>());
      if (++j == JA) j = 0, ++g;
      if (++slot == nring) slot = 0;
      __syncthreads();  // publishes stage s + 1 and retires the reads of stage s
    }
  }
  // one epilogue pass per residue (output row q * os + oo + r); the shared epilogue takes its scalar path (vec = 0, ks = 1)
  conv_tile_epilogue<TM, TN>(p, tg, acc[0], smem, nullptr, wave, wm, wn, lane, b, 0, u0, m0, p.oo, BM);
  conv_tile_epilogue<TM, TN>(p, tg, acc[1], smem, nullptr, wave, wm, wn, lane, b, 0, u0, m0, p.oo + 1, BM);
  if constexpr (PH > 2) conv_tile_epilogue<TM, TN>(p, tg, acc[2], smem, nullptr, wave, wm, wn, lane, b, 0, u0, m0, p.oo + 2, BM);
}

struct Plan {
  int variant, js;
  int merged, nring;  // merged-phase form (conv_x3_merged_kernel) and its weight-ring slots
  int BM, BN, NW;
  BfGeom g;
  size_t scratch_floats, pack_bytes, lds_bytes;
};

bool eligible(const VcvConvArgs& a) { return conv_eligible(a, true); }

bool make_plan(const VcvConvArgs& a, int BM, int BN, int NW, Plan& pl, int nring = NRING_DEF, int js = 1) {
  pl.BM = BM; pl.BN = BN; pl.NW = NW;
  pl.merged = 0; pl.nring = nring;
  BfGeom& g = pl.g;
  conv_span(a, BM, BN, 3, g);  // (up to three floats of round-down at the start)
  g.BKC = 16;
  g.ncg = 1;
  g.nch = vcv_cdiv(a.Cg, 16);
  g.a_bytes = js * 3 * 2 * BM * 16;  // the weight slab of a stage (js taps)
  pl.js = js;
  g.buf_bytes = 3 * 2 * g.xw * 16;
  pl.lds_bytes = (size_t)nring * g.a_bytes + 2ull * g.buf_bytes;
  if (pl.lds_bytes > VCV_LDS_LIMIT) return false;
  g.ks = 1;
  g.vec = 0;
  g.xcd = conv_xcd(g.nmt * g.phases);
  pl.pack_bytes = (size_t)g.phases * g.nmt * g.nch * g.JA * (3 * 2 * BM * 16);
  pl.scratch_floats = 0;
  return true;
}

// The merged-phase form of a phased launch: the geometry of make_plan with a ring slot of `phases` taps and the deepest ring
// (4, 3 or 2 slots) the LDS holds next to the two span buffers; the grid has no phase dimension.
bool make_plan_merged(const VcvConvArgs& a, int BM, int BN, int variant, Plan& pl) {
  if (!make_plan(a, BM, BN, 8, pl, 0, 1)) return false;
  BfGeom& g = pl.g;
  g.a_bytes *= g.phases;
  int nring = 4;
  while (nring >= 2 && (size_t)nring * g.a_bytes + 2ull * g.buf_bytes > VCV_LDS_LIMIT) --nring;
  if (nring < 2) return false;
  pl.lds_bytes = (size_t)nring * g.a_bytes + 2ull * g.buf_bytes;
  pl.merged = 1, pl.nring = nring, pl.variant = variant;
  g.xcd = conv_xcd(g.nmt);  // (the workgroups sharing a span are the m-tiles alone)
  return true;
}

// The tile variants (8 MFMA waves each): X(variant, TM, TN, WM, WN, ring slots, two-tap stages exist, merged form exists) gives
// the forced geometry, every plan's tile, the merged mapping and the dispatch; run_n instantiates the kernels in row order.
#define X3_VARIANTS(X)                              \
  X(0, 2, 2, 2, 4, NRING_DEF, 1, 0) /* 128 x 256 */ \
  X(1, 2, 1, 2, 4, NRING_DEF, 1, 1) /* 128 x 128 */ \
  X(2, 2, 2, 4, 2, 2, 0, 0)         /* 256 x 128 */ \
  X(3, 1, 2, 2, 4, NRING_DEF, 0, 1) /*  64 x 256 */ \
  X(4, 1, 1, 2, 4, NRING_DEF, 0, 0) /*  64 x 128 */ \
  X(6, 1, 4, 2, 4, NRING_DEF, 0, 0) /*  64 x 512 */ \
  X(5, 1, 1, 1, 8, NRING_DEF, 0, 1) /*  32 x 256 */
struct Variant { int BM, BN, NW, nring, js2, merged; };
#define X3_ROW(V, TM, TN, WM, WN, NRING, JS2, MRG) v == V ? Variant{32 * TM * WM, 32 * TN * WN, WM * WN, NRING, JS2, MRG} :
constexpr Variant variant(int v) { return X3_VARIANTS(X3_ROW) Variant{}; }  // (BM = 0: no such variant)
#undef X3_ROW

bool plan_variant(const VcvConvArgs& a, int v, Plan& pl, int js = 1) {
  pl.variant = v;
  return make_plan(a, variant(v).BM, variant(v).BN, variant(v).NW, pl, variant(v).nring, js);
}
int g_force_js = -1, g_force_ks = -1;

bool choose(const VcvConvArgs& a, Plan& pl) {
  const int U = a.Q * a.P;
  if (U < 96) return false;
  // tools/x3_variant_sweep.py: one fixed tile shape for every launch that can take it
  if (const int v = vcv_tuning().x3_variant; v >= 0) {
    if (!variant(v).BM || a.Mg < (variant(v).BM == 32 ? 32 : variant(v).BM / 2 + 1)) return false;
    const int js = (g_force_js == 2 && variant(v).js2 && vcv_cdiv(a.K, conv_phases(a)) >= 2) ? 2 : 1;
    if (!plan_variant(a, v, pl, js)) return false;
    if (g_force_ks >= 2 && conv_phases(a) == 1 && pl.g.nch >= 2 * g_force_ks) {
      pl.g.ks = g_force_ks;
      pl.scratch_floats = (size_t)g_force_ks * a.B * a.Mg * U;
    }
    pl.g.vec = conv_vec(a, pl.NW, pl.lds_bytes);
    return true;
  }
  const int nph = conv_phases(a);
  // Phased launches of 2 or 3 residues: one workgroup per (column tile, m-tile) computes every residue from one staged span
  // (conv_x3_merged_kernel).  Three accumulator sets fit the register file for 2 x 1, 1 x 2 and 1 x 1 wave tiles, so the rows
  // follow Mg as below and the columns are what those wave tiles leave.  The merged grid is 1 / phases of the per-residue one
  // with workgroups that run all K taps per group instead of ceil(K / phases): where even the per-residue grid is no more
  // than one round of 256 workgroups, that form finishes sooner (every tap in parallel) and keeps the launch.
  if (vcv_tuning().x3_merge_phases && (nph == 2 || nph == 3)) {
    const int v = a.Mg >= 96 ? 1 : a.Mg >= 48 ? 3 : 5;  // 128 x 128, 64 x 256, 32 x 256
    const long long nbm = (long long)a.B * vcv_cdiv(U, variant(v).BN) * vcv_cdiv(a.Mg, variant(v).BM);
    if ((vcv_tuning().x3_all || nbm * nph > 256) && make_plan_merged(a, variant(v).BM, variant(v).BN, v, pl)) return true;
  }
  auto blocks = [&](int bm, int bn) { return conv_blocks(a, bm, bn); };
  auto eff = [&](int bm, int bn) { return conv_round_fill_rows(a, bm, bn); };
  bool ok = false;
  if (a.Mg >= 96) {
    const double e256 = U > 160 ? eff(128, 256) : 0.0, e128 = eff(128, 128);
    if (e256 >= e128 - 0.02 && e256 > 0.0 && plan_variant(a, 0, pl)) ok = true;
    // 128 columns (the strided layers, whose input span is stride x as long, do not fit 256): 256 rows x 128 columns keeps
    // the 2 x 2 accumulator tiles per wave (12 fragment reads per 24 MFMAs instead of 9 per 12) with a two-slot ring
    else if (a.Mg >= 256 && eff(256, 128) >= e128 - 0.1 && plan_variant(a, 2, pl)) ok = true;
    else if (plan_variant(a, 1, pl)) ok = true;
  } else if (a.Mg >= 48) {
    // 64 x 512 (8 waves of 1 x 4 tiles: 15 fragment reads per 24 MFMAs instead of 9 per 12) where 64 x 256 needs more than one
    // round of 256 workgroups and the wider tile still fills the chip: the generator's 64-channel layers ran two full
    // rounds, each with its own 4 us prologue and 6 us store burst (tools/probes/x3_stamps.py)
    const bool no_v6 = !vcv_tuning().x3_v6;
    if (!no_v6 && nph == 1 && blocks(64, 256) > 256 && blocks(64, 512) >= 192 && eff(64, 512) >= eff(64, 256) - 0.02 &&
        plan_variant(a, 6, pl)) ok = true;
    else if (U > 160 && eff(64, 256) >= eff(64, 128) - 0.02 && plan_variant(a, 3, pl)) ok = true;
    else if (plan_variant(a, 4, pl)) ok = true;
  } else {
    if (plan_variant(a, 5, pl)) ok = true;
  }
  if (!ok) return false;
  // two taps per stage where the doubled weight ring fits (128-row tiles, K >= 2): half the barriers per MFMA
  const bool no_js2 = !vcv_tuning().x3_js2;
  if (!no_js2 && variant(pl.variant).js2 && vcv_cdiv(a.K, nph) >= 2) {
    Plan p2;
    if (plan_variant(a, pl.variant, p2, 2)) pl = p2;
  }
  // too few tiles for 256 CUs: split the channel groups over ks workgroups per tile (deterministic slabs + finishing pass)
  const long long nb = blocks(pl.BM, pl.BN);
  if (nph == 1 && nb < 192 && pl.g.nch >= 4) {
    // the split that costs the fewest (rounds of 256 workgroups) x (channel groups per workgroup): rounding to the nearest
    // count put 288 and 260 workgroups -- a second round for 32 and for 4 of them -- on two of DiscriminatorS's last layers
    long long ks = 1, best = (long long)1 << 60;
    const bool old_ks = vcv_tuning().x3_old_ks != 0;
    for (long long c = 2; c <= pl.g.nch / 2; ++c) {
      // (+ 3: a workgroup's prologue and epilogue cost about three channel groups of a 128-row tile; + c: the finishing pass reads c slabs)
      const long long cost = ((nb * c + 255) / 256) * ((pl.g.nch + c - 1) / c + 3) * 64 + c;
      if (cost < best) best = cost, ks = c;
    }
    if (old_ks) ks = (256 + nb / 2) / nb;
    if (ks > pl.g.nch / 2) ks = pl.g.nch / 2;
    if (ks >= 2) {
      pl.g.ks = (int)ks;
      pl.scratch_floats = (size_t)ks * a.B * a.Mg * U;
    }
  }
  pl.g.vec = conv_vec(a, pl.NW, pl.lds_bytes);
  return true;
}

// default: six product terms.  Measured against float64 on the layer shapes of both configs (tests/test_conv_x3_gpu.py,
// profiles/r3_x3_vs_f64.txt) the six- and nine-term results have the same error to three digits, 2e-7 .. 1e-6 of the
// output scale -- the error of the fp32 accumulation order, as large for the fp32-input MFMA kernel -- because each left
// out term is below 2^-24 of its product while one accumulator rounding is 2^-24 of the whole running sum.

// The weight pack (unless the caller's is valid) and the launch of `kern` (BM rows per tile, NT threads) over the plan's grid;
// last: the partial-sum slabs of a split launch, or the merged-phase kernel's ring depth (its grid has no phase dimension).
template <int NTERM, int BM, int NT, class Kern, class Last>
int pack_and_launch(Kern kern, const VcvConvArgs& a, const Plan& pl, char* wp, Last last, int flip, bool pack_valid, hipStream_t st,
                    int32_t* desc) {
  if (desc) { desc[3] = NT; return VCV_OK; }  // vcv_conv_plan_describe: the instantiation this launch would run
  const BfGeom& g = pl.g;
  if (!pack_valid) {
    const size_t total = (size_t)g.phases * g.nmt * g.nch * g.JA * 2 * BM;
    const int mode = g.phases > 1 ? 2 : (flip ? 1 : 0);
    hipLaunchKernelGGL(pack_x3_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a.w, (bf16x8*)wp, a.Mg, a.Cg,
                       a.K, BM, g.JA, g.nch, g.nmt, g.phases, mode, total);
  }
  // (a merged launch carries the profiler tag and flop count of the per-residue launch: one launch, counted once)
  return conv_launch_tail(kern, a, g, dim3(a.B * g.ntu * g.ks, g.nmt, pl.merged ? 1 : g.phases), NT, pl.lds_bytes, st,
                          {3, BM * 1000 + pl.BN, NTERM}, conv_abytes(a, 4.0, false), NTERM, (const char*)wp, last,
                          conv_pk_finish_kernel, conv_pk_finish4_kernel, g.vec != 0);
}

template <int NTERM, int PH, int TM, int TN, int WM, int WN, int NRING, int JS>  // PH = 0: conv_x3_kernel;  2, 3: the merged form
int launch(const VcvConvArgs& a, const Plan& pl, char* wp, float* part, int flip, bool pack_valid, hipStream_t st, int32_t* desc) {
  constexpr int BM = 32 * TM * WM, NT = 64 * (WM * WN + NPROD);
  const bool leaky = a.in_tf == VCV_TF_LEAKY;
  if constexpr (PH > 0)
    return pack_and_launch<NTERM, BM, NT>(leaky ? conv_x3_merged_kernel<NTERM, PH, TM, TN, WM, WN, true> : conv_x3_merged_kernel<NTERM, PH, TM, TN, WM, WN, false>,
                                          a, pl, wp, pl.nring, flip, pack_valid, st, desc);
  else
    return pack_and_launch<NTERM, BM, NT>(leaky ? conv_x3_kernel<NTERM, TM, TN, WM, WN, true, NRING, JS> : conv_x3_kernel<NTERM, TM, TN, WM, WN, false, NRING, JS>,
                                          a, pl, wp, part, flip, pack_valid, st, desc);
}

template <int NTERM>
int run_n(const VcvConvArgs& a, const Plan& pl, char* wp, float* part, int flip, bool pv, hipStream_t st, int32_t* desc) {
  auto pass = [&](auto ph) {  // one pass over the table per form: PH = 2, PH = 3, then per residue (PH = 0)
    constexpr int PH = decltype(ph)::value;
#define X3_RUN(V, TM, TN, WM, WN, NRING, JS2, MRG)                                                                             \
  if constexpr (PH == 0 || MRG) if (pl.variant == V) {                                                                         \
    if constexpr (PH == 0 && JS2) if (pl.js == 2) return launch<NTERM, 0, TM, TN, WM, WN, NRING, 2>(a, pl, wp, part, flip, pv, st, desc); \
    return launch<NTERM, PH, TM, TN, WM, WN, NRING, 1>(a, pl, wp, part, flip, pv, st, desc);                                   \
  }
    X3_VARIANTS(X3_RUN)
#undef X3_RUN
    return (int)VCV_EINVAL;  // (also: a merged plan on a tile without a merged form)
  };
  if (pl.merged) return pl.g.phases == 2 ? pass(std::integral_constant<int, 2>()) : pass(std::integral_constant<int, 3>());
  return pass(std::integral_constant<int, 0>());
}

}  // namespace

// Number of bf16 product terms per fp32 product: 9 (all of them: exact operands) or 6 (the three smallest left out).
extern "C" int vcv_conv_x3_set_terms(int n) {
  if (n != 6 && n != 9) return VCV_EINVAL;
  vcv_tuning().x3_terms = n;
  return VCV_OK;
}
extern "C" int vcv_conv_x3_get_terms(void) { return vcv_tuning().x3_terms; }
// all != 0: take every eligible launch (tests); 0: only the shapes where this kernel is the faster one (wanted())
extern "C" int vcv_conv_x3_set_all(int all) {
  vcv_tuning().x3_all = all ? 1 : 0;
  return VCV_OK;
}
extern "C" int vcv_conv_x3_get_all(void) { return vcv_tuning().x3_all; }
// Tuning probe (tools/x3_variant_sweep.py): fix the tile variant (0..6: 128x256, 128x128, 256x128, 64x256, 64x128, 32x256,
// 64x512; -1 = the library's choice), the taps per stage (2 or 1) and the channel-group split (>= 2, or -1) of every launch.
extern "C" int vcv_conv_x3_set_variant(int variant, int js, int ks) {
  vcv_tuning().x3_variant = variant;
  g_force_js = js;
  g_force_ks = ks;
  return VCV_OK;
}

// Same calling convention as vcv_conv_pk_plan / vcv_conv_pk_run: out[0] = size of the packed-weight buffer in 4-byte
// words, out[1] = floats of per-launch scratch, out[2] = signature of the pack layout.
// Where the split kernel is ahead of the fp32-input MFMA kernel (conv_pk.hip) in the training step
// (tools/prof_compare.py on the bench workload): everything but the 32-channel layers and the 64-channel k <= 3 layers,
// whose few reduction stages per tile leave the prologue / epilogue exposed.
static bool wanted(const VcvConvArgs& a) {
  if (vcv_tuning().x3_all) return true;
  if (a.Cg <= 32) return false;
  if (a.Cg <= 64 && a.K <= 3) return false;
  return true;
}

extern "C" int vcv_conv_x3_plan(const VcvConvArgs* args, int flip, int64_t* out) {
  if (!args || !out || !eligible(*args) || !wanted(*args)) return VCV_EINVAL;
  Plan pl;
  if (!choose(*args, pl)) return VCV_EINVAL;
  out[0] = (int64_t)((pl.pack_bytes + 3) / 4);
  out[1] = (int64_t)pl.scratch_floats;
  out[2] = ((int64_t)3 << 60) | ((int64_t)pl.BM << 40) | ((int64_t)pl.g.JA << 20) | ((int64_t)pl.g.phases << 8) | (flip ? 1 : 0);
  return 0;
}

extern "C" int vcv_conv_x3_pack_job(const VcvConvArgs* args, int flip, VcvPackJob* out) {
  if (!args || !out || !eligible(*args) || !wanted(*args)) return VCV_EINVAL;
  Plan pl;
  if (!choose(*args, pl)) return VCV_EINVAL;
  const BfGeom& g = pl.g;
  out->kind = 0;
  out->M = args->Mg, out->C = args->Cg, out->K = args->K;
  out->BM = pl.BM, out->BKC = 16, out->JA = g.JA, out->nch = g.nch, out->nmt = g.nmt, out->phases = g.phases;
  out->mode = g.phases > 1 ? 2 : (flip ? 1 : 0);
  out->total = (int64_t)g.phases * g.nmt * g.nch * g.JA * 2 * pl.BM;
  return VCV_OK;
}

static int run(const VcvConvArgs* args, float* pack_ws, float* scratch_ws, int flip, int pack_valid, void* stream, int32_t* desc) {
  if (!args || (!pack_ws && !desc) || !eligible(*args) || !wanted(*args)) return VCV_EINVAL;
  Plan pl;
  if (!choose(*args, pl)) return VCV_EINVAL;
  if (pl.g.ks > 1 && !scratch_ws && !desc) return VCV_EINVAL;
  if (desc) {
    const BfGeom& g = pl.g;
    const int32_t d[16] = {pl.variant, pl.BM, pl.BN, 0, g.BKC, g.JA, g.phases, g.nch, g.ks, g.vec, g.xcd, (int32_t)pl.lds_bytes,
                           pl.js, pl.nring, pl.merged, g.xw};
    for (int i = 0; i < 16; ++i) desc[i] = d[i];
  }
  hipStream_t st = (hipStream_t)stream;
  return vcv_tuning().x3_terms == 6 ? run_n<6>(*args, pl, (char*)pack_ws, scratch_ws, flip, pack_valid != 0, st, desc)
                      : run_n<9>(*args, pl, (char*)pack_ws, scratch_ws, flip, pack_valid != 0, st, desc);
}

extern "C" int vcv_conv_x3_run(const VcvConvArgs* args, float* pack_ws, float* scratch_ws, int flip, int pack_valid, void* stream) {
  return run(args, pack_ws, scratch_ws, flip, pack_valid, stream, nullptr);
}

// vcv_conv_plan_describe, family 3
extern "C" __attribute__((visibility("hidden"))) int vcv_conv_describe_x3(const VcvConvArgs* args, int flip, int32_t* out16) {
  return run(args, nullptr, nullptr, flip, 1, nullptr, out16);
}

#ifdef VCV_X3_STAMPS
extern "C" int vcv_x3_set_stamps(void* p) {
  unsigned long long* q = (unsigned long long*)p;
  return hipMemcpyToSymbol(HIP_SYMBOL(g_x3_stamps), &q, sizeof(q)) == hipSuccess ? 0 : 1;
}
#endif
