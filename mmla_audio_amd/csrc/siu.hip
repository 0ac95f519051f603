// SpeakerIdentification res units (speaker_identification.py:168-190), one to three of them as ONE
// kernel.  A unit without pooling (2-3, 5-6, 8-9 of the nine) is
//     y = x + Conv1D_b(ReLU(BN_mid(Conv1D_a(ReLU(BN_in(x))))))        Conv1D(C, 3, 'same')
// A workgroup stages its rows of x (BN_in + ReLU + 3xFP16 split, as conv_h3's staging), computes t1
// (GEMM a), writes it back into the same LDS already BN_mid + ReLU'd and split, and computes the
// unit's output (GEMM b) + bias + residual.  t1 never leaves the CU, and neither does the output of a
// unit that another follows in the same launch.
//
// The pool units (1, 4, 7: MaxPool1D(2, 'same') of x into BN_in, and the residual is the shortcut
// Conv1D(C, 1, strides=2) of x) run the same way with POOL: x's two source rows are max-pooled while
// staging (conv_h3's PIN) and the shortcut is a small 3xFP16 GEMM per 32-row tile (conv_h3's
// EPI_ADD_SC), so the pool unit's t1 stays on chip too.
//
// All GEMMs run as C^T = W^T X^T (weights the A operand): a lane's accumulator quad is 4 adjacent
// channels of one row, so t1 goes back to LDS as 8-B hi / lo quads and the epilogue moves float4s.
// Row -> (clip, position) by a multiply-high division (SiuArgs::tdiv_*), 32-bit offsets, the 2^4
// operand scale folded into the BatchNorm parameters, and a running range maximum: the round-6
// counters put the first version of this kernel at ~23 VALU per MFMA
// (profiles/r6_pmc_si_pipeline_summary.txt).
//
// Bit-identical to the conv_h3 pairs it replaces: the same staged operands (values and 2^4 scale:
// fma(v, 16 s, 16 t) = 16 fma(v, s, t) exactly), the same MFMA sequence per output element (channel
// chunks of 32, then taps, then k-steps, the three 3xFP16 products in conv_h3's order into one
// accumulator; the transposed product sums the same terms in the same order), the same epilogue
// arithmetic, and the same zero rows for taps that leave a clip (conv_h3's TW = 1 zero row).
#include "f16x3.h"
#include "conv.h"
#include "siu.h"

#include <type_traits>

namespace {

constexpr int CK = 32;                 // channel chunk (conv_h3's k order)
constexpr int KS = CK / 16;
constexpr int TAPS = 3;

// not f16x3.h's w_rsrc / w_frag: these descriptors also serve x (no readfirstlane, unbounded records)
MMLA_DEV __amdgpu_buffer_rsrc_t siu_rsrc(const void* p) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, (int)0xffffffff, 0x00020000);
}
MMLA_DEV float4 ld4(__amdgpu_buffer_rsrc_t r, uint32_t byte_off) {
  return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, 0));
}
MMLA_DEV f16x8 ldw(__amdgpu_buffer_rsrc_t r, int lofs, int u) {   // 16 B of a split weight
  return __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(r, (uint32_t)lofs * 2u, u * 2, 0));
}
// x / t for x < 2^31 (SiuArgs::tdiv_m, tdiv_s from siu_fastdiv)
MMLA_DEV uint32_t tdiv(uint32_t x, uint32_t m, uint32_t s) { return (__umulhi(x, m) + x) >> s; }

// v' = max(fma(v, sc', sh'), 0) (the BN already x 2^4), split into hi / lo quads; rmax tracks the
// largest v' (post-ReLU: never NaN, never negative)
MMLA_DEV void bn_split4(float4 v, float4 sc, float4 sh, f16x4& h, f16x4& l, float& rmax) {
  const float a = fmaxf(fmaf(v.x, sc.x, sh.x), 0.0f), b = fmaxf(fmaf(v.y, sc.y, sh.y), 0.0f);
  const float c = fmaxf(fmaf(v.z, sc.z, sh.z), 0.0f), d = fmaxf(fmaf(v.w, sc.w, sh.w), 0.0f);
  rmax = fmaxf(rmax, fmaxf(fmaxf(a, b), fmaxf(c, d)));
  h[0] = (_Float16)a;
  h[1] = (_Float16)b;
  h[2] = (_Float16)c;
  h[3] = (_Float16)d;
  const uint2 hu = __builtin_bit_cast(uint2, h);
  l = __builtin_bit_cast(f16x4, make_uint2(split_lo2(a, b, hu.x), split_lo2(c, d, hu.y)));
}

// the kernel's first output row per workgroup (its halo in front) and output rows: U units narrow
// the correct rows by 2 U at each end; FIN keeps both multiples of 4 (pool windows)
template <int U, bool FIN>
constexpr int chain_front() { return FIN ? (2 * U + 3) / 4 * 4 : 2 * U; }
template <int NR, int U, bool FIN>
constexpr int chain_rows() { return FIN ? (NR - chain_front<U, FIN>() - 2 * U) / 4 * 4 : NR - 4 * U; }

// A chain of res units: with POOL a pool unit p, then NU units without pooling (a, then b).  The
// launches of the SI net are a pool unit and the two units after it (1-3, 4-6, 7-9: POOL, NU 2);
// the A/B paths run two units (NU 2), one unit (NU 1) or the pool unit alone (POOL, NU 0).  Each
// unit's output stays in registers (the next unit's residual) and in LDS (BN + ReLU + split, the next
// unit's staged input), so only the chain's input and output touch HBM.  All GEMMs run over the same
// NR rows i <-> global (pooled) row rb + i (NR a multiple of the waves' 32-row MFMA tiles); each conv
// narrows the rows it computes correctly by one at each end, so the last unit's output is right for
// i in [2 U, NR - 2 U), U = the chain's units: every GEMM's tile row i is the same lane, and the
// running residual of row i is where the next epilogue needs it.  Output rows per workgroup
// [F, F + RO), F = 2 U (FIN: the next multiple of 4, so that rb and RO are multiples of 4).  LDS row
// L = i + 1 (rows 0 and NR + 1 are zero pads, ZR the zero row of taps that leave a clip); one buffer,
// overwritten stage by stage.
// FIN (unit 9 last): the epilogue writes BN + ReLU + AveragePooling1D(4) of the chain's output
// (speaker_identification.py:208-212, nets.hip bn_relu_avgpool4_kernel's arithmetic) instead of the
// output itself; a pool window is 4 adjacent lanes, summed in that kernel's order through DPP
// broadcasts.
// The struct of a unit the chain does not have is passed zeroed and never read.
template <int CIN, int C, int NR, int NW, bool POOL, int NU, bool FIN, int MINW>
__global__ void __launch_bounds__(64 * NW, MINW) siu_chain_kernel(SiuArgs p, SiuArgs a, SiuArgs b) {
  constexpr int NT = 64 * NW;
  constexpr int WN = C / 32;
  constexpr int WM = NW / WN;
  constexpr int MT = NR / (WM * 32);
  constexpr int NCHX = CIN / CK, NCH = C / CK;
  constexpr int LDP = C + 8;
  constexpr int U = (POOL ? 1 : 0) + NU;
  constexpr int F = chain_front<U, FIN>(), RO = chain_rows<NR, U, FIN>();
  constexpr int ZR = NR + 2;
  constexpr int QPP = CK / 4;
  constexpr int MAXT = (NR * QPP + NT - 1) / NT;
  constexpr int P0 = POOL ? 2 : 0;     // rows the pool unit narrows
  static_assert(WM * WN == NW && MT * WM * 32 == NR && NT % QPP == 0, "tiling");
  static_assert(POOL || CIN == C, "units without pooling keep their width");
  static_assert(U >= 1 && NU <= 2 && F >= 2 * U && RO > 0 && F + RO <= NR - 2 * U, "rows");
  static_assert(!FIN || (NU >= 1 && F % 4 == 0 && RO % 4 == 0), "the last unit keeps its width; pool windows");
  __shared__ __attribute__((aligned(16))) _Float16 lhi[(NR + 3) * LDP];
  __shared__ __attribute__((aligned(16))) _Float16 llo[(NR + 3) * LDP];
  // per-channel parameters: unit a [0] b_a [1] 16 s_mid [2] 16 t_mid [3] b_b; unit b [4] 16 s_in
  // [5] 16 t_in [6] b_a [7] 16 s_mid [8] 16 t_mid [9] b_b; FIN [10] fs [11] ft; POOL: unit a [12]
  // 16 s_in [13] 16 t_in, the pool unit [14] b_a [15] 16 s_mid [16] 16 t_mid [17] b_b [18] b_s
  // (the rows of a unit the chain does not have stay unused)
  constexpr int NPAR = POOL ? 19 : 12;
  __shared__ __attribute__((aligned(16))) float spar[NPAR * C];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave - (wave / WN) * WN;
  const SiuArgs& s0 = POOL ? p : a;                            // the chain's first unit: its input
  const SiuArgs& last = NU == 2 ? b : NU == 1 ? a : p;         // ... and its last: its output
  const SiuArgs& dims = NU >= 1 ? a : p;                       // n, t, tdiv_*, range_flag (equal in all)
  const int T = dims.t;
  const int HH = dims.n * T;                                   // rows of the batch (< 2^24, the launcher checks)
  const int rb = (int)blockIdx.x * RO - F;
  const int koff = (lane >> 5) * 8;
  const int h4 = 4 * (lane >> 5);
  const uint32_t tm = dims.tdiv_m, ts = dims.tdiv_s;
  float rmax = 0.0f;                                           // the largest scaled operand this thread split
  int rbad = 0;   // a raw shortcut operand out of range / NaN (an int, pinned per tile: see below)
  const __amdgpu_buffer_rsrc_t rx = siu_rsrc(s0.x);

  for (int e = tid; e < 3 * (LDP / 8); e += NT) {   // pad rows 0, NR + 1 and the zero row
    const int z = e / (LDP / 8), k8 = e - z * (LDP / 8);
    const int row = z == 0 ? 0 : z == 1 ? NR + 1 : ZR;
    *reinterpret_cast<f16x8*>(lhi + row * LDP + 8 * k8) = f16x8{};
    *reinterpret_cast<f16x8*>(llo + row * LDP + 8 * k8) = f16x8{};
  }
  for (int i = tid; i < C; i += NT) {
    if constexpr (NU >= 1) {
      spar[i] = a.ba[i];
      spar[C + i] = ACT_SCALE * a.s_mid[i];
      spar[2 * C + i] = ACT_SCALE * a.t_mid[i];
      spar[3 * C + i] = a.bb[i];
    }
    if constexpr (NU >= 2) {
      spar[4 * C + i] = ACT_SCALE * b.s_in[i];
      spar[5 * C + i] = ACT_SCALE * b.t_in[i];
      spar[6 * C + i] = b.ba[i];
      spar[7 * C + i] = ACT_SCALE * b.s_mid[i];
      spar[8 * C + i] = ACT_SCALE * b.t_mid[i];
      spar[9 * C + i] = b.bb[i];
    }
    if constexpr (FIN) {
      spar[10 * C + i] = last.fs[i];
      spar[11 * C + i] = last.ft[i];
    }
    if constexpr (POOL && NU >= 1) {
      spar[12 * C + i] = ACT_SCALE * a.s_in[i];
      spar[13 * C + i] = ACT_SCALE * a.t_in[i];
    }
    if constexpr (POOL) {
      spar[14 * C + i] = p.ba[i];
      spar[15 * C + i] = ACT_SCALE * p.s_mid[i];
      spar[16 * C + i] = ACT_SCALE * p.t_mid[i];
      spar[17 * C + i] = p.bb[i];
      spar[18 * C + i] = p.bs[i];
    }
  }

  // ---- stage the chain's input rows i < NR: BN_in + ReLU, x 2^4, split (all chunks, one barrier)
  //      into LDS rows 1 .. NR (POOL: row g = (clip, tt) is the max of the clip's unpooled rows 2 tt,
  //      2 tt + 1).  Rows outside the batch load row 0 / HH - 1 instead: a row of the batch reaches
  //      them only through taps that leave its clip (the zero row), and their own results are never
  //      written -----------------------------------------------------------------------------------
  {
    const int q = tid % QPP;
#pragma unroll 1
    for (int ch = 0; ch < NCHX; ++ch) {
      const int ci = ch * CK + 4 * q;
      float4 sc = *reinterpret_cast<const float4*>(s0.s_in + ci);
      float4 sh = *reinterpret_cast<const float4*>(s0.t_in + ci);
      sc = make_float4(ACT_SCALE * sc.x, ACT_SCALE * sc.y, ACT_SCALE * sc.z, ACT_SCALE * sc.w);
      sh = make_float4(ACT_SCALE * sh.x, ACT_SCALE * sh.y, ACT_SCALE * sh.z, ACT_SCALE * sh.w);
      float4 pre[MAXT];
#pragma unroll
      for (int j = 0; j < MAXT; ++j) {
        const int task = tid + j * NT;
        const int g = min(max(rb + task / QPP, 0), HH - 1);
        if constexpr (POOL) {
          const uint32_t cl = tdiv((uint32_t)g, tm, ts);
          const int tt = g - (int)cl * T;
          const uint32_t src = ((uint32_t)cl * (uint32_t)p.t_src + 2u * tt) * (CIN * 4u) + ci * 4u;
          const float4 v = ld4(rx, src);
          const float4 u = ld4(rx, 2 * tt + 1 < p.t_src ? src + CIN * 4u : src);
          pre[j] = make_float4(fmaxf(v.x, u.x), fmaxf(v.y, u.y), fmaxf(v.z, u.z), fmaxf(v.w, u.w));
        } else {
          pre[j] = ld4(rx, (uint32_t)g * (C * 4u) + ci * 4u);
        }
      }
#pragma unroll
      for (int j = 0; j < MAXT; ++j) {
        const int task = tid + j * NT;
        if (MAXT * NT > NR * QPP && task >= NR * QPP) continue;
        f16x4 hv, lv;
        bn_split4(pre[j], sc, sh, hv, lv, rmax);
        const int row = task / QPP + 1;
        *reinterpret_cast<f16x4*>(lhi + row * LDP + ci) = hv;
        *reinterpret_cast<f16x4*>(llo + row * LDP + ci) = lv;
      }
    }
  }

  constexpr int kstride = (C / 32) * 512;
  const int lofs = wn * 512 + lane * 8;
  int mrow[MT], trow[MT], grow[MT];   // per tile: this lane's row i, its position in its clip, rb + i
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    mrow[mt] = (wm * MT + mt) * 32 + (lane & 31);
    grow[mt] = rb + mrow[mt];
    const uint32_t gp = (uint32_t)(grow[mt] + T);
    trow[mt] = (int)(gp - tdiv(gp, tm, ts) * (uint32_t)T);
  }
  // acc = W^T X^T over LDS rows, NCHK 32-channel chunks (row i's taps: LDS rows i .. i + 2, or the
  // zero row)
  auto gemm = [&](auto nchk_c, const uint16_t* wh, const uint16_t* wl, f32x16 (&acc)[MT]) {
    constexpr int NCHK = decltype(nchk_c)::value;
    constexpr int tap_stride = C * NCHK * CK;
    const __amdgpu_buffer_rsrc_t rwh = siu_rsrc(wh), rwl = siu_rsrc(wl);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[mt][i] = 0.0f;
#pragma unroll 1
    for (int ch = 0; ch < NCHK; ++ch) {
#pragma unroll 1
      for (int tap = 0; tap < TAPS; ++tap) {
        f16x8 bh[KS], bl[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          const int u = tap * tap_stride + (ch * KS + s) * kstride;
          bh[s] = ldw(rwh, lofs, u);
          bl[s] = ldw(rwl, lofs, u);
        }
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            const int src = trow[mt] + tap - 1;
            const int off = (src < 0 || src >= T ? ZR : mrow[mt] + tap) * LDP + ch * CK + 16 * s + koff;
            const f16x8 ah = *reinterpret_cast<const f16x8*>(lhi + off);
            const f16x8 al = *reinterpret_cast<const f16x8*>(llo + off);
            acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bl[s], ah, acc[mt], 0, 0, 0);
            acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh[s], al, acc[mt], 0, 0, 0);
            acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh[s], ah, acc[mt], 0, 0, 0);
          }
      }
    }
  };
  // LDS row i + 1 = split(max(fma(v, s16, t16), 0)) of each tile's row; rows outside [lo, NR - lo)
  // or the batch stay out of the range guard
  auto put = [&](const float (&v)[MT][16], int ps, int pt, int lo) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int L = mrow[mt] + 1;
      float tmax = 0.0f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int co0 = wn * 32 + 8 * q + h4;
        const float4 s = *reinterpret_cast<const float4*>(spar + ps * C + co0);
        const float4 t = *reinterpret_cast<const float4*>(spar + pt * C + co0);
        f16x4 hv, lv;
        bn_split4(make_float4(v[mt][4 * q], v[mt][4 * q + 1], v[mt][4 * q + 2], v[mt][4 * q + 3]), s, t, hv, lv,
                  tmax);
        *reinterpret_cast<f16x4*>(lhi + L * LDP + co0) = hv;
        *reinterpret_cast<f16x4*>(llo + L * LDP + co0) = lv;
      }
      if (mrow[mt] >= lo && mrow[mt] < NR - lo && grow[mt] >= 0 && grow[mt] < HH) rmax = fmaxf(rmax, tmax);
    }
  };
  // v = fma(acc, u, bias[pb])
  auto unscale = [&](const f32x16 (&acc)[MT], float u, int pb, float (&v)[MT][16]) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 bq = *reinterpret_cast<const float4*>(spar + pb * C + wn * 32 + 8 * q + h4);
        v[mt][4 * q] = fmaf(acc[mt][4 * q], u, bq.x);
        v[mt][4 * q + 1] = fmaf(acc[mt][4 * q + 1], u, bq.y);
        v[mt][4 * q + 2] = fmaf(acc[mt][4 * q + 2], u, bq.z);
        v[mt][4 * q + 3] = fmaf(acc[mt][4 * q + 3], u, bq.w);
      }
  };

  // y = fma(acc, u, bias[pb]) + y (the unit's epilogue: conv + residual, in that order)
  auto unscale_add = [&](const f32x16 (&acc)[MT], float u, int pb, float (&y)[MT][16]) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 bq = *reinterpret_cast<const float4*>(spar + pb * C + wn * 32 + 8 * q + h4);
        y[mt][4 * q] = fmaf(acc[mt][4 * q], u, bq.x) + y[mt][4 * q];
        y[mt][4 * q + 1] = fmaf(acc[mt][4 * q + 1], u, bq.y) + y[mt][4 * q + 1];
        y[mt][4 * q + 2] = fmaf(acc[mt][4 * q + 2], u, bq.z) + y[mt][4 * q + 2];
        y[mt][4 * q + 3] = fmaf(acc[mt][4 * q + 3], u, bq.w) + y[mt][4 * q + 3];
      }
  };

  f32x16 acc[MT];
  float v[MT][16];
  float y[MT][16];   // the running residual: each unit's output
  __syncthreads();
  if constexpr (POOL) {
    // the pool unit: t1, then y1 = conv_b + the shortcut Conv1D(1, stride 2) of x as conv_h3's
    // EPI_ADD_SC: the row's source row 2 tt of x (raw, x 2^4, split) is the B operand, 16-channel
    // k-steps, its own accumulator (the shortcut first, into y, while GEMM a's accumulators are dead)
    gemm(std::integral_constant<int, NCHX>{}, p.wah, p.wal, acc);
    __syncthreads();
    unscale(acc, p.ua, 14, v);
    put(v, 15, 16, 1);
    const __amdgpu_buffer_rsrc_t rsh = siu_rsrc(p.wsh), rsl = siu_rsrc(p.wsl);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      f32x16 sacc;
#pragma unroll
      for (int i = 0; i < 16; ++i) sacc[i] = 0.0f;
      const int gs = min(max(grow[mt], 0), HH - 1);
      const uint32_t cl = tdiv((uint32_t)gs, tm, ts);
      const int tt = gs - (int)cl * T;
      const uint32_t sxo = ((uint32_t)cl * (uint32_t)p.t_src + 2u * tt) * (CIN * 4u) + koff * 4u;
#pragma unroll
      for (int s = 0; s < CIN / 16; ++s) {
        const f16x8 sbh = ldw(rsh, lofs, s * kstride);
        const f16x8 sbl = ldw(rsl, lofs, s * kstride);
        const float4 x0 = ld4(rx, sxo + 64u * s), x1 = ld4(rx, sxo + 64u * s + 16u);
        const float xv[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
        f16x8 xh, xl;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float w = xv[k] * ACT_SCALE;
          rbad |= !(fabsf(w) < SPLIT_MAX) ? 1 : 0;
          xh[k] = (_Float16)w;
          xl[k] = (_Float16)(w - (float)xh[k]);
        }
        sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(sbl, xh, sacc, 0, 0, 0);
        sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(sbh, xl, sacc, 0, 0, 0);
        sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(sbh, xh, sacc, 0, 0, 0);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 bs = *reinterpret_cast<const float4*>(spar + 18 * C + wn * 32 + 8 * q + h4);
        y[mt][4 * q] = fmaf(sacc[4 * q], p.us, bs.x);
        y[mt][4 * q + 1] = fmaf(sacc[4 * q + 1], p.us, bs.y);
        y[mt][4 * q + 2] = fmaf(sacc[4 * q + 2], p.us, bs.z);
        y[mt][4 * q + 3] = fmaf(sacc[4 * q + 3], p.us, bs.w);
      }
      // evaluate this tile's range tests here: left to the compiler, they sink to the kernel's end
      // and keep every scaled shortcut operand alive across the chain (hundreds of spilled VGPRs)
      asm volatile("" : "+v"(rbad));
      __builtin_amdgcn_sched_barrier(0);   // one tile's shortcut operands live at a time
    }
    __syncthreads();
    gemm(std::integral_constant<int, NCH>{}, p.wbh, p.wbl, acc);
    unscale_add(acc, p.ub, 17, y);
    if constexpr (NU >= 1) {
      __syncthreads();   // every wave has read t1
      put(y, 12, 13, 2);
      __syncthreads();
    }
  } else {
    // the raw x of each tile row: the first unit's residual, loaded under its GEMMs
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int g = min(max(grow[mt], 0), HH - 1);
        const float4 r = ld4(rx, (uint32_t)g * (C * 4u) + (wn * 32 + 8 * q + h4) * 4u);
        y[mt][4 * q] = r.x;
        y[mt][4 * q + 1] = r.y;
        y[mt][4 * q + 2] = r.z;
        y[mt][4 * q + 3] = r.w;
      }
  }
  if constexpr (NU >= 1) {   // unit a
    gemm(std::integral_constant<int, NCH>{}, a.wah, a.wal, acc);
    __syncthreads();
    unscale(acc, a.ua, 0, v);
    put(v, 1, 2, P0 + 1);
    __syncthreads();
    gemm(std::integral_constant<int, NCH>{}, a.wbh, a.wbl, acc);
    unscale_add(acc, a.ub, 3, y);
  }
  if constexpr (NU >= 2) {   // unit b
    __syncthreads();   // every wave has read t1
    put(y, 4, 5, P0 + 2);
    __syncthreads();
    gemm(std::integral_constant<int, NCH>{}, b.wah, b.wal, acc);
    __syncthreads();
    unscale(acc, b.ua, 6, v);
    put(v, 7, 8, P0 + 3);
    __syncthreads();
    gemm(std::integral_constant<int, NCH>{}, b.wbh, b.wbl, acc);
    unscale_add(acc, b.ub, 9, y);
  }
  // the last unit's output
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int i = mrow[mt], g = grow[mt];
    const bool ok = i >= F && i < F + RO && g < HH;
    if constexpr (!FIN) {
      if (ok) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 val = make_float4(y[mt][4 * q], y[mt][4 * q + 1], y[mt][4 * q + 2], y[mt][4 * q + 3]);
          *reinterpret_cast<float4*>(last.y + (size_t)g * C + wn * 32 + 8 * q + h4) = val;
        }
      }
    } else {
      // BN + ReLU of each row, then the 4-row window sum in bn_relu_avgpool4's order ((r0 + r1) + r2) + r3:
      // lanes 4k .. 4k + 3 hold rows rb + i, i = 0 .. 3 mod 4
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int co0 = wn * 32 + 8 * q + h4;
        const float4 fs = *reinterpret_cast<const float4*>(spar + 10 * C + co0);
        const float4 ft = *reinterpret_cast<const float4*>(spar + 11 * C + co0);
        const float fsv[4] = {fs.x, fs.y, fs.z, fs.w}, ftv[4] = {ft.x, ft.y, ft.z, ft.w};
        float out[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = __builtin_bit_cast(int, fmaxf(fmaf(y[mt][4 * q + e], fsv[e], ftv[e]), 0.0f));
          const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(r, 0x00, 0xf, 0xf, false));
          const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(r, 0x55, 0xf, 0xf, false));
          const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(r, 0xaa, 0xf, 0xf, false));
          const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(r, 0xff, 0xf, 0xf, false));
          out[e] = (((r0 + r1) + r2) + r3) / 4.0f;
        }
        if (ok && (i & 3) == 0)
          *reinterpret_cast<float4*>(last.seq + (size_t)(g >> 2) * C + co0) =
              make_float4(out[0], out[1], out[2], out[3]);
      }
    }
  }
  if ((rbad || !(rmax < SPLIT_MAX)) && dims.range_flag) *dims.range_flag = 1;
}

// q = x / d for x < 2^31 as (umulhi(x, m) + x) >> s: s = ceil(log2 d), m = floor(2^(32+s) / d) + 1 - 2^32
void siu_fastdiv(uint32_t d, uint32_t& m, uint32_t& s) {
  s = 0;
  while ((1u << s) < d) ++s;
  m = (uint32_t)(((uint64_t)1 << (32 + s)) / d + 1 - ((uint64_t)1 << 32));
}

// units: the chain in order, (POOL ? 1 : 0) + NU of them (siu_chain_launch has checked them)
template <int CIN, int C, int NR, bool POOL, int NU, bool FIN = false, int MINW = 2>
hipError_t launch(const SiuArgs* units, hipStream_t s) {
  constexpr int NW = 4, U = (POOL ? 1 : 0) + NU, RO = chain_rows<NR, U, FIN>();
  SiuArgs pab[3] = {};   // the kernel's p, a, b
  for (int k = 0; k < U; ++k) {
    SiuArgs& d = pab[k + (POOL ? 0 : 1)];
    d = units[k];
    siu_fastdiv((uint32_t)d.t, d.tdiv_m, d.tdiv_s);
  }
  // 32-bit row indices and byte offsets: x (a pool unit's: [n t_src, CIN]) and y below 4 GiB
  const int64_t rows = (int64_t)units[0].n * units[0].t;
  const int64_t xbytes = (int64_t)units[0].n * (POOL ? units[0].t_src : units[0].t) * CIN * 4;
  if (rows >= (1 << 24) || xbytes > 0xffffff00ll || rows * C * 4 > 0xffffff00ll) return hipErrorInvalidValue;
  const int64_t blocks = (rows + RO - 1) / RO;
  hipLaunchKernelGGL((siu_chain_kernel<CIN, C, NR, NW, POOL, NU, FIN, MINW>), dim3((unsigned)blocks), dim3(64 * NW),
                     0, s, pab[0], pab[1], pab[2]);
  return hipGetLastError();
}

}  // namespace

bool siu_chain_supported(int cin, int c, bool pool, int n_units, bool fin) {
  if (fin && c != 128) return false;   // the last unit of the net
  if (pool)   // alone, or with the two units after it; never the net's last
    return ((cin == 32 && c == 32) || (cin == 32 && c == 64) || (cin == 64 && c == 128)) &&
           (n_units == 3 || (n_units == 1 && !fin));
  return cin == c && (c == 32 || c == 64 || c == 128) && (n_units == 1 || n_units == 2);
}

hipError_t siu_chain_launch(const SiuArgs* units, int n_units, bool pool, int cin, int c, hipStream_t s) {
  if (n_units < 1 || n_units > 3) return hipErrorInvalidValue;
  const SiuArgs& first = units[0];
  const SiuArgs& last = units[n_units - 1];
  const bool fin = last.seq != nullptr;
  if ((int64_t)first.n * first.t == 0) return hipSuccess;
  if (!siu_chain_supported(cin, c, pool, n_units, fin) || !first.x || first.t < 1) return hipErrorInvalidValue;
  for (int k = 1; k < n_units; ++k)
    if (units[k].n != first.n || units[k].t != first.t) return hipErrorInvalidValue;
  if (pool && (!first.wsh || !first.wsl || !first.bs || first.t != (first.t_src + 1) / 2)) return hipErrorInvalidValue;
  if (fin ? !last.fs || !last.ft || last.t % 4 != 0 : !last.y || last.y == first.x) return hipErrorInvalidValue;
  const int nu = n_units - (pool ? 1 : 0);
  // Tiles (4 waves).  The chains of two and three units: 256 rows, C = 128 128 rows; 3 waves per SIMD
  // at C = 32
  if (nu == 2) {
    if (pool && fin) return launch<64, 128, 128, true, 2, true>(units, s);
    if (!pool && fin) return launch<128, 128, 128, false, 2, true>(units, s);
    if (pool && cin == 32 && c == 32) return launch<32, 32, 256, true, 2, false, 3>(units, s);
    if (pool && cin == 32 && c == 64) return launch<32, 64, 256, true, 2>(units, s);
    if (pool && cin == 64 && c == 128) return launch<64, 128, 128, true, 2>(units, s);
    if (c == 32) return launch<32, 32, 256, false, 2, false, 3>(units, s);
    if (c == 64) return launch<64, 64, 256, false, 2>(units, s);
    return launch<128, 128, 128, false, 2>(units, s);
  }
  if (pool) {   // the pool unit alone
    if (cin == 32 && c == 32) return launch<32, 32, 256, true, 0>(units, s);
    // unit 4 (32 -> 64 channels): 128-row tiles at 3 waves per SIMD (112 VGPRs, 37.7 KB) instead of
    // 256-row tiles at 2 (152 VGPRs, 74.6 KB): SI +1.1 % (A/B, 2 rounds; the same choice for the other
    // units -- C 32 pool / non-pool at 128 rows and 4 waves per SIMD, C 64 at 128 rows -- was neutral)
    if (cin == 32 && c == 64) return launch<32, 64, 128, true, 0, false, 3>(units, s);
    // unit 7 (64 -> 128): 64-row tiles at 3 waves per SIMD (158 VGPRs) instead of 128-row tiles at 2
    // (227): SI +1.0 % (A/B, 2 rounds; 64-row tiles for units 8 / 9 at 3 waves: +0.1-0.6 % / noise)
    return launch<64, 128, 64, true, 0, false, 3>(units, s);
  }
  // One unit: C = 32 256 rows (MT 2, 3 workgroups per CU); C = 64 256 rows and C = 128 128 rows
  // (MT 4, 2 per CU).  Measured per unit and SI step against the conv_h3 pair (round 4, with
  // ROWS - 2 output rows per workgroup where the chain geometry now gives NR - 4): C = 32 1.004 vs
  // 1.033 ms, C = 64 (128-row tiles) 1.061 vs 1.203 ms, C = 128 with 64-row tiles 1.672 vs 1.625 ms
  // (B streamed per 62 output rows).  Tried: 8-wave workgroups (one per CU) and 512-row C = 32 tiles
  // (occupancy 1): slower
  if (fin) return launch<128, 128, 128, false, 1, true>(units, s);
  if (c == 32) return launch<32, 32, 256, false, 1>(units, s);
  if (c == 64) return launch<64, 64, 256, false, 1>(units, s);
  return launch<128, 128, 128, false, 1>(units, s);
}
