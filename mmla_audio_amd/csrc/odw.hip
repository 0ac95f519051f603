// odu.hip's res block kernel (OverlapDetection blocks 4-9, one launch per block, t1 on chip) with TWO
// strips per workgroup on one weight stream.  Runs blocks 7 and 8-9, where it measured faster (odw_supported).
//
// odu gives a workgroup one strip of 64 or 128 pixels, and each of its waves streams its share of the
// block's whole split weight set (147-852 KB) from L2 for that one strip: 35-184 GB per 16 384-clip
// launch through the vector-memory path, several times the launch's HBM traffic.  Here workgroup b owns
// the logical strips 2 b and 2 b + 1 of odu's (clip-major, strip-minor) order, each with its own clip,
// column, buffer descriptor, x halo and t1 rows in LDS, and the tile loops of GEMM a, GEMM b and the
// shortcut GEMM run over both strips' tiles: one loaded weight fragment pair (hi, lo) feeds 2 MT tiles
// instead of MT, so the weight loads per MFMA halve.  The LDS doubles, so two workgroups share a CU
// (two waves per SIMD, 256 VGPRs each).
//
// Bit-identical to odu: per accumulator the product sequence is odu's (32-channel chunks, then taps,
// then 16-deep k-steps; lo*hi, hi*lo, hi*hi), the staged operands and both epilogues are odu's
// arithmetic.  Staging, the t1 write and the epilogue go strip by strip, so the staging registers do
// not double.  A pair may straddle two clips; when n * strips is odd the last workgroup's second strip
// does not exist: its column is past the image, so every load of it takes the out-of-range offset and
// stages zeros (nothing enters the range maximum), and its stores are skipped.
//
// LDS: the x halos keep odu's conflict-free layouts per strip.  The two strips' t1 planes are stacked
// and share their zero rows (strip 0's two rows below the image double as strip 1's row above it):
//     row 0 | strip 0 rows 1 .. H | H + 1, H + 2 | strip 1 rows H + 3 .. 2 H + 2 | 2 H + 3, 2 H + 4
// env MMLA_NO_ODW=1 at mmla_create runs odu instead (tests/test_gpu_odw.py compares the two).
#include "common.h"
#include "conv.h"
#include "odw.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

constexpr int CK = 32;                 // channel chunk (conv_h3's k order)
constexpr int KS = CK / 16;            // MFMA k-steps per chunk
constexpr int NS = 2;                  // strips per workgroup
constexpr float ACT_SCALE = 16.0f;     // 2^4, as conv_h3
constexpr float SPLIT_MAX = 65504.0f;  // largest finite fp16 (operands are compared once scaled)

// the helpers below are odu.hip's (that file's kernel objects are pinned, so it keeps its own copies)
MMLA_DEV __amdgpu_buffer_rsrc_t odw_rsrc(const void* p) {
  const uint64_t u = reinterpret_cast<uint64_t>(p);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)u);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(u >> 32));
  return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((uint64_t)hi << 32) | lo), (short)0,
                                           (int)0x7fffffff, 0x00020000);
}
// 16 B of a split weight: wave-uniform half offset uoff + this lane's lofs
MMLA_DEV f16x8 odw_frag(__amdgpu_buffer_rsrc_t r, size_t uoff, int lofs) {
  return __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(r, (uint32_t)lofs * 2u, (int)(uoff * 2), 0));
}

MMLA_DEV float bn_elu16(float v, float sc16, float sh16) { return elu16(fmaf(v, sc16, sh16)); }
MMLA_DEV float4 x16(float4 v) { return make_float4(ACT_SCALE * v.x, ACT_SCALE * v.y, ACT_SCALE * v.z, ACT_SCALE * v.w); }

// v (already x 2^4) = hi + lo, both fp16
MMLA_DEV void split4(float4 v, f16x4& h, f16x4& l) {
  h[0] = (_Float16)v.x;
  h[1] = (_Float16)v.y;
  h[2] = (_Float16)v.z;
  h[3] = (_Float16)v.w;
  const uint2 hu = __builtin_bit_cast(uint2, h);
  l = __builtin_bit_cast(f16x4, make_uint2(split_lo2(v.x, v.y, hu.x), split_lo2(v.z, v.w, hu.y)));
}

MMLA_DEV float amax4(float r, float4 v) {
  return fmaxf(r, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
}

// a group's issue order, for the scheduler: NR LDS reads (a later group's fragments), then 3 MFMAs
template <int LA, int NR>
MMLA_DEV void odw_pin_group() {
  if constexpr (LA > 0) {
    if constexpr (NR > 0) __builtin_amdgcn_sched_group_barrier(0x100, NR, 0);   // DS_READ
    __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);                          // MFMA
    __builtin_amdgcn_sched_barrier(0);
  }
}

// odu_kernel's geometry (H x W image, CIN -> C channels, strips of TW columns, 4 waves: WN = C / 32
// along the output channels, WM along a strip's H * TW pixels, MT 32-pixel tiles per wave and strip),
// two strips: tile t = strip * MT + mt.  DBUF: two halo buffers per strip where CIN has several chunks
// (odu's DB).  LA, LB: odu's LDS operand pipeline depths.
template <int H, int W, int CIN, int C, int TW, bool POOL, bool DBUF, int LA, int LB>
__global__ void __launch_bounds__(256, 2) odw_kernel(OduArgs a) {
  constexpr int NW = 4, NT = 64 * NW;
  constexpr int NB = LA + 1;
  constexpr int WN = C / 32, WM = NW / WN;
  constexpr int M = H * TW;
  constexpr int MT = M / (WM * 32);
  constexpr int NTL = NS * MT;                            // tiles per wave
  static_assert(MT * WM * 32 == M && WN * WM == NW, "tiling");
  static_assert(!POOL || (TW == 2 && H % 2 == 0 && W % 2 == 0 && MT <= 4), "pool strips");
  static_assert(POOL || CIN == C, "residual blocks keep their width");
  constexpr int TLW = (W + TW - 1) / TW;
  constexpr int XP = TW + 2, XH = H + 2, NXP = XH * XP;   // x halo: rows -1 .. H, columns -1 .. TW
  constexpr int LDX = TW == 2 ? CK : CK + 8;              // fp16 per staged x pixel (odu's layouts)
  constexpr int XRP = TW == 2 ? 144 : TW == 4 ? 288 : XP * LDX;   // fp16 per halo row
  constexpr bool XSW = TW == 2;                           // odd-column half swap
  constexpr int LDT = C + 8;                              // fp16 per t1 pixel
  constexpr int T1S = (H + 2) * TW * LDT;                 // strip s's t1 row r is plane row s (H + 2) + r
  constexpr int T1TOT = (NS * (H + 2) + 1) * TW * LDT;
  constexpr int NCHX = CIN / CK, NCH = C / CK;
  constexpr bool DB = DBUF && NCHX > 1;
  constexpr int XBUF = XH * XRP;                          // fp16 per halo buffer and plane
  constexpr int XTOT = DB ? 2 * XBUF : XBUF;              // ... per strip
  constexpr int PLANE = NS * XTOT > T1TOT ? NS * XTOT : T1TOT;
  constexpr int QPP = CK / 4;                             // float4 per pixel and chunk
  constexpr int MAXT = (NXP * QPP + NT - 1) / NT;
  static_assert(NT % QPP == 0, "a thread's channel quad is fixed");
  __shared__ __attribute__((aligned(16))) _Float16 lhi[PLANE];
  __shared__ __attribute__((aligned(16))) _Float16 llo[PLANE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave - (wave / WN) * WN;
  const uint32_t bid = xcd_block_id();
  const int64_t strips = (int64_t)a.n * TLW;
  // the two strips: clip, first column (past the image for a strip that does not exist, so its halo,
  // t1 and residual all take their out-of-image paths) and the clip's input through a buffer
  // descriptor (out-of-image pixels read zeros with no branch around the load)
  bool live[NS];
  int64_t clip[NS];
  int w0[NS];
  __amdgpu_buffer_rsrc_t rxc[NS];
#pragma unroll
  for (int sp = 0; sp < NS; ++sp) {
    const int64_t sid = (int64_t)bid * NS + sp;
    live[sp] = sid < strips;
    clip[sp] = live[sp] ? sid / TLW : 0;
    w0[sp] = live[sp] ? (int)(sid - clip[sp] * TLW) * TW : W + TW;
    rxc[sp] = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x + clip[sp] * ((int64_t)H * W * CIN)), (short)0,
                                                live[sp] ? (int)(H * W * CIN * 4) : 0, 0x00020000);
  }
  const int koff = (lane >> 5) * 8;
  const int hsel = 4 * (lane >> 5);
  const int cob = wn * 32;                    // this wave's output-channel tile
  const int lofs = wn * 512 + lane * 8;       // its B fragment inside a (tap, k-step) 1 KB block
  constexpr size_t kstr = (size_t)(C / 32) * 512;
  float rmax = 0.0f;   // the largest |operand| this thread split (x 2^4)

  int mpix[MT];   // the wave's pixels in either strip: strip pixel m = i * TW + c
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) mpix[mt] = (wm * MT + mt) * 32 + (lane & 31);

  f32x16 acc[NTL];
#pragma unroll
  for (int t = 0; t < NTL; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;

  // ---- GEMM a: t1^T = Wa^T X^T over both halos, chunk by chunk -------------------------------------
  {
    const __amdgpu_buffer_rsrc_t rh = odw_rsrc(a.wah), rl = odw_rsrc(a.wal);
    constexpr size_t tap_stride = (size_t)C * CIN;
    const int q = tid % QPP;
    const int kx0 = XSW ? 8 * ((lane >> 5) ^ (lane & 1)) : koff;
    const int kx1 = XSW ? 8 * ((lane >> 5) ^ (lane & 1) ^ 1) : koff;
    // global loads of chunk ch's halo quads of strip sp, then BN_in + ELU + 2^4 + split into its buffer buf
    auto load_stage = [&](int sp, int ch, int buf) {
      const int ci = ch * CK + 4 * q;
      const float4 sc = x16(*reinterpret_cast<const float4*>(a.s_in + ci));
      const float4 sh = x16(*reinterpret_cast<const float4*>(a.t_in + ci));
      float4 pre[MAXT];
      uint32_t valid = 0;
#pragma unroll
      for (int j = 0; j < MAXT; ++j) {
        const int task = tid + j * NT;
        const int px = task / QPP;
        const int ih = px / XP - 1, iw = w0[sp] + px % XP - 1;
        const bool ok = task < NXP * QPP && ih >= 0 && ih < H && iw >= 0 && iw < W;
        pre[j] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(
                                                rxc[sp], ok ? (uint32_t)((ih * W + iw) * CIN + ci) * 4u : 0x80000000u, 0, 0));
        valid |= (uint32_t)ok << j;
      }
      // keep the flags one VGPR: seen through, they become a lane-mask SGPR pair per load, live for
      // both strips at once where the scheduler hoists strip 1's loads, and the kernel spills SGPRs
      asm volatile("" : "+v"(valid));
      _Float16* const xh = lhi + sp * XTOT + buf * XBUF;
      _Float16* const xl = llo + sp * XTOT + buf * XBUF;
#pragma unroll
      for (int j = 0; j < MAXT; ++j) {
        const int task = tid + j * NT;
        if (task >= NXP * QPP) continue;
        float4 v = pre[j];
        if (valid & (1u << j)) {
          v.x = bn_elu16(v.x, sc.x, sh.x);
          v.y = bn_elu16(v.y, sc.y, sh.y);
          v.z = bn_elu16(v.z, sc.z, sh.z);
          v.w = bn_elu16(v.w, sc.w, sh.w);
        }
        rmax = amax4(rmax, v);
        f16x4 hv, lv;
        split4(v, hv, lv);
        const int px = task / QPP;
        const int cx = px % XP;
        const int xo = (px / XP) * XRP + cx * LDX + (XSW ? 8 * ((q >> 1) ^ (cx & 1)) + 4 * (q & 1) : 4 * q);
        *reinterpret_cast<f16x4*>(xh + xo) = hv;
        *reinterpret_cast<f16x4*>(xl + xo) = lv;
      }
    };
    if constexpr (DB) {
#pragma unroll
      for (int sp = 0; sp < NS; ++sp) load_stage(sp, 0, 0);
      __syncthreads();
    }
#pragma unroll 1
    for (int ch = 0; ch < NCHX; ++ch) {
      const int buf = DB ? (ch & 1) : 0;
      // tap 0's B fragments, in flight across the staging
      f16x8 bh[KS], bl[KS];
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        bh[s] = odw_frag(rh, (size_t)(ch * KS + s) * kstr, lofs);
        bl[s] = odw_frag(rl, (size_t)(ch * KS + s) * kstr, lofs);
      }
      if constexpr (!DB) {
        if (ch > 0) __syncthreads();   // every wave is done reading the previous chunk
#pragma unroll
        for (int sp = 0; sp < NS; ++sp) load_stage(sp, ch, 0);
        __syncthreads();
      }
      // group g = (tap * KS + s) * NTL + t of this chunk: its A fragments' LDS offset
      constexpr int NG = 9 * KS * NTL;
      auto aoff = [&](int g) {
        const int t = g % NTL, s = (g / NTL) % KS, tap = g / (NTL * KS);
        const int dy = tap / 3, dx = tap - (tap / 3) * 3;
        const int m = mpix[t % MT];
        return (t / MT) * XTOT + buf * XBUF + (m / TW + dy) * XRP + (m % TW + dx) * LDX + 16 * s + (dx & 1 ? kx1 : kx0);
      };
      f16x8 fah[NB], fal[NB];
#pragma unroll
      for (int d = 0; d < LA; ++d) {
        fah[d] = *reinterpret_cast<const f16x8*>(lhi + aoff(d));
        fal[d] = *reinterpret_cast<const f16x8*>(llo + aoff(d));
      }
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        f16x8 nbh[KS], nbl[KS];
        if (tap + 1 < 9) {   // the next tap's fragments under this tap's MFMAs
#pragma unroll
          for (int s = 0; s < KS; ++s) {
            const size_t u = (tap + 1) * tap_stride + (size_t)(ch * KS + s) * kstr;
            nbh[s] = odw_frag(rh, u, lofs);
            nbl[s] = odw_frag(rl, u, lofs);
          }
        }
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
          for (int t = 0; t < NTL; ++t) {
            const int g = (tap * KS + s) * NTL + t;
            if (g + LA < NG) {
              fah[(g + LA) % NB] = *reinterpret_cast<const f16x8*>(lhi + aoff(g + LA));
              fal[(g + LA) % NB] = *reinterpret_cast<const f16x8*>(llo + aoff(g + LA));
            }
            const f16x8 ah = fah[g % NB], al = fal[g % NB];
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bl[s], ah, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh[s], al, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh[s], ah, acc[t], 0, 0, 0);
            if (g + LA < NG) odw_pin_group<LA, 2>(); else odw_pin_group<LA, 0>();
          }
        if (tap + 1 < 9) {
#pragma unroll
          for (int s = 0; s < KS; ++s) {
            bh[s] = nbh[s];
            bl[s] = nbl[s];
          }
        }
      }
      if constexpr (DB) {
        if (ch + 1 < NCHX) {
          // buffer (ch + 1) & 1 was last read in chunk ch - 1, whose readers all passed the barrier
          // that ended that chunk; this chunk's MFMAs are issued and run on meanwhile
#pragma unroll
          for (int sp = 0; sp < NS; ++sp) load_stage(sp, ch + 1, buf ^ 1);
          __syncthreads();
        }
      }
    }
  }
  __syncthreads();   // every wave has read the x halos: the t1 planes overlay them

  // ---- t1 = ELU(BN_mid(acc * ua + ba)), x 2^4, split, into each strip's LDS rows 1 .. H ------------
#pragma unroll
  for (int qd = 0; qd < 4; ++qd) {
    const int c0 = cob + 8 * qd + hsel;   // the accumulator quad's 4 consecutive channels
    const float4 b4 = *reinterpret_cast<const float4*>(a.ba + c0);
    const float4 s4 = x16(*reinterpret_cast<const float4*>(a.s_mid + c0));
    const float4 t4 = x16(*reinterpret_cast<const float4*>(a.t_mid + c0));
#pragma unroll
    for (int t = 0; t < NTL; ++t) {
      const int sp = t / MT;
      const int m = mpix[t % MT];
      const int i = m / TW, c = m % TW;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (w0[sp] + c < W) {
        v.x = bn_elu16(fmaf(acc[t][4 * qd + 0], a.ua, b4.x), s4.x, t4.x);
        v.y = bn_elu16(fmaf(acc[t][4 * qd + 1], a.ua, b4.y), s4.y, t4.y);
        v.z = bn_elu16(fmaf(acc[t][4 * qd + 2], a.ua, b4.z), s4.z, t4.z);
        v.w = bn_elu16(fmaf(acc[t][4 * qd + 3], a.ua, b4.w), s4.w, t4.w);
      }
      rmax = amax4(rmax, v);
      f16x4 hv, lv;
      split4(v, hv, lv);
      const int px = (i + 1) * TW + c;
      *reinterpret_cast<f16x4*>(lhi + sp * T1S + px * LDT + c0) = hv;
      *reinterpret_cast<f16x4*>(llo + sp * T1S + px * LDT + c0) = lv;
    }
  }
  // the zero rows: plane rows 0, H + 1, H + 2, 2 H + 3, 2 H + 4
  for (int e = tid; e < (2 * NS + 1) * TW * (LDT / 8); e += NT) {
    const int z = e / (LDT / 8), k8 = e - z * (LDT / 8);
    const int zr = z / TW;
    const int row = zr == 0 ? 0 : ((zr + 1) / 2) * (H + 2) - 1 + ((zr + 1) & 1);
    const int px = row * TW + (z - zr * TW);
    *reinterpret_cast<f16x8*>(lhi + px * LDT + 8 * k8) = f16x8{};
    *reinterpret_cast<f16x8*>(llo + px * LDT + 8 * k8) = f16x8{};
  }

  // residual blocks: the raw x at the wave's output pixels.  Strip 0's is loaded now, so GEMM b hides
  // the latency; strip 1's behind GEMM b, under strip 0's epilogue (both across GEMM b: 64 more live
  // registers, spills at the 256 cap)
  float4 rsd[POOL ? 1 : NS][POOL ? 1 : MT][4];
  auto load_rsd = [&](int sp) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int m = mpix[mt];
      const int i = m / TW, c = m % TW;
      const bool ok = w0[sp] + c < W;
#pragma unroll
      for (int qd = 0; qd < 4; ++qd)
        rsd[sp][mt][qd] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(
                              rxc[sp], ok ? (uint32_t)((i * W + w0[sp] + c) * C + cob + 8 * qd + hsel) * 4u : 0x80000000u, 0, 0));
    }
  };
  if constexpr (!POOL) load_rsd(0);
#pragma unroll
  for (int t = 0; t < NTL; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;
  __syncthreads();

  // ---- GEMM b: conv(4,1) over t1 (output row i, tap dy reads the strip's t1 row i + dy) -------------
  {
    const __amdgpu_buffer_rsrc_t rh = odw_rsrc(a.wbh), rl = odw_rsrc(a.wbl);
    constexpr size_t tap_stride = (size_t)C * C;
#pragma unroll 1
    for (int ch = 0; ch < NCH; ++ch) {
      f16x8 bh[KS], bl[KS];
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        bh[s] = odw_frag(rh, (size_t)(ch * KS + s) * kstr, lofs);
        bl[s] = odw_frag(rl, (size_t)(ch * KS + s) * kstr, lofs);
      }
      // group g = (tap * KS + s) * NTL + t of this chunk, as in GEMM a
      constexpr int NG = 4 * KS * NTL;
      auto boff = [&](int g) {
        const int t = g % NTL, s = (g / NTL) % KS, tap = g / (NTL * KS);
        const int m = mpix[t % MT];
        return (t / MT) * T1S + ((m / TW + tap) * TW + m % TW) * LDT + ch * CK + 16 * s + koff;
      };
      f16x8 fah[LB + 1], fal[LB + 1];
#pragma unroll
      for (int d = 0; d < LB; ++d) {
        fah[d] = *reinterpret_cast<const f16x8*>(lhi + boff(d));
        fal[d] = *reinterpret_cast<const f16x8*>(llo + boff(d));
      }
#pragma unroll
      for (int tap = 0; tap < 4; ++tap) {
        f16x8 nbh[KS], nbl[KS];
        if (tap + 1 < 4) {
#pragma unroll
          for (int s = 0; s < KS; ++s) {
            const size_t u = (tap + 1) * tap_stride + (size_t)(ch * KS + s) * kstr;
            nbh[s] = odw_frag(rh, u, lofs);
            nbl[s] = odw_frag(rl, u, lofs);
          }
        }
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
          for (int t = 0; t < NTL; ++t) {
            const int g = (tap * KS + s) * NTL + t;
            if (g + LB < NG) {
              fah[(g + LB) % (LB + 1)] = *reinterpret_cast<const f16x8*>(lhi + boff(g + LB));
              fal[(g + LB) % (LB + 1)] = *reinterpret_cast<const f16x8*>(llo + boff(g + LB));
            }
            const f16x8 ah = fah[g % (LB + 1)], al = fal[g % (LB + 1)];
            if constexpr (POOL) {   // pixel rows: a register quad is one pool window
              acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl[s], acc[t], 0, 0, 0);
              acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh[s], acc[t], 0, 0, 0);
              acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh[s], acc[t], 0, 0, 0);
            } else {                // C^T: a register quad is 4 channels of one pixel
              acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bl[s], ah, acc[t], 0, 0, 0);
              acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh[s], al, acc[t], 0, 0, 0);
              acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh[s], ah, acc[t], 0, 0, 0);
            }
            if (g + LB < NG) odw_pin_group<LB, 2>(); else odw_pin_group<LB, 0>();
          }
        if (tap + 1 < 4) {
#pragma unroll
          for (int s = 0; s < KS; ++s) {
            bh[s] = nbh[s];
            bl[s] = nbl[s];
          }
        }
      }
    }
  }

  // ---- epilogue, strip by strip --------------------------------------------------------------------
  if constexpr (!POOL) {
    load_rsd(1);
#pragma unroll
    for (int t = 0; t < NTL; ++t) {
      const int sp = t / MT;
      const int m = mpix[t % MT];
      const int i = m / TW, c = m % TW;
      if (w0[sp] + c >= W) continue;   // also every pixel of a strip that does not exist
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) {
        const int c0 = cob + 8 * qd + hsel;
        const float4 b4 = *reinterpret_cast<const float4*>(a.bb + c0);
        const float4 r = rsd[sp][t % MT][qd];
        float4 v = make_float4(fmaf(acc[t][4 * qd + 0], a.ub, b4.x), fmaf(acc[t][4 * qd + 1], a.ub, b4.y),
                               fmaf(acc[t][4 * qd + 2], a.ub, b4.z), fmaf(acc[t][4 * qd + 3], a.ub, b4.w));
        v = make_float4(v.x + r.x, v.y + r.y, v.z + r.z, v.w + r.w);
        *reinterpret_cast<float4*>(a.y + ((clip[sp] * H + i) * W + w0[sp] + c) * C + c0) = v;
      }
    }
  } else {
    // the shortcut Conv2D(1x1, stride 2), odu's: A row rho = window (mt = rho >> 3, quad q = rho & 3,
    // lane half (rho >> 2) & 1) of a strip's main tiles; one weight fragment pair feeds both strips
    f32x16 sacc[NS];
#pragma unroll
    for (int sp = 0; sp < NS; ++sp)
#pragma unroll
      for (int i = 0; i < 16; ++i) sacc[sp][i] = 0.0f;
    {
      const int rho = lane & 31;
      const int smt = rho >> 3, sq = rho & 3, sh = (rho >> 2) & 1;
      const int m0 = (wm * MT + (smt < MT ? smt : 0)) * 32 + 8 * sq + 4 * sh;
      const __amdgpu_buffer_rsrc_t rh = odw_rsrc(a.wsh), rl = odw_rsrc(a.wsl);
#pragma unroll
      for (int s = 0; s < CIN / 16; ++s) {
        const f16x8 wh = odw_frag(rh, (size_t)s * kstr, lofs);
        const f16x8 wl = odw_frag(rl, (size_t)s * kstr, lofs);
#pragma unroll
        for (int sp = 0; sp < NS; ++sp) {
          const bool sok = smt < MT && live[sp];
          const float* sx = a.x + ((clip[sp] * H + m0 / TW) * W + (live[sp] ? w0[sp] : 0)) * CIN + koff;
          float4 x0 = make_float4(0.f, 0.f, 0.f, 0.f), x1 = x0;
          if (sok) {
            x0 = *reinterpret_cast<const float4*>(sx + 16 * s);
            x1 = *reinterpret_cast<const float4*>(sx + 16 * s + 4);
          }
          x0 = x16(x0);
          x1 = x16(x1);
          rmax = amax4(amax4(rmax, x0), x1);
          f16x4 h0, l0, h1, l1;
          split4(x0, h0, l0);
          split4(x1, h1, l1);
          const f16x8 xh = {h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
          const f16x8 xl = {l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]};
          sacc[sp] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xh, wl, sacc[sp], 0, 0, 0);
          sacc[sp] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xl, wh, sacc[sp], 0, 0, 0);
          sacc[sp] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xh, wh, sacc[sp], 0, 0, 0);
        }
      }
    }
    const int co = cob + (lane & 31);
    const float b = a.bb[co], bsc = a.bs[co];
#pragma unroll
    for (int t = 0; t < NTL; ++t) {
      const int sp = t / MT, mt = t % MT;
      if (!live[sp]) continue;
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) {
        // register quad qd: rows i0, i0 + 1 (i0 = m0 / 2, even) x columns w0, w0 + 1
        const int m0 = (wm * MT + mt) * 32 + 8 * qd + hsel;
        const int i0 = m0 / TW;
        float mx = fmaf(acc[t][4 * qd], a.ub, b);
        mx = fmaxf(mx, fmaf(acc[t][4 * qd + 1], a.ub, b));
        mx = fmaxf(mx, fmaf(acc[t][4 * qd + 2], a.ub, b));
        mx = fmaxf(mx, fmaf(acc[t][4 * qd + 3], a.ub, b));
        mx += fmaf(sacc[sp][4 * mt + qd], a.us, bsc);
        a.y[((clip[sp] * (H / 2) + i0 / 2) * (W / 2) + w0[sp] / 2) * C + co] = mx;
      }
    }
  }
  if (!(rmax < SPLIT_MAX) && a.range_flag) *a.range_flag = 1;
}

template <int H, int W, int CIN, int C, int TW, bool POOL, bool DBUF, int LA, int LB>
hipError_t launch(const OduArgs& a, hipStream_t s) {
  constexpr int TLW = (W + TW - 1) / TW;
  const int64_t blocks = ((int64_t)a.n * TLW + NS - 1) / NS;
  hipLaunchKernelGGL((odw_kernel<H, W, CIN, C, TW, POOL, DBUF, LA, LB>), dim3((unsigned)blocks), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace

// the blocks that run faster here than on odu (rocprof, three alternating runs on one box, ms per
// 16 384-clip launch, odu -> odw): block 7 14.19 -> 13.47, blocks 8-9 5.70 -> 5.35.
// Blocks 4 and 5-6 fit as well (218 / 238 VGPRs, 76.6 / 79.5 KB) but lose four and three workgroups
// per CU for two: 15.46 -> 15.57 and 6.49 -> 6.65, so they stay on odu and are not instantiated
bool odw_supported(int h, int w, int cin, int c, bool pool) {
  return (h == 32 && w == 38 && cin == 64 && c == 128 && pool) ||   // block 7
         (h == 16 && w == 19 && cin == 128 && c == 128 && !pool);   // blocks 8-9
}

hipError_t odw_launch(const OduArgs& a, int h, int w, int cin, int c, bool pool, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  if (!a.x || !a.y || a.x == a.y || !odw_supported(h, w, cin, c, pool) ||
      (pool && (!a.wsh || !a.wsl || !a.bs)))
    return hipErrorInvalidValue;
  // block 7 keeps odu's two halo buffers per strip (78 336 B, 248 VGPRs).  Blocks 8-9 would need
  // 82 944 B with them, 1 KB past two workgroups per CU: one buffer per strip (80 512 B, 236 VGPRs).
  // Operand pipeline depths (LA, LB): (1, 1) as in odu; (2, 2), (2, 1), (1, 2) are the same within
  // 0.02 ms, (1, 0) +0.1-0.15 ms, (0, 0) +0.3-0.4 ms
  if (pool) return launch<32, 38, 64, 128, 2, true, true, 1, 1>(a, s);
  return launch<16, 19, 128, 128, 4, false, false, 1, 1>(a, s);
}
