// OverlapDetection res_block (overlap_detector_temp.py:253-277) of the 64- and 128-channel stages as
// ONE kernel per block (blocks 1-3 run fused in resblk.hip):
//     t1 = Conv3x3(ELU(BN_in(x)))                      (GEMM a, K = 9 * cin)
//     t2 = Conv(4,1)(ELU(BN_mid(t1)))                  (GEMM b, K = 4 * c)
//     y  = x + t2                                      (blocks 5-6, 8-9)
//     y  = MaxPool2D(2, 'same')(t2) + Conv1x1/2(x)     (blocks 4, 7)
// The two conv_h3 launches it replaces write t1 to HBM (float32) and read it back with a halo, and the
// second re-reads x for the residual / shortcut.  Here a workgroup owns a FULL-HEIGHT strip of TW output
// columns of one clip: the conv(4,1) is vertical, so the strip's t1 is exactly its own H x TW pixels
// (no recomputed rows; Keras 'same' pads t1 with one zero row above and two below), held in LDS as
// BN_mid + ELU'd fp16 hi / lo next to nothing else -- it overlays the x halo GEMM a has finished with.
//
// Per strip: x halo (H + 2) x (TW + 2) staged in 32-channel chunks (BN_in + ELU + 2^4 + split, as
// conv_h3's staging), GEMM a as C^T = W^T X^T (a lane's accumulator quad = 4 consecutive channels of
// one pixel, so t1 goes back to LDS as 8-byte channel quads), t1 staged, GEMM b, epilogue:
//   * residual blocks: C^T again, bias + the raw x residual as float4 loads / stores;
//   * pool blocks (TW = 2): pixel rows in the accumulator, so a lane's register quad IS one 2x2 pool
//     window (rows i, i + 1 x columns 0, 1), and the shortcut Conv2D(1x1, stride 2) is a small 3xFP16
//     GEMM whose accumulator register 4 mt + q holds the window of main register quad (mt, q) --
//     its A row is that window's top-left input pixel (conv_h3's fused-shortcut trick).
//
// Bit-identical to the conv_h3 pair: the same staged operands (values, 2^4 scale, split), the same MFMA
// sequence per output element (32-channel chunks, then taps, then 16-channel k-steps; hi*lo, lo*hi,
// hi*hi into one accumulator -- C^T computes each element from the same products), the same epilogue
// arithmetic (fmaf(acc, unscale, bias), then + residual / max-pool + shortcut).  env MMLA_NO_ODU=1 at
// mmla_create runs the pair instead (tests/test_gpu_odu.py checks every block both ways).
//
// Strips per workgroup (NS).  With one strip each wave streams its share of the block's whole split
// weight set (147-852 KB) from L2 for 64 or 128 pixels: 35-184 GB per 16 384-clip launch through the
// vector-memory path, several times the launch's HBM traffic.  With NS = 2 workgroup b owns the
// logical strips 2 b and 2 b + 1 of the (clip-major, strip-minor) order, each with its own clip,
// column, buffer descriptor, x halo and t1 rows in LDS, and the tile loops of GEMM a, GEMM b and the
// shortcut GEMM run over both strips' tiles (tile t = strip * MT + mt): one loaded weight fragment
// pair (hi, lo) feeds 2 MT tiles, so the weight loads per MFMA halve.  The LDS doubles, so two
// workgroups share a CU (two waves per SIMD, 256 VGPRs each); blocks 7 and 8-9 gain by it
// (odu_two_strips), blocks 4 and 5-6 lose.  Per accumulator the product sequence does not depend on
// NS, and staging, the t1 write and the epilogue go strip by strip (the staging registers do not
// double), so both strip counts give the same bits.  A pair may straddle two clips; when n * strips
// is odd the last workgroup's second strip does not exist: its column is past the image and its
// descriptor has no records, so every load of it stages zeros (nothing enters the range maximum), and
// its stores are skipped.  env MMLA_NO_ODW=1 at mmla_create runs one strip per workgroup everywhere
// (tests/test_gpu_odw.py compares the two).
//
// LDS: the x halos keep their conflict-free layouts per strip.  The strips' t1 planes are stacked and
// share their zero rows (strip 0's two rows below the image double as strip 1's row above it):
//     row 0 | strip 0 rows 1 .. H | H + 1, H + 2 | strip 1 rows H + 3 .. 2 H + 2 | 2 H + 3, 2 H + 4
#include "f16x3.h"
#include "conv.h"
#include "odu.h"

namespace {

constexpr int CK = 32;                 // channel chunk (conv_h3's k order)
constexpr int KS = CK / 16;            // MFMA k-steps per chunk

// H x W image, CIN -> C channels, strips of TW columns, NS strips per workgroup, NW waves: WN = C / 32
// waves along the output channels (one 32-channel tile each, so no weight fragment is fetched twice
// per workgroup), WM along a strip's H * TW pixels, MT 32-pixel tiles per wave and strip
//
// LA (GEMM a), LB (GEMM b): the LDS operand pipeline.  A (tap, k-step, tile) group is two
// ds_read_b128 (hi, lo) and three MFMAs; its fragments are read LA groups ahead into LA + 1 register
// sets and every group is pinned as "the reads of group g + LA, then the MFMAs of group g"
// (pin_group), so a read has 3 LA MFMAs before its s_waitcnt.  Depth 0 reads a group's fragments
// right before its MFMAs and leaves the order to the scheduler (every MFMA triple then starts with an
// LDS round trip that only the SIMD's other waves can hide).
template <int H, int W, int CIN, int C, int TW, bool POOL, int NS, bool DBUF, int NW, int MINW, int LA, int LB>
__global__ void __launch_bounds__(64 * NW, MINW) odu_kernel(OduArgs a) {
  constexpr int NT = 64 * NW;
  constexpr int NB = LA + 1;                              // GEMM a's fragment register sets
  constexpr int WN = C / 32, WM = NW / WN;
  constexpr int M = H * TW;
  constexpr int MT = M / (WM * 32);
  constexpr int NTL = NS * MT;                            // tiles per wave
  static_assert(MT * WM * 32 == M && WN * WM == NW, "tiling");
  static_assert(!POOL || (TW == 2 && H % 2 == 0 && W % 2 == 0 && MT <= 4), "pool strips");
  static_assert(POOL || CIN == C, "residual blocks keep their width");
  constexpr int TLW = (W + TW - 1) / TW;
  constexpr int XP = TW + 2, XH = H + 2, NXP = XH * XP;   // x halo: rows -1 .. H, columns -1 .. TW
  // x halo layout, chosen so GEMM a's 16-lane ds_read_b128 groups (8 rows x 2 columns at TW 2, 4 x 4
  // at TW 4) hit 64 distinct banks (tools: the guide's lane groups, MI355X_MICROARCH.md section LDS):
  //   TW 2: 64-B pixels (no pad), 288-B rows, the two 16-B halves of each 32-B k-step swapped in odd
  //         halo columns -- conflict-free reads AND staging stores at 38 KB for block 4's halo, so its
  //         LDS plane (t1, 38.6 KB) admits four workgroups per CU (42.2 KB with 80-B pixels: three);
  //   TW 4: 80-B pixels (16-B pad), 576-B rows instead of 480 (2-way conflicts), same plane size.
  constexpr int LDX = TW == 2 ? CK : CK + 8;              // fp16 per staged x pixel
  constexpr int XRP = TW == 2 ? 144 : TW == 4 ? 288 : XP * LDX;   // fp16 per halo row
  constexpr bool XSW = TW == 2;                           // odd-column half swap
  constexpr int LDT = C + 8;                              // fp16 per t1 pixel
  constexpr int T1S = (H + 2) * TW * LDT;                 // strip s's t1 row r is plane row s (H + 2) + r
  constexpr int T1TOT = (NS * (H + 2) + 1) * TW * LDT;
  constexpr int NCHX = CIN / CK, NCH = C / CK;
  // DB: two halo buffers per strip, so chunk ch + 1 is loaded and staged right behind chunk ch's MFMAs
  // (which run on in the matrix pipe) instead of after a barrier; only where the second buffer fits
  // inside the LDS the t1 planes already hold (DBUF, see odu_launch)
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
  // the strips: clip, first column (past the image for a strip that does not exist, so its halo, t1
  // and residual all take their out-of-image paths) and the clip's input through a buffer descriptor:
  // out-of-image halo pixels read zeros with no branch around the load (a load inside a divergent
  // branch is waited for inside it).  One strip per workgroup always exists
  bool live[NS];
  int64_t clip[NS];
  int w0[NS];
  __amdgpu_buffer_rsrc_t rxc[NS];
#pragma unroll
  for (int sp = 0; sp < NS; ++sp) {
    const int64_t sid = (int64_t)bid * NS + sp;
    live[sp] = NS == 1 || sid < strips;
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

  int mpix[MT];   // the wave's pixels (C^T columns / pixel rows) in every strip: strip pixel m = i * TW + c
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) mpix[mt] = (wm * MT + mt) * 32 + (lane & 31);

  f32x16 acc[NTL];
#pragma unroll
  for (int t = 0; t < NTL; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;

  // ---- GEMM a: t1^T = Wa^T X^T over the halos, chunk by chunk --------------------------------------
  {
    const __amdgpu_buffer_rsrc_t rh = w_rsrc(a.wah), rl = w_rsrc(a.wal);
    constexpr size_t tap_stride = (size_t)C * CIN;
    const int q = tid % QPP;
    // XSW: this lane's k-half offset in an even / odd halo column (m % TW = lane & 1 at TW 2)
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
      // (one strip: the pin costs VGPRs and blocks 5-6 spill at their 168)
      if constexpr (NS > 1) asm volatile("" : "+v"(valid));
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
        bh[s] = w_frag(rh, (size_t)(ch * KS + s) * kstr, lofs);
        bl[s] = w_frag(rl, (size_t)(ch * KS + s) * kstr, lofs);
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
            nbh[s] = w_frag(rh, u, lofs);
            nbl[s] = w_frag(rl, u, lofs);
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
            if (g + LA < NG) pin_group<LA, 2>(); else pin_group<LA, 0>();
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
  // (conv_h3 writes fmaf(acc, unscale, bias) to HBM and the next launch stages BN + ELU + split of it;
  // columns past the image stage as zeros there, as here)
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
  // the zero rows: plane row 0 and the two below every strip (H + 1, H + 2, 2 H + 3, 2 H + 4)
  for (int e = tid; e < (2 * NS + 1) * TW * (LDT / 8); e += NT) {
    const int z = e / (LDT / 8), k8 = e - z * (LDT / 8);
    const int zr = z / TW;
    const int row = zr == 0 ? 0 : ((zr + 1) / 2) * (H + 2) - 1 + ((zr + 1) & 1);
    const int px = row * TW + (z - zr * TW);
    *reinterpret_cast<f16x8*>(lhi + px * LDT + 8 * k8) = f16x8{};
    *reinterpret_cast<f16x8*>(llo + px * LDT + 8 * k8) = f16x8{};
  }

  // residual blocks: the raw x at the wave's output pixels.  Strip 0's is loaded now, so GEMM b hides
  // the latency; a second strip's behind GEMM b, under strip 0's epilogue (both across GEMM b: 64 more
  // live registers, spills at the 256 cap)
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
    const __amdgpu_buffer_rsrc_t rh = w_rsrc(a.wbh), rl = w_rsrc(a.wbl);
    constexpr size_t tap_stride = (size_t)C * C;
#pragma unroll 1
    for (int ch = 0; ch < NCH; ++ch) {
      f16x8 bh[KS], bl[KS];
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        bh[s] = w_frag(rh, (size_t)(ch * KS + s) * kstr, lofs);
        bl[s] = w_frag(rl, (size_t)(ch * KS + s) * kstr, lofs);
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
            nbh[s] = w_frag(rh, u, lofs);
            nbl[s] = w_frag(rl, u, lofs);
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
            if (g + LB < NG) pin_group<LB, 2>(); else pin_group<LB, 0>();
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
#pragma unroll
    for (int sp = 1; sp < NS; ++sp) load_rsd(sp);   // under strip 0's epilogue
#pragma unroll
    for (int sp = 0; sp < NS; ++sp) {
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) {
        const int c0 = cob + 8 * qd + hsel;
        const float4 b4 = *reinterpret_cast<const float4*>(a.bb + c0);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const int t = sp * MT + mt;
          const int m = mpix[mt];
          const int i = m / TW, c = m % TW;
          if (w0[sp] + c >= W) continue;   // also every pixel of a strip that does not exist
          const float4 r = rsd[sp][mt][qd];
          float4 v = make_float4(fmaf(acc[t][4 * qd + 0], a.ub, b4.x), fmaf(acc[t][4 * qd + 1], a.ub, b4.y),
                                 fmaf(acc[t][4 * qd + 2], a.ub, b4.z), fmaf(acc[t][4 * qd + 3], a.ub, b4.w));
          v = make_float4(v.x + r.x, v.y + r.y, v.z + r.z, v.w + r.w);
          *reinterpret_cast<float4*>(a.y + ((clip[sp] * H + i) * W + w0[sp] + c) * C + c0) = v;
        }
      }
    }
  } else {
    // the shortcut Conv2D(1x1, stride 2): A row rho = window (mt = rho >> 3, quad q = rho & 3, lane
    // half (rho >> 2) & 1) of a strip's main tiles, i.e. its top-left input pixel; accumulator register
    // 4 mt + q of lane half h then holds main register quad (mt, q) of that half's window.  One weight
    // fragment pair feeds every strip
    f32x16 sacc[NS];
#pragma unroll
    for (int sp = 0; sp < NS; ++sp)
#pragma unroll
      for (int i = 0; i < 16; ++i) sacc[sp][i] = 0.0f;
    {
      const int rho = lane & 31;
      const int smt = rho >> 3, sq = rho & 3, sh = (rho >> 2) & 1;
      const int m0 = (wm * MT + (smt < MT ? smt : 0)) * 32 + 8 * sq + 4 * sh;
      const __amdgpu_buffer_rsrc_t rh = w_rsrc(a.wsh), rl = w_rsrc(a.wsl);
#pragma unroll
      for (int s = 0; s < CIN / 16; ++s) {
        // the k-step's weight fragments: ahead of the x loads where they feed two strips, behind them
        // with one (ahead: 136 VGPRs for 133 in block 7 and 0.6 % slower)
        f16x8 wh, wl;
        auto load_w = [&] {
          wh = w_frag(rh, (size_t)s * kstr, lofs);
          wl = w_frag(rl, (size_t)s * kstr, lofs);
        };
        if constexpr (NS > 1) load_w();
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
          if constexpr (NS == 1) load_w();
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

template <int H, int W, int CIN, int C, int TW, bool POOL, int NS, bool DBUF, int NW, int MINW, int LA, int LB>
hipError_t launch(const OduArgs& a, hipStream_t s) {
  constexpr int TLW = (W + TW - 1) / TW;
  const int64_t blocks = ((int64_t)a.n * TLW + NS - 1) / NS;
  hipLaunchKernelGGL((odu_kernel<H, W, CIN, C, TW, POOL, NS, DBUF, NW, MINW, LA, LB>), dim3((unsigned)blocks),
                     dim3(64 * NW), 0, s, a);
  return hipGetLastError();
}

}  // namespace

bool odu_supported(int h, int w, int cin, int c, bool pool) {
  return (h == 64 && w == 76 && cin == 32 && c == 64 && pool) ||    // block 4
         (h == 32 && w == 38 && cin == 64 && c == 64 && !pool) ||   // blocks 5-6
         (h == 32 && w == 38 && cin == 64 && c == 128 && pool) ||   // block 7
         (h == 16 && w == 19 && cin == 128 && c == 128 && !pool);   // blocks 8-9
}

bool odu_two_strips(int h, int w, int cin, int c, bool pool) {
  return (h == 32 && w == 38 && cin == 64 && c == 128 && pool) ||   // block 7
         (h == 16 && w == 19 && cin == 128 && c == 128 && !pool);   // blocks 8-9
}

hipError_t odu_launch(const OduArgs& a, int h, int w, int cin, int c, bool pool, int strips, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  if (!a.x || !a.y || a.x == a.y || (pool && (!a.wsh || !a.wsl || !a.bs)) ||
      !(strips == 1 ? odu_supported(h, w, cin, c, pool) : strips == 2 && odu_two_strips(h, w, cin, c, pool)))
    return hipErrorInvalidValue;
  // One strip.  Strips and register budgets, measured per kernel (rocprof, one box, per 16 384-clip
  // launch): blocks 5-6 TW 4 at 3 waves per SIMD (<= 168 VGPRs, 1 spilled) 8.56 -> 7.55 ms; TW 2 with
  // two-wave workgroups 8.16 ms; 4 waves per SIMD (<= 128 VGPRs) spill 20-44 VGPRs: block 7 15.5 ->
  // 17.2 ms, blocks 5-6 10.6 ms.  Blocks 4 and 8-9 are LDS-bound at 3 workgroups per CU (42 / 41 KB).
  // The second halo buffer (DBUF) only where it fits inside the t1 plane the LDS already holds
  // (blocks 7, 8-9; blocks 5-6 would drop to two workgroups per CU).
  // Operand pipeline depths (LA, LB): one group ahead pays 2.2-2.4 % in blocks 5-9
  // (168 / 133 / 165 VGPRs, no spills); block 4, with four waves per SIMD to cover its reads, gains
  // nothing from GEMM a's and would spill 5 VGPRs at its 128 cap with GEMM b's.
  if (strips == 1) {
    if (h == 64 && pool) return launch<64, 76, 32, 64, 2, true, 1, false, 4, 4, 0, 0>(a, s);
    if (h == 32 && c == 64) return launch<32, 38, 64, 64, 4, false, 1, false, 4, 3, 1, 1>(a, s);
    if (h == 32 && pool) return launch<32, 38, 64, 128, 2, true, 1, true, 4, 2, 1, 1>(a, s);
    return launch<16, 19, 128, 128, 4, false, 1, true, 4, 2, 1, 1>(a, s);
  }
  // Two strips, two workgroups per CU (rocprof, three alternating runs on one box, ms per 16 384-clip
  // launch, one strip -> two): block 7 14.19 -> 13.47, blocks 8-9 5.70 -> 5.35.
  // Blocks 4 and 5-6 fit as well (218 / 238 VGPRs, 76.6 / 79.5 KB) but lose four and three workgroups
  // per CU for two: 15.46 -> 15.57 and 6.49 -> 6.65, so they are not instantiated (odu_two_strips).
  // Block 7 keeps two halo buffers per strip (78 336 B, 248 VGPRs).  Blocks 8-9 would need 82 944 B
  // with them, 1 KB past two workgroups per CU: one buffer per strip (80 512 B).
  // Operand pipeline depths (LA, LB): (1, 1) as with one strip; (2, 2), (2, 1), (1, 2) are the same
  // within 0.02 ms, (1, 0) +0.1-0.15 ms, (0, 0) +0.3-0.4 ms
  if (pool) return launch<32, 38, 64, 128, 2, true, 2, true, 4, 2, 1, 1>(a, s);
  return launch<16, 19, 128, 128, 4, false, 2, false, 4, 2, 1, 1>(a, s);
}
