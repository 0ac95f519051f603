// The strip kernel of OD-NET res_blocks 1-3 (rbs.hip documents the algorithm), instantiated by rbs.hip,
// rbs_w1l.hip and rbs_tp.hip.  The including file defines, before the #include,
//   RBS_KERNEL  the kernel template's name in that translation unit, and
//   RBS_W1L     where GEMM 1 reads its split 3x3 weights: false: from global memory through a register
//               ring, every chunk (rbs.hip: block 1, and blocks 2-3 under MMLA_NO_RBS_W1L=1); true: from
//               an LDS copy the workgroup makes once per strip (rbs_w1l.hip).
//   RBS_TAILPAIR  (optional, default false; block 1 only: rbs_tp.hip) true: the grid is 9 n + ceil(n / 2)
//               workgroups instead of 10 n: the ragged tenth strips (7 of 16 columns in the image) of clips
//               2p and 2p + 1 share one workgroup, each in its own half of the halo ring and of the tile.
//               Only the column tables computed before the chunk loop differ (rbs_tp.hip has the map).
//   RBS_SC_DEDUP  (optional, default false; with RBS_TAILPAIR: rbs_tp.hip turns it on) true: the
//               shortcut's stem is computed once per pool window, two channels per lane of a quad, and
//               assembled by DPP broadcasts.
// The switches are macros and not template parameters so that rbs.hip's kernels keep their names and
// compile to the code they had as the only user of this body (a wrapper kernel around an inlined device
// function compiled to a different schedule and seven more VGPRs for blocks 2-3).
#pragma once
#include "f16x3.h"
#include "resblk.h"
#if !defined(RBS_KERNEL) || !defined(RBS_W1L)
#error "define RBS_KERNEL and RBS_W1L before including rbs_body.h"
#endif
#ifndef RBS_TAILPAIR
#define RBS_TAILPAIR false
#endif
#ifndef RBS_SC_DEDUP
#define RBS_SC_DEDUP false
#endif

namespace {

constexpr int NT = 256;            // 4 waves
constexpr int TW = 16;             // strip width (output columns)
constexpr int R = 8;               // output rows per chunk (4 waves x 2 rows)
constexpr int C = 32;              // output channels of blocks 1-3
#ifndef RBS_TRACE
#define RBS_TRACE 0
#endif
#if RBS_TRACE
// dev timeline (RBS_TRACE builds only): s_memtime at 8 phase points of chunks 2..5, waves 0-3, of the
// first 2048 workgroups of each launch (the last launch wins)
__device__ unsigned long long rbs_trace_buf[2048 * 4 * 4 * 8];
#define RBS_T(i) do { if (bid < 2048 && k >= 2 && k < 6) tt[i] = __builtin_amdgcn_s_memtime(); } while (0)
#define RBS_TFLUSH() do { if (bid < 2048 && k >= 2 && k < 6 && lane == 0) { for (int i_ = 0; i_ < 8; ++i_) rbs_trace_buf[(((size_t)bid * 4 + wave) * 4 + (k - 2)) * 8 + i_] = tt[i_]; } } while (0)
#else
#define RBS_T(i) do { } while (0)
#define RBS_TFLUSH() do { } while (0)
#endif

template <int H, int W, int CIN, bool POOL>
struct SG {
  static constexpr int XW = TW + 2;                     // halo columns w0 - 1 .. w0 + 16
  static constexpr int XRING = R + 2, TRING = R + 3;    // ring rows
  static constexpr int XROW = XW * CIN;                 // halfs per x ring row: 1152 / 576 B
  static constexpr int XPLANE = XRING * XROW;
  static constexpr int TROW = TW * C;                   // 512 halfs = 1024 B
  static constexpr int TPLANE = TRING * TROW;
  static constexpr int NCHUNK = H / R;
  static constexpr int STRIPS = (W + TW - 1) / TW;
  static constexpr int QPP = CIN / 4;                   // channel quads per pixel
  static constexpr int MAXT = (R * XW * QPP + NT - 1) / NT;      // staging tasks per thread, chunk
  static constexpr int MAXT0 = (4 * XW * QPP + NT - 1) / NT;     // the prologue's 4 rows
  static constexpr int KPT = CIN / 16;                  // 16-deep k-steps per tap
  static constexpr int KS1 = 9 * KPT, KS2 = 8;
  // block 1 keeps GEMM 2's weights in LDS (sw2; 51 KB in all) to fit the registers of 3 workgroups per CU;
  // blocks 2-3 keep them in registers at 2 (measured: deeper weight prefetch does not pay; LDS-resident GEMM 1
  // weights do where they cost no workgroup, i.e. in blocks 2-3: RBS_W1L)
  static constexpr bool W2L = CIN == 16;                // GEMM 2's weights in LDS
  // ... where a GEMM 2 k-step reads four fragments from LDS (t1 and sw2, hi and lo).  Those of step
  // s + 1 go to a second register set and each k-step is pinned as "the reads for step s + 1, then
  // the three MFMAs of step s" (pin_group<1, NR>), so a ds_read_b128 has 3 MFMAs (96 cycles) before its
  // s_waitcnt; left to the scheduler, a source-order prefetch shares registers between the two steps
  // and issues the reads after the first or second MFMA.  Block 1's GEMM 2: 1 540 -> 1 370 cycles per
  // chunk.  GEMM 1 of either kernel and blocks 2-3's GEMM 2 (two reads per step) do not gain from the
  // same pinning and keep the source-order prefetch
  static constexpr int MINB = CIN == 16 ? 3 : 2;        // resident workgroups per CU
  static constexpr int PF = 3;                          // GEMM 1 weight k-steps in flight
  static constexpr int PD = CIN == 16 ? 1 : 2;                      // input prefetch distance (chunks)
  static_assert(H % R == 0, "geometry");
  static_assert(NT % QPP == 0, "a thread's channel quad is fixed");
  static_assert(XROW <= 1024 && W * CIN * 4 < 65536 && W * 12 < 65536, "staging task fields");
};

// the x ring: pixel (row r, halo column x), 16-B channel group g -> half offset in a plane
// (rows unpadded: 72 / 36 16-B units; the swizzle keeps GEMM 1's ds_read_b128 conflict-free for
// every tap, both lane halves and either row parity -- searched against the guide's lane groups)
template <int CIN>
MMLA_DEV int xoff(int slot, int x, int g) {
  constexpr int XROW = (TW + 2) * CIN;
  const int f = CIN == 32 ? ((x >> 1) & 3) : ((x >> 1) & 1);
  return slot * XROW + x * CIN + 8 * (g ^ f);
}
// the t1 ring: pixel (row j, column c), channel group g (4 per pixel)
template <bool POOL>
MMLA_DEV int toff(int slot, int j, int c, int g) {
  const int f = POOL ? (((c >> 2) ^ (2 * (j & 1))) & 3) : ((c >> 2) & 3);
  return slot * (TW * C) + c * C + 8 * (g ^ f);
}

// one strip per workgroup: NT threads, SG::STRIPS workgroups per clip
template <int H, int W, int CIN, bool POOL, bool STEM>
__global__ void __launch_bounds__(NT, (SG<H, W, CIN, POOL>::MINB)) RBS_KERNEL(ResBlkArgs a) {
  using G = SG<H, W, CIN, POOL>;
  constexpr bool W1L = RBS_W1L;
  static_assert(!STEM || (CIN == 16 && POOL), "the stem feeds block 1");
  static_assert(POOL || CIN == C, "residual blocks keep their width");
  static_assert(!W1L || G::MINB == 2, "LDS-resident GEMM 1 weights: two workgroups per CU");
  // GEMM 1's k-steps whose weights are LDS-resident (W1L): all 18 are 896 B more than half a CU's LDS
  // holds beside the rings, so the last one stays in registers for the strip (KS1 - KS1L fragments)
  constexpr int KS1L = W1L ? G::KS1 - 1 : 0;
  static_assert(!W1L || 4 * (G::XPLANE + G::TPLANE + KS1L * 512) + 3 * C * 4 <= 160 * 1024 / 2, "LDS of two workgroups");
  __shared__ __attribute__((aligned(16))) _Float16 sx[2 * G::XPLANE];   // x ring: hi plane, lo plane
  __shared__ __attribute__((aligned(16))) _Float16 st[2 * G::TPLANE];   // t1 ring: hi plane, lo plane
  // per-channel parameters: [0] 16 s2 u1, [1] 16 (b1 s2 + t2), [2] b2 (+ stem {w_r, w_g, w_b, b} rows)
  __shared__ float4 spar[3 * C / 4 + (STEM ? 16 : 0)];
  // GEMM 2's weights in fragment order (W2L): [k-step][lane][8] hi, then lo
  __shared__ __attribute__((aligned(16))) _Float16 sw2[G::W2L ? 2 * G::KS2 * 512 : 8];
  // GEMM 1's weights in fragment order (W1L): [k-step < KS1L][lane][8] hi, then lo
  __shared__ __attribute__((aligned(16))) _Float16 sw1[W1L ? 2 * KS1L * 512 : 8];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5;                       // lane half: k group / channel group
  const uint32_t bid = xcd_block_id();
  constexpr bool TP = RBS_TAILPAIR, SCD = RBS_SC_DEDUP;
  static_assert(!TP || (STEM && W % TW == TW / 2 - 1), "paired tails: block 1, two 7-column tails in one strip");
  static_assert(!SCD || TP, "the de-duplicated shortcut stem belongs to the paired-tails kernel");
  // TP: workgroups 0 .. FS n - 1 are the full strips (clip bid / FS, strip bid % FS); workgroup FS n + p is
  // the tails of clips 2p (part 0: ring columns 0-8, tile columns 0-7) and 2p + 1 (part 1: ring columns
  // 9-17, tile columns 8-15; absent, has_b false, when n is odd and p the last pair).  All wave-uniform.
  constexpr int FS = TP ? G::STRIPS - 1 : G::STRIPS;
  const bool pair = TP && bid >= (uint32_t)a.n * FS;
  const int clip = pair ? 2 * (int)(bid - (uint32_t)a.n * FS) : (int)(bid / FS);
  const int w0 = pair ? FS * TW : (int)(bid - (uint32_t)clip * FS) * TW;
  const bool has_b = pair && clip + 1 < a.n;
  // ring column x (0 .. 17) -> its part and image column; false: outside the image (or of the absent clip)
  auto ring_col = [&](int x, int& part, int& iw) -> bool {
    part = TP && pair && x >= G::XW / 2;
    iw = w0 - 1 + x - (TP ? part * (G::XW / 2) : 0);
    return iw >= 0 && iw < W && (!TP || !part || has_b);
  };
  const int lofs = lane * 8;
  float rmax = 0.0f;   // 3xFP16 range guard: the largest |operand| this thread split (ResBlkArgs::range_flag)

  // ---- parameters -------------------------------------------------------------------------------
  float* const sp = reinterpret_cast<float*>(spar);
  if (tid < C) {
    const float s2 = a.s2[tid];
    sp[tid] = 16.0f * (s2 * a.u1);
    sp[C + tid] = 16.0f * fmaf(a.b1[tid], s2, a.t2[tid]);
    sp[2 * C + tid] = a.b2[tid];
  }
  if constexpr (STEM) {
    if (tid < 64) {   // [co][k]: k < 3 the r, g, b weights, k = 3 the bias (od_stem_kernel's operands)
      const int co = tid >> 2, k = tid & 3;
      sp[3 * C + tid] = k < 3 ? a.wst[k * a.ldst + co] : a.bst[co];
    }
  }
  // GEMM 2's weights (8 k-steps, hi / lo) stay in registers for the whole strip: GEMM 2 then issues no
  // vector loads, so the next chunk's input loads can be in flight across it (vector loads complete
  // in issue order: a weight load behind them would wait for HBM)
  const __amdgpu_buffer_rsrc_t rw1h = w_rsrc(a.w1h), rw1l = w_rsrc(a.w1l);
  f16x8 w2h[G::W2L ? 1 : G::KS2], w2l[G::W2L ? 1 : G::KS2];
  if constexpr (G::W2L) {
    for (int e = tid; e < 2 * G::KS2 * 64; e += NT) {   // 16-B pieces
      const int pl = e / (G::KS2 * 64), i = e - pl * (G::KS2 * 64);
      *reinterpret_cast<f16x8*>(sw2 + 8 * e) = *reinterpret_cast<const f16x8*>((pl ? a.w2l : a.w2h) + 8 * i);
    }
  } else {
    const __amdgpu_buffer_rsrc_t rw2h = w_rsrc(a.w2h), rw2l = w_rsrc(a.w2l);
#pragma unroll
    for (int s = 0; s < G::KS2; ++s) {
      w2h[s] = w_frag(rw2h, s * 512, lofs);
      w2l[s] = w_frag(rw2l, s * 512, lofs);
    }
  }
  // W1L: the workgroup's copy of GEMM 1's weights (already contiguous in fragment order), issued here
  // so that it overlaps the prologue's staging loads; its first reader is behind the prologue's barrier
  f16x8 w1th[W1L ? G::KS1 - KS1L : 1], w1tl[W1L ? G::KS1 - KS1L : 1];   // the k-steps that did not fit
  if constexpr (W1L) {
    for (int e = tid; e < 2 * KS1L * 64; e += NT) {   // 16-B pieces
      const int pl = e / (KS1L * 64), i = e - pl * (KS1L * 64);
      *reinterpret_cast<f16x8*>(sw1 + 8 * e) = *reinterpret_cast<const f16x8*>((pl ? a.w1l : a.w1h) + 8 * i);
    }
#pragma unroll
    for (int s = KS1L; s < G::KS1; ++s) {
      w1th[s - KS1L] = w_frag(rw1h, s * 512, lofs);
      w1tl[s - KS1L] = w_frag(rw1l, s * 512, lofs);
    }
  }
  f16x8 wsh_, wsl_;   // block 1's shortcut weights
  if constexpr (POOL) {
    wsh_ = w_frag(w_rsrc(a.wsh), 0, lofs);
    wsl_ = w_frag(w_rsrc(a.wsl), 0, lofs);
  }
  // this thread's staging quad: BN1 x 2^4 (exact); block 1: folded into the stem weights
  const int q = tid % G::QPP;
  float bnw[4][4];   // blocks 2-3: [c] = {16 s1, 16 t1}; block 1: [c] = 16 s1 {w_r, w_g, w_b} , 16 (s1 b + t1)
  __syncthreads();   // spar
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float s16 = 16.0f * a.s1[4 * q + c], t16 = 16.0f * a.t1[4 * q + c];
    if constexpr (STEM) {
      const float4 v = spar[3 * C / 4 + 4 * q + c];
      bnw[c][0] = s16 * v.x;
      bnw[c][1] = s16 * v.y;
      bnw[c][2] = s16 * v.z;
      bnw[c][3] = fmaf(s16, v.w, t16);
    } else {
      bnw[c][0] = s16;
      bnw[c][1] = t16;
    }
  }

  // ---- staging: task j of this thread = (pixel, quad) of the chunk's R x 18 new halo pixels --------
  // source: a per-clip buffer, so rows / columns outside the image read zeros with no branches
  // (offsets past the clip or negative, wrapped, are out of range)
  constexpr uint32_t ROWB = STEM ? 0u : (uint32_t)W * CIN * 4;
  const __amdgpu_buffer_rsrc_t rx = STEM ? w_rsrc(nullptr) :
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x) + (int64_t)clip * H * W * CIN, (short)0,
                                        (int)(H * ROWB), 0x00020000);
  // block 1: the clip's image (u8 or float NHWC) through a buffer descriptor as well
  // (TP: a pair's two clips are contiguous and share one descriptor; part 1's pixels start H W pixels
  // in.  Rows -1 and >= H of a part are then no longer out of range, so whoever loads them masks by row:
  // load_src by its own test, the last chunk's staging by r0 + rr < H)
  const bool im8 = STEM && a.img8 != nullptr;
  const __amdgpu_buffer_rsrc_t rimg = !STEM ? w_rsrc(nullptr) :
      __builtin_amdgcn_make_buffer_rsrc(im8 ? (void*)(a.img8 + (int64_t)clip * H * W * 3)
                                            : (void*)(a.imgf + (int64_t)clip * H * W * 3),
                                        (short)0, TP ? __builtin_amdgcn_readfirstlane((int)(H * W * 3 * (im8 ? 1 : 4)) * (has_b ? 2 : 1))
                                                     : (int)(H * W * 3 * (im8 ? 1 : 4)), 0x00020000);
  // per task: LDS column offset (bits 0-9), tile row (10-13), column inside the image (14), task exists
  // (15), its source byte offset within a row (16-31)
  // (TP: the source offset, which then includes part 1's clip, has a register of its own: tsrc)
  uint32_t tinfo[G::MAXT];
  uint32_t tsrc[TP ? G::MAXT : 1];
#pragma unroll
  for (int j = 0; j < G::MAXT; ++j) {
    const int t = tid + j * NT;
    const int px = t / G::QPP;
    const int rr = px / G::XW, x = px - rr * G::XW;
    int part, iw;
    const bool col_ok = ring_col(x, part, iw);
    const uint32_t tc = !col_ok ? 0u : STEM ? (uint32_t)iw * (a.img8 ? 3u : 12u) : (uint32_t)(iw * CIN + 4 * q) * 4u;
    if constexpr (TP) tsrc[j] = tc + (uint32_t)(part * H * W) * (a.img8 ? 3u : 12u);
    tinfo[j] = (uint32_t)(xoff<CIN>(0, x, q >> 1) + 4 * (q & 1)) | ((uint32_t)(rr & 15) << 10) |
               ((uint32_t)col_ok << 14) | ((uint32_t)(rr < R) << 15) | ((TP ? 0u : tc) << 16);
  }
  // the image pixel {r, g, b, 1} (1: inside the image), or x channels 4q .. 4q+3
  // (no branch around a load: a load inside a divergent branch is waited for inside it; the raw image
  // bytes are converted where they are used)
  auto load_src = [&](int ih, int iw, bool col_ok, int part = 0) -> float4 {
    if constexpr (STEM) {
      const int pix = TP ? (part * H + ih) * W + iw : ih * W + iw;
      const bool ok = col_ok && ih >= 0 && ih < H;
      if (im8) {
        const uint32_t off = ok ? (uint32_t)pix * 3u : 0x80000000u;
        const uint32_t r = __builtin_amdgcn_raw_buffer_load_b8(rimg, off, 0, 0);
        const uint32_t g = __builtin_amdgcn_raw_buffer_load_b8(rimg, off + 1u, 0, 0);
        const uint32_t b = __builtin_amdgcn_raw_buffer_load_b8(rimg, off + 2u, 0, 0);
        return make_float4(__builtin_bit_cast(float, r), __builtin_bit_cast(float, g), __builtin_bit_cast(float, b), 0.f);
      }
      const uint32_t off = ok ? (uint32_t)pix * 12u : 0x80000000u;
      return make_float4(__builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rimg, off, 0, 0)),
                         __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rimg, off + 4u, 0, 0)),
                         __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rimg, off + 8u, 0, 0)), 0.f);
    } else {
      const uint32_t off = col_ok ? (uint32_t)ih * ROWB + (uint32_t)(iw * CIN + 4 * q) * 4u : 0x80000000u;
      return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rx, off, 0, 0));
    }
  };
  // a loaded image pixel as floats
  auto img_px = [&](float4 v) -> float4 {
    if (im8)
      return make_float4((float)__builtin_bit_cast(uint32_t, v.x), (float)__builtin_bit_cast(uint32_t, v.y),
                         (float)__builtin_bit_cast(uint32_t, v.z), 0.f);
    return v;
  };
  // task j's 4 channels at x row r0 + its tile row (rows outside the image: the wrapped or past-the-end
  // row offset is out of range, as in load_src)
  auto load_task = [&](int r0, int j) -> float4 {
    const uint32_t ti = tinfo[j];
    const uint32_t off = (ti >> 14) & 1u ? (uint32_t)((r0 + (int)((ti >> 10) & 15)) * (STEM ? W * 3 * (im8 ? 1 : 4) : (int)ROWB)) +
                                               (TP ? tsrc[TP ? j : 0] : ti >> 16)
                                         : 0x80000000u;
    if constexpr (STEM) {
      if (im8) {
        const uint32_t r = __builtin_amdgcn_raw_buffer_load_b8(rimg, off, 0, 0);
        const uint32_t g = __builtin_amdgcn_raw_buffer_load_b8(rimg, off + 1u, 0, 0);
        const uint32_t b = __builtin_amdgcn_raw_buffer_load_b8(rimg, off + 2u, 0, 0);
        return make_float4(__builtin_bit_cast(float, r), __builtin_bit_cast(float, g), __builtin_bit_cast(float, b), 0.f);
      }
      return make_float4(__builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rimg, off, 0, 0)),
                         __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rimg, off + 4u, 0, 0)),
                         __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rimg, off + 8u, 0, 0)), 0.f);
    } else {
      return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rx, off, 0, 0));
    }
  };
  // BN1 + ELU (+ the stem) + split of one task's 4 channels at x row ih, into the x ring at lds
  // BN1 + ELU (+ the stem) + split of one task's 4 channels into the x ring at half offset o; MASK:
  // zero unless `in` (the 3x3 conv's padding rows; padding columns are zeroed once, see below)
  auto stage4 = [&](int o, bool in, float4 v, auto MASK_) {
    constexpr bool MASK = decltype(MASK_)::value;
    if constexpr (STEM) {
      // a float image is a caller's input: a NaN / inf pixel flags the launch here (f16x3.h nonfinite3;
      // every pixel of the image is staged by some strip, the shortcut re-reads staged pixels).  u8
      // pixels are finite: the test is behind the wave-uniform im8
      if (!im8 && (!MASK || in) && nonfinite3(v.x, v.y, v.z)) rmax = SPLIT_MAX;
      v = img_px(v);
    }
    float u[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if constexpr (STEM) {   // 16 BN1(stem(x)) with the BN folded into the stem weights
        float acc = v.x * bnw[c][0];
        acc = fmaf(v.y, bnw[c][1], acc);
        acc = fmaf(v.z, bnw[c][2], acc);
        u[c] = acc + bnw[c][3];
      } else {
        u[c] = fmaf((&v.x)[c], bnw[c][0], bnw[c][1]);
      }
    }
    float e[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) e[c] = (!MASK || in) ? elu16(u[c]) : 0.0f;
    rmax = fmaxf(rmax, amax4(e[0], e[1], e[2], e[3]));
    f16x4 hv, lv;
    split4(e[0], e[1], e[2], e[3], hv, lv);
    *reinterpret_cast<f16x4*>(sx + o) = hv;
    *reinterpret_cast<f16x4*>(sx + G::XPLANE + o) = lv;
  };
  // a chunk's task j: rows r0 .. r0 + 7; tasks on a column outside the image do nothing (their ring
  // column stays zero); rows past the image only occur in the last chunk (MASK)
  auto stage_task = [&](int r0, int j, float4 v, auto MASK_) {
    const uint32_t ti = tinfo[j];
    if (((ti >> 14) & 3u) != 3u) return;   // task exists and its column is inside the image
    const int rr = (int)((ti >> 10) & 15);
    uint32_t slot = (uint32_t)((r0 + 1) % G::XRING) + (uint32_t)rr;   // (r0 + 1) % XRING: scalar
    slot = min(slot, slot - (uint32_t)G::XRING);
    stage4((int)slot * G::XROW + (int)(ti & 1023), r0 + rr < H, v, MASK_);
  };
  // the ring's columns outside the image (strip 0: image column -1; the last strip: columns >= W),
  // zeroed once in every slot and both planes: no task writes them (TP, a pair: ring columns 8 and 17,
  // image column W of either part, and all of an absent part 1)
  for (int e = tid; e < 2 * G::XRING * G::XW * G::QPP; e += NT) {
    const int pl = e / (G::XRING * G::XW * G::QPP), r = e - pl * (G::XRING * G::XW * G::QPP);
    const int slot = r / (G::XW * G::QPP), x = (r / G::QPP) % G::XW, qq = r % G::QPP;
    int part, iw;
    if (!ring_col(x, part, iw))
      *reinterpret_cast<f16x4*>(sx + pl * G::XPLANE + xoff<CIN>(slot, x, qq >> 1) + 4 * (qq & 1)) = f16x4{};
  }
  // ---- GEMM 1 for t1 rows j0, j0 + 1 (one 32-pixel tile, natural order: pixel n = lane & 31 is row
  //      j0 + (n >> 4), column n & 15) as t1^T: acc[4 jj + i] = channel 8 jj + 4 h + i of pixel n ----
  const int n = lane & 31, nr = n >> 4, nc = n & 15;
  // this lane's x column offsets for dx = 0..2 and its k groups (ks): ring column nc + dx.  TP, a pair:
  // part 1's tile columns 8-14 read ring columns nc + 1 + dx (its ring half starts at 9, its tile half
  // at the even column 8 so that its pool windows stay aligned), and the junk tile columns 7 and 15 read
  // the zero ring column of their own part (8, 17) for every dx, so that no lane of one part reads a
  // ring column of the other and a junk column's t1 is what a column outside the image gives
  auto tile_ring = [&](int c, int dx) -> int {
    if (!(TP && pair)) return c + dx;
    const int p = c >= TW / 2, cl = c - p * (TW / 2);
    return p * (G::XW / 2) + (cl == TW / 2 - 1 ? G::XW / 2 - 1 : cl + dx);
  };
  int xco[3][G::KPT];
#pragma unroll
  for (int dx = 0; dx < 3; ++dx)
#pragma unroll
    for (int ks = 0; ks < G::KPT; ++ks) xco[dx][ks] = xoff<CIN>(0, tile_ring(nc, dx), G::KPT == 2 ? 2 * ks + h : h);

  // GEMM 1's weight ring (PF k-steps ahead), first steps issued early; W1L: no loads, the fragments
  // come from sw1 one k-step ahead like the x fragments
  f16x8 w1h[W1L ? 1 : G::PF], w1l[W1L ? 1 : G::PF];
  auto gemm1_issue = [&]() {
    if constexpr (!W1L) {
#pragma unroll
      for (int s = 0; s < G::PF; ++s) {
        w1h[s] = w_frag(rw1h, s * 512, lofs);
        w1l[s] = w_frag(rw1l, s * 512, lofs);
      }
    }
  };
  auto gemm1 = [&](int j0) -> f32x16 {
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    int xr[3];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {   // x row j - 1 + dy: ring slot (j0 % XRING: scalar) + nr + dy, wrapped
      const uint32_t sl = (uint32_t)(j0 % G::XRING) + (uint32_t)(nr + dy);
      xr[dy] = (int)min(sl, sl - (uint32_t)G::XRING) * G::XROW;
    }
    // the x fragments one k-step ahead (an LDS read's latency would otherwise sit before every
    // step's MFMAs)
    auto xo = [&](int s) {
      const int tap = s / G::KPT, ks = s % G::KPT;
      return xr[tap / 3] + xco[tap % 3][ks];
    };
    f16x8 nxh = *reinterpret_cast<const f16x8*>(sx + xo(0));
    f16x8 nxl = *reinterpret_cast<const f16x8*>(sx + G::XPLANE + xo(0));
    f16x8 nbh, nbl;   // W1L: the next step's weight fragments (lane * 16 B: linear, conflict-free)
    if constexpr (W1L) {
      nbh = *reinterpret_cast<const f16x8*>(sw1 + lofs);
      nbl = *reinterpret_cast<const f16x8*>(sw1 + KS1L * 512 + lofs);
    }
#pragma unroll
    for (int s = 0; s < G::KS1; ++s) {
      f16x8 bh, bl;
      if constexpr (W1L) {
        bh = s < KS1L ? nbh : w1th[s < KS1L ? 0 : s - KS1L];
        bl = s < KS1L ? nbl : w1tl[s < KS1L ? 0 : s - KS1L];
        if (s + 1 < KS1L) {
          nbh = *reinterpret_cast<const f16x8*>(sw1 + (s + 1) * 512 + lofs);
          nbl = *reinterpret_cast<const f16x8*>(sw1 + (KS1L + s + 1) * 512 + lofs);
        }
      } else {
        bh = w1h[s % G::PF];
        bl = w1l[s % G::PF];
        if (s + G::PF < G::KS1) {
          w1h[s % G::PF] = w_frag(rw1h, (s + G::PF) * 512, lofs);
          w1l[s % G::PF] = w_frag(rw1l, (s + G::PF) * 512, lofs);
        }
      }
      const f16x8 xh = nxh, xl = nxl;
      if (s + 1 < G::KS1) {
        nxh = *reinterpret_cast<const f16x8*>(sx + xo(s + 1));
        nxl = *reinterpret_cast<const f16x8*>(sx + G::XPLANE + xo(s + 1));
      }
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(bl, xh, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh, xl, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh, xh, acc, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);   // keep the register footprint: no deeper hoisting
    }
    return acc;
  };
  // BN2(acc u1 + b1) + ELU + split -> t1 ring rows j0 + nr; rows past the image are the (4,1) conv's
  // zero padding (j0 is even and so is H: both rows of a wave are inside or both outside)
  auto t1_write = [&](int j0, const f32x16& acc) {
    const int j = j0 + nr;
    const uint32_t sl = (uint32_t)((j0 + 1) % G::TRING) + (uint32_t)nr;   // (j + 1) % TRING
    const int slot = (int)min(sl, sl - (uint32_t)G::TRING);
    if (j0 < H) {
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int c0 = 8 * jj + 4 * h;
        const float4 sv = spar[c0 / 4], cv = spar[C / 4 + c0 / 4];
        float e[4];
        e[0] = elu16(fmaf(acc[4 * jj + 0], sv.x, cv.x));
        e[1] = elu16(fmaf(acc[4 * jj + 1], sv.y, cv.y));
        e[2] = elu16(fmaf(acc[4 * jj + 2], sv.z, cv.z));
        e[3] = elu16(fmaf(acc[4 * jj + 3], sv.w, cv.w));
        rmax = fmaxf(rmax, amax4(e[0], e[1], e[2], e[3]));
        f16x4 hv, lv;
        split4(e[0], e[1], e[2], e[3], hv, lv);
        const int o = toff<POOL>(slot, j, nc, jj) + 4 * h;
        *reinterpret_cast<f16x4*>(st + o) = hv;
        *reinterpret_cast<f16x4*>(st + G::TPLANE + o) = lv;
      }
    } else {
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int o = toff<POOL>(slot, j, nc, jj) + 4 * h;
        *reinterpret_cast<f16x4*>(st + o) = f16x4{};
        *reinterpret_cast<f16x4*>(st + G::TPLANE + o) = f16x4{};
      }
    }
  };

  // ---- prologue: x rows -1 .. 2, t1 rows 0, 1 (wave 0) and the zero t1 row -1 --------------------
  {
    constexpr int T0 = 4 * G::XW * G::QPP;
#pragma unroll
    for (int j = 0; j < G::MAXT0; ++j) {
      const int t = tid + j * NT;
      const int px = t / G::QPP;
      const int rr = px / G::XW, x = px - rr * G::XW;
      const int ih = rr - 1;
      int part, iw;
      const bool col_ok = ring_col(x, part, iw);
      const float4 v = load_src(ih, iw, col_ok, part);
      if (t < T0 && col_ok)
        stage4(xoff<CIN>((ih + 1) % G::XRING, x, q >> 1) + 4 * (q & 1), ih >= 0, v, std::true_type{});
    }
    for (int e = tid; e < 2 * G::TROW / 8; e += NT)   // t1 row -1 (slot 0), both planes
      *reinterpret_cast<f16x8*>(st + (e >= G::TROW / 8 ? G::TPLANE - G::TROW : 0) + 8 * e) = f16x8{};
  }
  __syncthreads();
  if (wave == 0) {
    gemm1_issue();
    const f32x16 acc = gemm1(0);
    t1_write(0, acc);
  }
  // the new rows of chunk k, loaded G::PD chunks ahead (blocks 2-3: two, in preA for even k and preB
  // for odd k, so a whole chunk of work stands between a load and its use; block 1, whose register
  // budget is three workgroups per CU: one)
  float4 preA[G::MAXT], preB[G::PD == 2 ? G::MAXT : 1];
#pragma unroll
  for (int j = 0; j < G::MAXT; ++j) preA[j] = load_task(3, j);
  if constexpr (G::PD == 2) {
#pragma unroll
    for (int j = 0; j < G::MAXT; ++j) preB[j] = load_task(3 + R, j);
  }
  __syncthreads();   // wave 0 is done with x rows -1, 0 (the first chunk overwrites their slots)

  // block 1's shortcut pixel of a chunk: this lane's pool window's top-left, conv row 8 k + 2 wave
  // (TP, a pair: windows 4-7 are part 1's, at the same image columns as windows 0-3; sc_ok: inside the
  // image, and of a clip that exists)
  const int win = n >> 2;
  const int sc_part = TP && pair && win >= 4;
  const int sc_col = w0 + 2 * (win - 4 * sc_part);
  const bool sc_ok_tp = sc_col < W && (!sc_part || has_b);
  auto sc_ok = [&]() -> bool {
    if constexpr (TP) return sc_ok_tp; else return sc_col < W;
  };
  // its shortcut bias, read once: a global load inside the chunk loop would queue behind the next
  // chunk's image prefetch (vector loads complete in issue order)
  float bsc = 0.0f;
  if constexpr (POOL) bsc = a.bs[n];

#if RBS_TRACE
  unsigned long long tt[8];
#endif
  static_assert(G::NCHUNK % 2 == 0, "chunk pairs");
  auto chunk = [&](const int k, float4* pre) {
    RBS_T(0);
    const int rx0 = R * k + 3;            // the chunk's new x rows rx0 .. rx0 + 7
    const int j0 = R * k + 2 + 2 * wave;  // this wave's t1 rows (GEMM 1)
    const int o0 = R * k + 2 * wave;      // this wave's output rows (GEMM 2)
    // ---- stage the new x rows, start GEMM 1's weight stream ------------------------------------
    if (k + 1 < G::NCHUNK) {
#pragma unroll
      for (int j = 0; j < G::MAXT; ++j) stage_task(rx0, j, pre[j], std::false_type{});
    } else {
#pragma unroll
      for (int j = 0; j < G::MAXT; ++j) stage_task(rx0, j, pre[j], std::true_type{});
    }
    gemm1_issue();
    RBS_T(1);
    __syncthreads();
    RBS_T(2);
    // ---- GEMM 1 -> t1 ring ------------------------------------------------------------------------
    {
      const f32x16 acc = gemm1(j0);
      RBS_T(3);
      t1_write(j0, acc);
    }
    RBS_T(4);
    // ---- the epilogue's operands, then the next chunk's rows (issue order = completion order) -----
    const int pr = POOL ? (n & 3) >> 1 : nr;
    const int pc = POOL ? 2 * (n >> 2) + (n & 1) : nc;
    float4 rsd[POOL ? 1 : 4];
    float4 scpx = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (!POOL) {
      const uint32_t off = w0 + pc < W ? (uint32_t)(o0 + pr) * ROWB + (uint32_t)((w0 + pc) * C + 4 * h) * 4u : 0x80000000u;
#pragma unroll
      for (int jj = 0; jj < 4; ++jj)
        rsd[jj] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rx, off, jj * 32, 0));
    } else {
      scpx = load_src(o0, sc_col, sc_ok(), sc_part);
    }
    if (k + G::PD < G::NCHUNK) {
#pragma unroll
      for (int j = 0; j < G::MAXT; ++j) pre[j] = load_task(rx0 + G::PD * R, j);
    }
    __syncthreads();
    RBS_T(5);
    // ---- GEMM 2 (weights in registers or sw2) ----------------------------------------------------
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    {
      int tr[4], tj[4];
#pragma unroll
      for (int dy = 0; dy < 4; ++dy) {
        tj[dy] = o0 + pr - 1 + dy;
        const uint32_t sl = (uint32_t)(o0 % G::TRING) + (uint32_t)(pr + dy);   // (tj + 1) % TRING
        tr[dy] = (int)min(sl, sl - (uint32_t)G::TRING);
      }
      auto to = [&](int s) { return toff<POOL>(tr[s >> 1], tj[s >> 1], pc, 2 * (s & 1) + h); };
      // one k-step's MFMAs
      auto step2 = [&](f16x8 xh, f16x8 xl, f16x8 gh, f16x8 gl) {
        if constexpr (POOL) {   // y: pixel rows (a register quad = one 2x2 window), channel = lane
          acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(xh, gl, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(xl, gh, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(xh, gh, acc, 0, 0, 0);
        } else {                // y^T: a register quad = 4 channels of this lane's pixel
          acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(gl, xh, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(gh, xl, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(gh, xh, acc, 0, 0, 0);
        }
      };
      if constexpr (G::W2L) {
        // block 1: the t1 and sw2 fragments of step s + 1 in a second register set, each step pinned
        // as "four reads, three MFMAs" (SG::W2L)
        f16x8 fxh[2], fxl[2], fgh[2], fgl[2];
        auto fetch = [&](int s) {
          fxh[s & 1] = *reinterpret_cast<const f16x8*>(st + to(s));
          fxl[s & 1] = *reinterpret_cast<const f16x8*>(st + G::TPLANE + to(s));
          fgh[s & 1] = *reinterpret_cast<const f16x8*>(sw2 + s * 512 + lofs);
          fgl[s & 1] = *reinterpret_cast<const f16x8*>(sw2 + (G::KS2 + s) * 512 + lofs);
        };
        fetch(0);
#pragma unroll
        for (int s = 0; s < G::KS2; ++s) {
          if (s + 1 < G::KS2) fetch(s + 1);
          step2(fxh[s & 1], fxl[s & 1], fgh[s & 1], fgl[s & 1]);
          if (s + 1 < G::KS2) pin_group<1, 4>(); else pin_group<1, 0>();
        }
      } else {
        f16x8 nxh = *reinterpret_cast<const f16x8*>(st + to(0));
        f16x8 nxl = *reinterpret_cast<const f16x8*>(st + G::TPLANE + to(0));
#pragma unroll
        for (int s = 0; s < G::KS2; ++s) {
          const f16x8 xh = nxh, xl = nxl;
          if (s + 1 < G::KS2) {   // the next step's fragments under this step's MFMAs
            nxh = *reinterpret_cast<const f16x8*>(st + to(s + 1));
            nxl = *reinterpret_cast<const f16x8*>(st + G::TPLANE + to(s + 1));
          }
          step2(xh, xl, w2h[s], w2l[s]);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
    RBS_T(6);
    // ---- epilogue ---------------------------------------------------------------------------------
    if constexpr (!POOL) {
      const int ow = w0 + pc, oh = o0 + pr;
      if (ow < W) {
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const int c0 = 8 * jj + 4 * h;
          const float4 b = spar[2 * C / 4 + c0 / 4];
          const float4 r = rsd[jj];
          const float4 v = make_float4(fmaf(acc[4 * jj + 0], a.u2, b.x) + r.x, fmaf(acc[4 * jj + 1], a.u2, b.y) + r.y,
                                       fmaf(acc[4 * jj + 2], a.u2, b.z) + r.z, fmaf(acc[4 * jj + 3], a.u2, b.w) + r.w);
          *reinterpret_cast<float4*>(a.y + (((int64_t)clip * H + oh) * W + ow) * C + c0) = v;
        }
      }
    } else {
      // the shortcut Conv2D(1x1, stride 2) of the raw stem output: A row m = window m >> 2 (x4),
      // k = stem channels 8 h .. 8 h + 7; accumulator register 4 jj + i then holds window 2 jj + h
      f32x16 sacc;
#pragma unroll
      for (int i = 0; i < 16; ++i) sacc[i] = 0.0f;
      if constexpr (SCD) {
        // lanes n, n ^ 1, n ^ 2, n ^ 3 are one window (A row m = window m >> 2): lane n computes stem
        // channels 8 h + 2 j, + 1 (j = n & 3) with the expressions below, splits the pair (split4's
        // operations) and the quad's four lanes exchange their packed pairs by DPP quad broadcasts.  The
        // same operand bits; the wave folds the same set of values into the range maximum
        const float4 px = img_px(scpx);
        const int j = n & 3;
        float o2[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const float4 wv = spar[3 * C / 4 + 8 * h + 2 * j + c];
          float s = px.x * wv.x;
          s = fmaf(px.y, wv.y, s);
          s = fmaf(px.z, wv.z, s);
          o2[c] = sc_ok() ? 16.0f * (s + wv.w) : 0.0f;
        }
        rmax = fmaxf(rmax, fmaxf(fabsf(o2[0]), fabsf(o2[1])));
        typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
        const f16x2 hp = {(_Float16)o2[0], (_Float16)o2[1]};
        const uint32_t hu = __builtin_bit_cast(uint32_t, hp);
        const uint32_t lu = split_lo2(o2[0], o2[1], hu);
        uint4 au, bu;
        au.x = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hu, 0x00, 0xf, 0xf, false);   // quad_perm:[0,0,0,0]
        au.y = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hu, 0x55, 0xf, 0xf, false);   // [1,1,1,1]
        au.z = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hu, 0xaa, 0xf, 0xf, false);   // [2,2,2,2]
        au.w = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hu, 0xff, 0xf, 0xf, false);   // [3,3,3,3]
        bu.x = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)lu, 0x00, 0xf, 0xf, false);
        bu.y = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)lu, 0x55, 0xf, 0xf, false);
        bu.z = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)lu, 0xaa, 0xf, 0xf, false);
        bu.w = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)lu, 0xff, 0xf, 0xf, false);
        const f16x8 ah = __builtin_bit_cast(f16x8, au), al = __builtin_bit_cast(f16x8, bu);
        sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, wsl_, sacc, 0, 0, 0);
        sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, wsh_, sacc, 0, 0, 0);
        sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, wsh_, sacc, 0, 0, 0);
      } else {
        float o8[8];
        const float4 px = img_px(scpx);
#pragma unroll
        for (int c = 0; c < 8; ++c) {   // od_stem_kernel's order
          const float4 wv = spar[3 * C / 4 + 8 * h + c];
          float s = px.x * wv.x;
          s = fmaf(px.y, wv.y, s);
          s = fmaf(px.z, wv.z, s);
          o8[c] = sc_ok() ? 16.0f * (s + wv.w) : 0.0f;
        }
        rmax = fmaxf(rmax, fmaxf(amax4(o8[0], o8[1], o8[2], o8[3]), amax4(o8[4], o8[5], o8[6], o8[7])));
        f16x4 h0, l0, h1, l1;
        split4(o8[0], o8[1], o8[2], o8[3], h0, l0);
        split4(o8[4], o8[5], o8[6], o8[7], h1, l1);
        const f16x8 ah = {h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
        const f16x8 al = {l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]};
        sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, wsl_, sacc, 0, 0, 0);
        sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, wsh_, sacc, 0, 0, 0);
        sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, wsh_, sacc, 0, 0, 0);
      }
      constexpr int HP = H / 2, WP = (W + 1) / 2;
      const int co = n;
      const float b2 = sp[2 * C + co], bs = bsc;
      const int prow = (R / 2) * k + wave;
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int wdw = 2 * jj + h;                  // window: conv columns w0 + 2 wdw, + 1
        // TP, a pair: windows 4-7 (jj >= 2) are part 1's windows 0-3: the next clip, the same columns
        const int op = TP && pair && jj >= 2;
        const int cc = w0 + 2 * (wdw - 4 * op);
        if (cc >= W || (TP && op && !has_b)) continue;
        float m0 = fmaf(acc[4 * jj + 0], a.u2, b2);  // (row 0, col 0)
        float m1 = fmaf(acc[4 * jj + 1], a.u2, b2);  // (row 0, col 1)
        float m2 = fmaf(acc[4 * jj + 2], a.u2, b2);  // (row 1, col 0)
        float m3 = fmaf(acc[4 * jj + 3], a.u2, b2);  // (row 1, col 1)
        if (cc + 1 >= W) {                           // MaxPool 'same' on the odd width: window cut
          m1 = m0;
          m3 = m2;
        }
        const float mx = fmaxf(fmaxf(m0, m1), fmaxf(m2, m3)) + fmaf(sacc[4 * jj], a.us, bs);
        a.y[(((int64_t)(clip + op) * HP + prow) * WP + (w0 >> 1) + wdw - 4 * op) * C + co] = mx;
      }
    }
    RBS_T(7);
    RBS_TFLUSH();
  };
  if constexpr (G::PD == 2) {
#pragma unroll 1
    for (int k = 0; k < G::NCHUNK; k += 2) {
      chunk(k, preA);
      chunk(k + 1, preB);
    }
  } else {
#pragma unroll 1
    for (int k = 0; k < G::NCHUNK; ++k) chunk(k, preA);
  }
  if (!(rmax < SPLIT_MAX) && a.range_flag) *a.range_flag = 1;
}

}  // namespace
