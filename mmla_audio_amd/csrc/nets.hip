// Network glue kernels: OD stem, Lambda mean, MaxPool1D, SI BN+ReLU+AvgPool, BiLSTM, heads.
//
// BiLSTM (Keras 2.6 LSTM, gates i,f,c,o, sigmoid/tanh, h0 = c0 = 0; Bidirectional concat of the
// last states -- overlap_detector_temp.py:297, speaker_identification.py:213) runs as one launch per
// layer: a workgroup owns 32 clips of one direction for all T steps.  Each step is one f32-MFMA
// product [32 x (256 + D)] x [(256 + D) x 1024] with A = [h_{t-1} | x_t] staged in LDS and B (the
// stacked recurrent + input kernels, 1.5 MB, L2-resident) streamed from global; wave w owns hidden
// units [64w, 64w+64) for all four gates, so the gate math and the c-state stay in registers.
#include "common.h"
#include "nets.h"

#include <cstring>

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

template <typename T>
__global__ void od_stem_kernel(const T* __restrict__ x, int64_t n_pix, const float* __restrict__ w, int ldw,
                               const float* __restrict__ b, float* __restrict__ y) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // (pixel, output quad)
  if (i >= n_pix * 4) return;
  const int64_t p = i >> 2;
  const int q = (int)(i & 3);
  const float x0 = (float)x[p * 3 + 0], x1 = (float)x[p * 3 + 1], x2 = (float)x[p * 3 + 2];
  float4 o;
  float* op = &o.x;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int co = q * 4 + j;
    // Keras Conv2D 1x1: sum over ci in order, then bias
    float acc = x0 * w[0 * ldw + co];
    acc = fmaf(x1, w[1 * ldw + co], acc);
    acc = fmaf(x2, w[2 * ldw + co], acc);
    op[j] = acc + b[co];
  }
  reinterpret_cast<float4*>(y)[i] = o;
}

// float4 over channels (c % 4 == 0): the same per-channel summation order, a quarter of the loads
__global__ void mean_h4_kernel(const float4* __restrict__ x, int n, int h, int w, int c4,
                               float4* __restrict__ y) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // over n*w*c4
  const int64_t tot = (int64_t)n * w * c4;
  if (i >= tot) return;
  const int ci = (int)(i % c4);
  const int64_t r = i / c4;
  const int wi = (int)(r % w);
  const int64_t ni = r / w;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int hh = 0; hh < h; ++hh) {
    const float4 v = x[((ni * h + hh) * w + wi) * c4 + ci];
    s.x += v.x;
    s.y += v.y;
    s.z += v.z;
    s.w += v.w;
  }
  const float fh = (float)h;
  y[i] = make_float4(s.x / fh, s.y / fh, s.z / fh, s.w / fh);
}

__global__ void mean_h_kernel(const float* __restrict__ x, int n, int h, int w, int c,
                              float* __restrict__ y) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // over n*w*c
  const int64_t tot = (int64_t)n * w * c;
  if (i >= tot) return;
  const int ci = (int)(i % c);
  const int64_t r = i / c;
  const int wi = (int)(r % w);
  const int64_t ni = r / w;
  float s = 0.0f;
  for (int hh = 0; hh < h; ++hh) s += x[((ni * h + hh) * w + wi) * c + ci];
  y[i] = s / (float)h;
}

__global__ void maxpool_t2_kernel(const float* __restrict__ x, int n, int t, int c,
                                  float* __restrict__ y) {
  const int to = (t + 1) / 2;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t tot = (int64_t)n * to * c;
  if (i >= tot) return;
  const int ci = (int)(i % c);
  const int64_t r = i / c;
  const int ti = (int)(r % to);
  const int64_t ni = r / to;
  float m = x[(ni * t + 2 * ti) * c + ci];
  if (2 * ti + 1 < t) {   // a max that keeps NaN (the exact-f32 path returns what the oracle does)
    const float u = x[(ni * t + 2 * ti + 1) * c + ci];
    m = u > m || u != u ? u : m;
  }
  y[i] = m;
}

__global__ void bn_relu_avgpool4_kernel(const float* __restrict__ x, int n, int t, int c,
                                        const float* __restrict__ sc, const float* __restrict__ sh,
                                        float* __restrict__ y) {
  const int to = t / 4;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t tot = (int64_t)n * to * c;
  if (i >= tot) return;
  const int ci = (int)(i % c);
  const int64_t r = i / c;
  const int ti = (int)(r % to);
  const int64_t ni = r / to;
  float s = 0.0f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {   // ReLU that keeps NaN (np.maximum; fmaxf drops it), the same bits otherwise
    const float v = fmaf(x[(ni * t + 4 * ti + j) * c + ci], sc[ci], sh[ci]);
    s += v > 0.0f ? v : v == v ? 0.0f : v;
  }
  y[i] = s / 4.0f;
}

MMLA_DEV float sigm(float z) { return 1.0f / (1.0f + expf(-z)); }

constexpr int LSTM_U = 256;
constexpr int LSTM_ROWS = 32;

template <int D>
__global__ void __launch_bounds__(256) bilstm_kernel(const float* __restrict__ seq, int n, int T,
                                                     const float* __restrict__ wf,
                                                     const float* __restrict__ wb,
                                                     const float* __restrict__ bf,
                                                     const float* __restrict__ bb,
                                                     float* __restrict__ out) {
  constexpr int K = LSTM_U + D;
  constexpr int LDH = K + 1;
  __shared__ float Ah[LSTM_ROWS][LDH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int dir = blockIdx.y;
  const float* __restrict__ W = dir == 0 ? wf : wb;
  const float* __restrict__ B = dir == 0 ? bf : bb;
  const int64_t c0 = (int64_t)blockIdx.x * LSTM_ROWS;

  for (int e = tid; e < LSTM_ROWS * LSTM_U; e += 256) Ah[e / LSTM_U][e % LSTM_U] = 0.0f;
  float cst[2][16];
#pragma unroll
  for (int ht = 0; ht < 2; ++ht)
#pragma unroll
    for (int r = 0; r < 16; ++r) cst[ht][r] = 0.0f;

  const int col_base = 64 * wave + (lane & 31);   // + 32*ht + 256*g
  const int khalf = lane >> 5;

  for (int s = 0; s < T; ++s) {
    const int t = dir == 0 ? s : T - 1 - s;
    for (int e = tid; e < LSTM_ROWS * D; e += 256) {
      const int r = e / D, d = e - r * D;
      const int64_t clip = c0 + r;
      Ah[r][LSTM_U + d] = clip < n ? seq[(clip * T + t) * D + d] : 0.0f;
    }
    __syncthreads();
    f32x16 acc[4][2];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int ht = 0; ht < 2; ++ht) {
        const float bv = B[g * LSTM_U + col_base + 32 * ht];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[g][ht][r] = bv;
      }
    const float* wp = W + (int64_t)khalf * 1024 + col_base;
#pragma unroll 4
    for (int k2 = 0; k2 < K / 2; ++k2) {
      const float av = Ah[lane & 31][2 * k2 + khalf];
      const float* wr = wp + (int64_t)(2 * k2) * 1024;
      float bv[4][2];
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int ht = 0; ht < 2; ++ht) bv[g][ht] = wr[g * LSTM_U + 32 * ht];
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int ht = 0; ht < 2; ++ht)
          acc[g][ht] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[g][ht], acc[g][ht], 0, 0, 0);
    }
    __syncthreads();   // every wave has read h_{t-1}
#pragma unroll
    for (int ht = 0; ht < 2; ++ht)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        const float ig = sigm(acc[0][ht][r]);
        const float fg = sigm(acc[1][ht][r]);
        const float gg = tanhf(acc[2][ht][r]);
        const float og = sigm(acc[3][ht][r]);
        const float c = fg * cst[ht][r] + ig * gg;
        cst[ht][r] = c;
        Ah[row][col_base + 32 * ht] = og * tanhf(c);
      }
    __syncthreads();
  }
  for (int e = tid; e < LSTM_ROWS * LSTM_U; e += 256) {
    const int r = e / LSTM_U, j = e - r * LSTM_U;
    const int64_t clip = c0 + r;
    if (clip < n) out[clip * 512 + dir * LSTM_U + j] = Ah[r][j];
  }
}


// ---- 3xFP16 BiLSTM ----------------------------------------------------------------------------
// (Round 4: 32 clips per workgroup at two workgroups per CU, or 64 clips at one per CU for batches
// >= 8192; B by buffer loads one gate ahead; gate reciprocals on v_rcp_f32 -- see lstm_rcp,
// bilstm_h3_kernel and bilstm_h3_launch.)
// The same recurrence with the [32 x 384] x [384 x 1024] step product on the f16 MFMA
// (v_mfma_f32_32x32x16_f16) with 3xFP16 products: A = [h_{t-1} | x_t] split into fp16 hi/lo in LDS,
// B = the stacked kernels pre-split on the host and packed in MFMA fragment order (a lane's 8
// k-values are one 16-B load, a wave's 64 loads one contiguous KB).  Unlike conv_h3 the lo halves are not rescaled by 2^11, so
// hi*hi, hi*lo and lo*hi accumulate into ONE f32 accumulator per gate tile (the registers that frees
// hold the next k-step's B fragments: the weight stream from L2 is what the step waits on); to keep
// the lo halves out of the fp16 subnormals both operands are scaled by exact powers of two first
// (weights x 2^8 on the host, [h | x] x 2^6 here) and the accumulator is unscaled once.  Eight waves: wave w
// owns hidden units [32w, 32w + 32) of all four gates, so the gate math stays in registers; the
// c-state stays in registers.
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

// gate nonlinearities on the hardware exp / rcp (a few ulp from expf / tanhf; far inside the 1e-4
// probability tolerance)
// v_rcp_f32 (1 ulp) for the reciprocal (round 4; __frcp_rn, correctly rounded, compiles to
// the ~10-instruction IEEE division sequence -- 80 of them per lane and step sit between a step's
// last MFMA and its barrier
MMLA_DEV float lstm_rcp(float x) {
  return __builtin_amdgcn_rcpf(x);
}
MMLA_DEV float sigm_f(float z) { return lstm_rcp(1.0f + __expf(-z)); }
MMLA_DEV float tanh_f(float x) { return 1.0f - 2.0f * lstm_rcp(1.0f + __expf(2.0f * x)); }

// raw buffer descriptor over [p, p + bytes) for a wave-uniform p (SGPRs), as od_fe.hip wave_rsrc
MMLA_DEV __amdgpu_buffer_rsrc_t lstm_rsrc(const void* p, uint32_t bytes) {
  const uint64_t u = reinterpret_cast<uint64_t>(p);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)u);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(u >> 32));
  return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((uint64_t)hi << 32) | lo), (short)0,
                                           (int)bytes, 0x00020000);
}

// weights: a per-direction power-of-two scale ws (bilstm_h3_split_weights; weights.cpp pick_wscale)
constexpr float LSTM_AS = 64.0f;    // [h | x] scale

MMLA_DEV void split1(float v, _Float16& h, _Float16& l) {   // v * 2^6 = hi + lo
  v *= LSTM_AS;
  h = (_Float16)v;
  l = (_Float16)(v - (float)h);
}

// MT 32-clip row tiles per workgroup (1, or 2 where the batch still fills the chip: half the weight
// stream per clip); PF: prefetch the next k-step's B fragments (MT 1 only: registers)
// (round 4): two workgroups per CU (4 waves per SIMD, <= 128 VGPRs) instead of one with a
// k-step-ahead B ring at 242 VGPRs.  2 (the product): B fragments one GATE ahead (the next
// (k-step, gate)'s 2 x 16 B in flight under this gate's 3 MFMAs); 1: loaded right before their MFMAs,
// the other workgroup's waves hiding the L2 latency.  Bit-identical to 0 (same MFMA order per
// accumulator).  Measured (A/B, one box): SI LSTM stage 9.36 -> 8.71 ms per 3 steps (2) / 9.31 (1);
// OD LSTM 23.8 -> 21.7 ms per 3 steps (2); SI 2.63 -> 2.65 M clips/s
template <int D, int MT>
__global__ void __launch_bounds__(512, MT == 1 ? 4 : 2) bilstm_h3_kernel(const float* __restrict__ seq, int n, int T,
                                                        const uint16_t* __restrict__ wfh,
                                                        const uint16_t* __restrict__ wfl,
                                                        const uint16_t* __restrict__ wbh,
                                                        const uint16_t* __restrict__ wbl,
                                                        const float* __restrict__ bf,
                                                        const float* __restrict__ bb,
                                                        float* __restrict__ out,
                                                        int* __restrict__ range_flag, float ws_f,
                                                        float ws_b) {
  constexpr int K = LSTM_U + D;          // 384
  constexpr int KST = K / 16;            // k-steps
  constexpr int LDA = K + 8;             // fp16 per A row (16-B pad)
  constexpr int NTH = 512;
  constexpr int ROWS = 32 * MT;
  constexpr bool W4 = MT == 1;
  constexpr bool GA = true;            // the gate-ahead buffer-load k-loop (any MT)
  constexpr bool PF = MT == 1 && !W4;
  __shared__ __attribute__((aligned(16))) _Float16 Ahi[ROWS * LDA];
  __shared__ __attribute__((aligned(16))) _Float16 Alo[ROWS * LDA];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int dir = blockIdx.y;
  const uint16_t* __restrict__ Wh = dir == 0 ? wfh : wbh;
  const uint16_t* __restrict__ Wl = dir == 0 ? wfl : wbl;
  const float* __restrict__ B = dir == 0 ? bf : bb;
  const float WS = dir == 0 ? ws_f : ws_b;
  const float LSTM_UNSCALE = 1.0f / (WS * LSTM_AS);   // exact: powers of two
  const int64_t c0 = (int64_t)blockIdx.x * ROWS;

  for (int e = tid; e < ROWS * LSTM_U; e += NTH) {   // h_{-1} = 0
    Ahi[(e / LSTM_U) * LDA + e % LSTM_U] = (_Float16)0.0f;
    Alo[(e / LSTM_U) * LDA + e % LSTM_U] = (_Float16)0.0f;
  }
  const int col = 32 * wave + (lane & 31);   // hidden unit of this lane's accumulator column
  const int koff = 8 * (lane >> 5);
  // B in MFMA fragment order (bilstm_h3_split_weights): the wave's 64 16-B fragments of one gate and
  // k-step are 1 KB contiguous, so a load instruction fills 8 whole 128-B lines.  (Column-major B
  // put the 64 lanes on 32 lines 768 B apart and used 32 B of each: the L1 could not hold the
  // 256 KB of lines a k-step touched, so every 128-B line came from L2 four times.)
  // gate g: + g * GS; k-step ks: + 512 * ks
  const uint16_t* wh0 = Wh + (size_t)wave * KST * 512 + lane * 8;
  const uint16_t* wl0 = Wl + (size_t)wave * KST * 512 + lane * 8;
  constexpr size_t GS = (size_t)LSTM_U * K;
  static_assert(GS == (size_t)(LSTM_U / 32) * KST * 512, "fragment-major gate stride");
  const _Float16* arow_h = Ahi + (lane & 31) * LDA + koff;
  const _Float16* arow_l = Alo + (lane & 31) * LDA + koff;
  float cst[MT][16];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 16; ++r) cst[mt][r] = 0.0f;

  bool rbad = false;   // 3xFP16 range guard: |x * 2^6| must stay below 65504 (|h| < 1 always)
  for (int s = 0; s < T; ++s) {
    const int t = dir == 0 ? s : T - 1 - s;
    // x_t -> A[:, 256:256+D] (float4 loads, split once)
    for (int e = tid; e < ROWS * D / 4; e += NTH) {
      const int r = e / (D / 4), d4 = e - r * (D / 4);
      const int64_t clip = c0 + r;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (clip < n) v = *reinterpret_cast<const float4*>(seq + (clip * T + t) * D + 4 * d4);
      rbad |= !(fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))) <
                65504.0f / LSTM_AS);
      _Float16 h0, h1, h2, h3, l0, l1, l2, l3;
      split1(v.x, h0, l0);
      split1(v.y, h1, l1);
      split1(v.z, h2, l2);
      split1(v.w, h3, l3);
      const f16x4 hv = {h0, h1, h2, h3}, lv = {l0, l1, l2, l3};
      *reinterpret_cast<f16x4*>(Ahi + r * LDA + LSTM_U + 4 * d4) = hv;
      *reinterpret_cast<f16x4*>(Alo + r * LDA + LSTM_U + 4 * d4) = lv;
    }
    f16x8 bh[4], bl[4];
    if constexpr (PF) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {   // k-step 0's B: issued before the barrier
        bh[g] = *reinterpret_cast<const f16x8*>(wh0 + g * GS);
        bl[g] = *reinterpret_cast<const f16x8*>(wl0 + g * GS);
      }
    }
    __syncthreads();
    f32x16 acc[MT][4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float bv = B[g * LSTM_U + col] * (WS * LSTM_AS);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][g][r] = bv;
    }
    if constexpr (GA) {
      // one gate ahead: the next (k-step, gate)'s B fragments in flight under this gate's MFMAs.
      // Addressed as a uniform (SGPR) base + this lane's 32-bit byte offset, so every load is one
      // global_load with saddr and no per-load 64-bit address arithmetic
      const uint32_t lob = (uint32_t)(wave * KST * 512 + lane * 8) * 2u;
      const __amdgpu_buffer_rsrc_t rh = lstm_rsrc(Wh, (uint32_t)(4 * GS * 2));
      const __amdgpu_buffer_rsrc_t rl = lstm_rsrc(Wl, (uint32_t)(4 * GS * 2));
      auto frag = [&](__amdgpu_buffer_rsrc_t r, size_t uoff) {
        return __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(r, lob, (int)(uoff * 2), 0));
      };
      f16x8 gh = frag(rh, 0);
      f16x8 gl = frag(rl, 0);
#pragma unroll 1
      for (int ks = 0; ks < KST; ++ks) {
        f16x8 ah[MT], al[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          ah[mt] = *reinterpret_cast<const f16x8*>(arow_h + 32 * mt * LDA + 16 * ks);
          al[mt] = *reinterpret_cast<const f16x8*>(arow_l + 32 * mt * LDA + 16 * ks);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int gn = g < 3 ? g + 1 : 0, kn = g < 3 ? ks : (ks + 1 < KST ? ks + 1 : ks);
          const f16x8 nh = frag(rh, gn * GS + 512 * (size_t)kn);
          const f16x8 nl = frag(rl, gn * GS + 512 * (size_t)kn);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            acc[mt][g] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[mt], gh, acc[mt][g], 0, 0, 0);
            acc[mt][g] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[mt], gl, acc[mt][g], 0, 0, 0);
            acc[mt][g] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[mt], gh, acc[mt][g], 0, 0, 0);
          }
          gh = nh;
          gl = nl;
        }
      }
    } else if constexpr (W4) {
#pragma unroll 1
      for (int ks = 0; ks < KST; ++ks) {
        const f16x8 ah = *reinterpret_cast<const f16x8*>(arow_h + 16 * ks);
        const f16x8 al = *reinterpret_cast<const f16x8*>(arow_l + 16 * ks);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f16x8 gh = *reinterpret_cast<const f16x8*>(wh0 + g * GS + 512 * ks);
          const f16x8 gl = *reinterpret_cast<const f16x8*>(wl0 + g * GS + 512 * ks);
          acc[0][g] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, gh, acc[0][g], 0, 0, 0);
          acc[0][g] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, gl, acc[0][g], 0, 0, 0);
          acc[0][g] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, gh, acc[0][g], 0, 0, 0);
        }
      }
    } else
#pragma unroll 2
    for (int ks = 0; ks < KST; ++ks) {
      f16x8 nh[4], nl[4];
      if constexpr (PF) {   // next k-step's B under this one's MFMAs
        const int kn = ks + 1 < KST ? ks + 1 : ks;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          nh[g] = *reinterpret_cast<const f16x8*>(wh0 + g * GS + 512 * kn);
          nl[g] = *reinterpret_cast<const f16x8*>(wl0 + g * GS + 512 * kn);
        }
      } else {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          bh[g] = *reinterpret_cast<const f16x8*>(wh0 + g * GS + 512 * ks);
          bl[g] = *reinterpret_cast<const f16x8*>(wl0 + g * GS + 512 * ks);
        }
      }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const f16x8 ah = *reinterpret_cast<const f16x8*>(arow_h + 32 * mt * LDA + 16 * ks);
        const f16x8 al = *reinterpret_cast<const f16x8*>(arow_l + 32 * mt * LDA + 16 * ks);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          acc[mt][g] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh[g], acc[mt][g], 0, 0, 0);
          acc[mt][g] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl[g], acc[mt][g], 0, 0, 0);
          acc[mt][g] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh[g], acc[mt][g], 0, 0, 0);
        }
      }
      if constexpr (PF) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          bh[g] = nh[g];
          bl[g] = nl[g];
        }
      }
    }
    __syncthreads();   // every wave has read h_{t-1}
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        const float ig = sigm_f(acc[mt][0][r] * LSTM_UNSCALE);
        const float fg = sigm_f(acc[mt][1][r] * LSTM_UNSCALE);
        const float gg = tanh_f(acc[mt][2][r] * LSTM_UNSCALE);
        const float og = sigm_f(acc[mt][3][r] * LSTM_UNSCALE);
        const float c = fg * cst[mt][r] + ig * gg;
        cst[mt][r] = c;
        const float h = og * tanh_f(c);
        if (s == T - 1) {   // the last state (Keras return_sequences=False), float32
          int rr = row;
          asm volatile("" : "+v"(rr));   // the address formed here: hoisted, 16 of them were spilled
          const int64_t clip = c0 + rr;
          if (clip < n) out[clip * 512 + dir * LSTM_U + col] = h;
        }
        _Float16 hh, hl;
        split1(h, hh, hl);
        Ahi[row * LDA + col] = hh;
        Alo[row * LDA + col] = hl;
      }
  }
  if (rbad && range_flag) *range_flag = 1;
}

// ---- small-batch BiLSTM: a direction's hidden units over eight CUs ------------------------------
// bilstm_h3_kernel<128,1> with n <= 32 runs each direction as ONE workgroup: every step streams the
// direction's 1.5 MB of B fragments through one CU's L2 port (the batch-1 real-time call's largest
// kernel).  Here the direction runs on eight workgroups, workgroup w owning bilstm_h3_kernel wave w's
// 32 hidden units, and inside it wave g owns gate g: the wave's B fragments for one gate (24 k-steps
// x hi / lo, 192 VGPRs) are loaded ONCE and stay in registers for all T steps, so a step streams no
// weights at all.  Per step: the 72 MFMAs of the wave's gate (the same accumulator sequence as
// bilstm_h3_kernel's gate-ahead loop), the four gates' pre-activations exchanged through LDS, the
// gate math (each thread owns 4 of the 32 x 32 units and their c-state), and the 32 x 256 h_{t-1}
// planes (fp16 hi / lo, 32 KB) exchanged through HBM: each workgroup publishes its 32 columns into
// xbuf[dir][s & 1] and bumps sync[dir] (release fence at agent scope: the eight workgroups sit on
// different XCDs, whose L2s are not coherent with each other), then waits for the counter to reach
// 8 (s + 1) (acquire) before reading all 256 columns.  Outputs are bit-identical to
// bilstm_h3_kernel (tests/test_gpu_batching.py).  Batches of up to 8 x 32 clips: one 32-row tile per
// grid z, with its own counters sync[2 tile + dir] (zero at launch: bilstm_h3_split_launch clears them
// on the stream) and exchange buffers.  Waits are bounded at `spin` polls (LSTM_SPLIT_SPIN unless a
// debug limit is given): thread 0 polls and the decision is broadcast through LDS, so a workgroup gives
// up as a whole -- it sets sync[63] and *timeout_flag, writes NaN for its units and exits, and the grid
// always drains.  The host reads the flag (pipeline.cpp guarded(): a host call re-runs the micro-batch on
// bilstm_h3_kernel, bit-identical; a device-pointer call reports MMLA_E_HIP at mmla_synchronize).
// Publication: each wave's h stores, its agent-scope release fence, the workgroup barrier, then
// thread 0's counter increment as an agent-scope RELEASE read-modify-write; the reader's thread 0
// observes the count, the barrier hands that on, and every wave fences acquire at agent scope before
// it reads the exchange buffer.
constexpr int LSTM_SPLIT_ROWS = 32;
constexpr int LSTM_SPLIT_SPIN = 1 << 22;
// up to 8 row tiles of 32 clips (grid z): at most 128 workgroups, so all of them are resident at once
constexpr int LSTM_SPLIT_TILES = 8;

template <int D>
__global__ void __launch_bounds__(256, 1) bilstm_h3_split_kernel(const float* __restrict__ seq, int n, int T,
                                                                 const uint16_t* __restrict__ wfh,
                                                                 const uint16_t* __restrict__ wfl,
                                                                 const uint16_t* __restrict__ wbh,
                                                                 const uint16_t* __restrict__ wbl,
                                                                 const float* __restrict__ bf,
                                                                 const float* __restrict__ bb,
                                                                 float* __restrict__ out,
                                                                 int* __restrict__ range_flag,
                                                                 float ws_f, float ws_b, int* sync,
                                                                 _Float16* xbuf, int* timeout_flag,
                                                                 int spin) {
  constexpr int K = LSTM_U + D;
  constexpr int KST = K / 16;
  constexpr int LDA = K + 8;
  constexpr int ROWS = LSTM_SPLIT_ROWS;
  constexpr int PLANE = ROWS * LSTM_U;   // fp16 per h plane
  constexpr int NTH = 256;
  __shared__ __attribute__((aligned(16))) _Float16 Ahi[ROWS * LDA];
  __shared__ __attribute__((aligned(16))) _Float16 Alo[ROWS * LDA];
  __shared__ float G[4][16][64];   // the four gates' accumulators, [gate][register][lane]
  __shared__ int arrived;          // thread 0's wait result, the same for the whole workgroup
  const int tid = threadIdx.x, lane = tid & 63, gate = tid >> 6;
  const int grp = blockIdx.x;   // hidden units [32 grp, 32 grp + 32) (bilstm_h3_kernel's wave grp)
  const int dir = blockIdx.y;
  const uint16_t* __restrict__ Wh = dir == 0 ? wfh : wbh;
  const uint16_t* __restrict__ Wl = dir == 0 ? wfl : wbl;
  const float* __restrict__ B = dir == 0 ? bf : bb;
  const float WS = dir == 0 ? ws_f : ws_b;
  const float LSTM_UNSCALE = 1.0f / (WS * LSTM_AS);
  const int tile = blockIdx.z;   // clips [32 tile, 32 tile + 32)
  const int nr = n - 32 * tile;   // rows of this tile that are clips
  int* cnt = sync + 2 * tile + dir;
  _Float16* xh = xbuf + (size_t)(2 * tile + dir) * 2 * 2 * PLANE;   // [parity][hi, lo][row][256]
  seq += (int64_t)32 * tile * T * D;
  out += (int64_t)32 * tile * 512;
  const int col = 32 * grp + (lane & 31);
  const int koff = 8 * (lane >> 5);
  constexpr size_t GS = (size_t)LSTM_U * K;

  // the wave's gate of the group's B fragments, resident for the launch
  const uint32_t lob = (uint32_t)(grp * KST * 512 + lane * 8) * 2u;
  const __amdgpu_buffer_rsrc_t rh = lstm_rsrc(Wh, (uint32_t)(4 * GS * 2));
  const __amdgpu_buffer_rsrc_t rl = lstm_rsrc(Wl, (uint32_t)(4 * GS * 2));
  f16x8 bh[KST], bl[KST];
#pragma unroll
  for (int ks = 0; ks < KST; ++ks) {
    const int uo = (int)((gate * GS + 512 * (size_t)ks) * 2);
    bh[ks] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(rh, lob, uo, 0));
    bl[ks] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(rl, lob, uo, 0));
  }
  const float bias = B[gate * LSTM_U + col] * (WS * LSTM_AS);

  for (int e = tid; e < ROWS * LSTM_U / 8; e += NTH) {   // h_{-1} = 0
    const int r = e / (LSTM_U / 8), q = e - r * (LSTM_U / 8);
    *reinterpret_cast<f16x8*>(Ahi + r * LDA + 8 * q) = f16x8{};
    *reinterpret_cast<f16x8*>(Alo + r * LDA + 8 * q) = f16x8{};
  }
  bool rbad = false;
  auto stage_x = [&](int t) {   // x_t -> A[:, 256:256+D], as bilstm_h3_kernel
    for (int e = tid; e < ROWS * D / 4; e += NTH) {
      const int r = e / (D / 4), d4 = e - r * (D / 4);
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < nr) v = *reinterpret_cast<const float4*>(seq + ((int64_t)r * T + t) * D + 4 * d4);
      rbad |= !(fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))) <
                65504.0f / LSTM_AS);
      _Float16 h0, h1, h2, h3, l0, l1, l2, l3;
      split1(v.x, h0, l0);
      split1(v.y, h1, l1);
      split1(v.z, h2, l2);
      split1(v.w, h3, l3);
      const f16x4 hv = {h0, h1, h2, h3}, lv = {l0, l1, l2, l3};
      *reinterpret_cast<f16x4*>(Ahi + r * LDA + LSTM_U + 4 * d4) = hv;
      *reinterpret_cast<f16x4*>(Alo + r * LDA + LSTM_U + 4 * d4) = lv;
    }
  };
  const _Float16* arow_h = Ahi + (lane & 31) * LDA + koff;
  const _Float16* arow_l = Alo + (lane & 31) * LDA + koff;
  float cst[4] = {0.0f, 0.0f, 0.0f, 0.0f};   // units (register 4 gate + j, lane)

  stage_x(dir == 0 ? 0 : T - 1);
  bool dead = false;
  for (int s = 0; s < T; ++s) {
    if (s > 0) {   // every workgroup's h_{t-1} published
      if (tid == 0) {
        int it = 0;
        while (__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 8 * s && it < spin) {
          __builtin_amdgcn_s_sleep(1);
          ++it;
        }
        // spin < 0 (test hook): give up at the first wait without polling, deterministically
        arrived = spin >= 0 &&
                  (it < spin || __hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= 8 * s);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // pairs with the publishers' release RMW
      }
      __syncthreads();
      if (!arrived) {   // workgroup-uniform: no wave is left at a barrier the others skip
        dead = true;
        break;
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      const _Float16* src = xh + (size_t)((s - 1) & 1) * 2 * PLANE;
      for (int e = tid; e < 2 * PLANE / 8; e += NTH) {   // planes hi, lo: 16-B chunks, row-major
        const int hl = e / (PLANE / 8), rem = e - hl * (PLANE / 8);
        const int r = rem / (LSTM_U / 8), q = rem - r * (LSTM_U / 8);
        const f16x8 v = *reinterpret_cast<const f16x8*>(src + (size_t)e * 8);
        *reinterpret_cast<f16x8*>((hl ? Alo : Ahi) + r * LDA + 8 * q) = v;
      }
    }
    __syncthreads();
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = bias;
#pragma unroll
    for (int ks = 0; ks < KST; ++ks) {
      const f16x8 ah = *reinterpret_cast<const f16x8*>(arow_h + 16 * ks);
      const f16x8 al = *reinterpret_cast<const f16x8*>(arow_l + 16 * ks);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh[ks], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl[ks], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh[ks], acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) G[gate][r][lane] = acc[r];
    __syncthreads();   // the gates are in LDS; every wave has read h_{t-1} and x_t
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = 4 * gate + j;
      const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      const float ig = sigm_f(G[0][r][lane] * LSTM_UNSCALE);
      const float fg = sigm_f(G[1][r][lane] * LSTM_UNSCALE);
      const float gg = tanh_f(G[2][r][lane] * LSTM_UNSCALE);
      const float og = sigm_f(G[3][r][lane] * LSTM_UNSCALE);
      const float c = fg * cst[j] + ig * gg;
      cst[j] = c;
      const float h = og * tanh_f(c);
      if (s == T - 1 && row < nr) out[(int64_t)row * 512 + dir * LSTM_U + col] = h;
      _Float16 hh, hl;
      split1(h, hh, hl);
      Ahi[row * LDA + col] = hh;
      Alo[row * LDA + col] = hl;
    }
    if (s + 1 < T) {
      __syncthreads();
      {   // this group's 32 columns of both planes -> xbuf[dir][s & 1]: one 16-B chunk per thread
        _Float16* dst = xh + (size_t)(s & 1) * 2 * PLANE;
        const int hl = tid / (ROWS * 4), rem = tid - hl * (ROWS * 4);
        const int r = rem >> 2, q = rem & 3;
        const f16x8 v = *reinterpret_cast<const f16x8*>((hl ? Alo : Ahi) + r * LDA + 32 * grp + 8 * q);
        *reinterpret_cast<f16x8*>(dst + (size_t)hl * PLANE + r * LSTM_U + 32 * grp + 8 * q) = v;
      }
      static_assert(2 * ROWS * 4 == NTH, "one publish chunk per thread");
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");   // each wave: its stores, then L2 written back
      __syncthreads();
      if (tid == 0) __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      stage_x(dir == 0 ? s + 1 : T - 2 - s);   // under the other workgroups' arrival
    }
  }
  if (dead) {
    if (tid == 0) {
      __hip_atomic_store(sync + 63, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (timeout_flag) *timeout_flag = 1;
    }
    for (int j = 0; j < 4; ++j) {
      const int r = 4 * gate + j, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if (row < nr) out[(int64_t)row * 512 + dir * LSTM_U + col] = __builtin_nanf("");
    }
  }
  if (rbad && range_flag) *range_flag = 1;
}

__global__ void od_head_kernel(const float* __restrict__ h, int n, const float* __restrict__ w,
                               const float* __restrict__ b, float* __restrict__ probs,
                               int32_t* __restrict__ argmax, const int32_t* __restrict__ lens,
                               int clip_len, uint8_t* __restrict__ silent,
                               const float* __restrict__ ssim, float ssim_threshold) {
  // one wave per clip
  const int lane = threadIdx.x & 63;
  const int64_t clip = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (clip >= n) return;
  const float alpha = 0.30000001192092896f;   // LeakyReLU(alpha=0.3) stored float32
  float z0 = 0.0f, z1 = 0.0f;
  for (int i = lane; i < 512; i += 64) {
    float v = h[clip * 512 + i];
    v = v > 0.0f ? v : v * alpha;
    z0 = fmaf(v, w[i * 2 + 0], z0);
    z1 = fmaf(v, w[i * 2 + 1], z1);
  }
  z0 = wave_sum(z0) + b[0];
  z1 = wave_sum(z1) + b[1];
  if (lane == 0) {
    const float m = fmaxf(z0, z1);
    const float e0 = expf(z0 - m), e1 = expf(z1 - m);
    const float s = e0 + e1;
    if (probs) {
      probs[clip * 2 + 0] = e0 / s;
      probs[clip * 2 + 1] = e1 / s;
    }
    // record_on_pc.py:141-154: fewer than 4000 samples (after VAD) -> 'silent', no class
    // record_on_pi.py:103-124: ... or the clip's image barely changed by denoising it (its SSIM
    // against the denoised clip's image below the threshold)
    const bool sil = clip_len >= 0 && ((lens ? lens[clip] : clip_len) < 4000 ||
                                       (ssim && ssim[clip] < ssim_threshold));
    if (silent) silent[clip] = sil ? 1 : 0;
    if (argmax) argmax[clip] = sil ? -1 : (e1 / s > e0 / s ? 1 : 0);
  }
}

// the K-way head (2 < K <= OD_HEAD_MAX_K): od_head_kernel's walk with K accumulators in registers -- every
// loop over the classes is unrolled to OD_HEAD_MAX_K and cut at K, which is the same for the whole launch
__global__ void od_head_k_kernel(const float* __restrict__ h, int n, int K, const float* __restrict__ w,
                                 const float* __restrict__ b, float* __restrict__ probs,
                                 int32_t* __restrict__ argmax, const int32_t* __restrict__ lens,
                                 int clip_len, uint8_t* __restrict__ silent,
                                 const float* __restrict__ ssim, float ssim_threshold) {
  const int lane = threadIdx.x & 63;
  const int64_t clip = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (clip >= n) return;
  const float alpha = 0.30000001192092896f;   // LeakyReLU(alpha=0.3) stored float32
  float z[OD_HEAD_MAX_K];
#pragma unroll
  for (int k = 0; k < OD_HEAD_MAX_K; ++k) z[k] = 0.0f;
  for (int i = lane; i < 512; i += 64) {
    float v = h[clip * 512 + i];
    v = v > 0.0f ? v : v * alpha;
#pragma unroll
    for (int k = 0; k < OD_HEAD_MAX_K; ++k)
      if (k < K) z[k] = fmaf(v, w[i * K + k], z[k]);
  }
#pragma unroll
  for (int k = 0; k < OD_HEAD_MAX_K; ++k)
    if (k < K) z[k] = wave_sum(z[k]) + b[k];
  if (lane == 0) {
    float m = z[0];
#pragma unroll
    for (int k = 1; k < OD_HEAD_MAX_K; ++k)
      if (k < K) m = fmaxf(m, z[k]);
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < OD_HEAD_MAX_K; ++k)
      if (k < K) {
        z[k] = expf(z[k] - m);
        s += z[k];
      }
    // the first index whose probability, as written, is above every earlier one
    int best = 0;
    float pbest = z[0] / s;
#pragma unroll
    for (int k = 0; k < OD_HEAD_MAX_K; ++k)
      if (k < K) {
        const float p = z[k] / s;
        if (probs) probs[clip * K + k] = p;
        if (p > pbest) {
          pbest = p;
          best = k;
        }
      }
    // the 'silent' rule of od_head_kernel
    const bool sil = clip_len >= 0 && ((lens ? lens[clip] : clip_len) < 4000 ||
                                       (ssim && ssim[clip] < ssim_threshold));
    if (silent) silent[clip] = sil ? 1 : 0;
    if (argmax) argmax[clip] = sil ? -1 : best;
  }
}

__global__ void si_head_kernel(const float* __restrict__ logits, int n, int k, int ld, int head,
                               float* __restrict__ probs, int32_t* __restrict__ argmax,
                               const uint8_t* __restrict__ silent) {
  const int lane = threadIdx.x & 63;
  const int64_t clip = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (clip >= n) return;
  const float* z = logits + clip * ld;
  // the logits are read once (K <= 64 KREG: registers; larger K: re-read), each exponential taken once
  constexpr int KREG = 16;
  float zr[KREG];
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < KREG; ++j) {
    const int i = lane + 64 * j;
    zr[j] = i < k ? z[i] : -INFINITY;
    m = fmaxf(m, zr[j]);
  }
  for (int i = lane + 64 * KREG; i < k; i += 64) m = fmaxf(m, z[i]);
  m = wave_max(m);
  float s = 0.0f;
  if (head == 0) {
#pragma unroll
    for (int j = 0; j < KREG; ++j) {
      if (lane + 64 * j < k) {
        zr[j] = expf(zr[j] - m);
        s += zr[j];
      }
    }
    for (int i = lane + 64 * KREG; i < k; i += 64) s += expf(z[i] - m);
    s = wave_sum(s);
  }
  float best = -INFINITY;
  int bi = 0x7fffffff;
  auto take = [&](int i, float p) {
    if (probs) probs[clip * k + i] = p;
    if (p > best) {   // first occurrence within the lane's strided subset
      best = p;
      bi = i;
    }
  };
#pragma unroll
  for (int j = 0; j < KREG; ++j) {
    const int i = lane + 64 * j;
    if (i < k) take(i, head == 0 ? zr[j] / s : 1.0f / (1.0f + expf(-zr[j])));
  }
  for (int i = lane + 64 * KREG; i < k; i += 64)
    take(i, head == 0 ? expf(z[i] - m) / s : 1.0f / (1.0f + expf(-z[i])));
  // wave argmax, ties -> lowest index (numpy argmax)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ob > best || (ob == best && oi < bi)) {
      best = ob;
      bi = oi;
    }
  }
  if (lane == 0 && argmax) argmax[clip] = (silent && silent[clip]) ? -1 : bi;
}

inline unsigned blocks_for(int64_t work, int bs) { return (unsigned)((work + bs - 1) / bs); }

}  // namespace

hipError_t od_stem_launch(const uint8_t* img_u8, const float* img_f32, int64_t n_pix, int ldw,
                          const float* w, const float* b, float* y, hipStream_t s) {
  if (n_pix <= 0) return hipSuccess;
  if (img_u8)
    hipLaunchKernelGGL(od_stem_kernel<uint8_t>, dim3(blocks_for(n_pix * 4, 256)), dim3(256), 0, s,
                       img_u8, n_pix, w, ldw, b, y);
  else
    hipLaunchKernelGGL(od_stem_kernel<float>, dim3(blocks_for(n_pix * 4, 256)), dim3(256), 0, s,
                       img_f32, n_pix, w, ldw, b, y);
  return hipGetLastError();
}

hipError_t mean_h_launch(const float* x, int n, int h, int w, int c, float* y, hipStream_t s) {
  const int64_t tot = (int64_t)n * w * c;
  if (tot <= 0) return hipSuccess;
  if (c % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0) {
    hipLaunchKernelGGL(mean_h4_kernel, dim3(blocks_for(tot / 4, 256)), dim3(256), 0, s,
                       reinterpret_cast<const float4*>(x), n, h, w, c / 4, reinterpret_cast<float4*>(y));
    return hipGetLastError();
  }
  hipLaunchKernelGGL(mean_h_kernel, dim3(blocks_for(tot, 256)), dim3(256), 0, s, x, n, h, w, c, y);
  return hipGetLastError();
}

hipError_t maxpool_t2_launch(const float* x, int n, int t, int c, float* y, hipStream_t s) {
  const int64_t tot = (int64_t)n * ((t + 1) / 2) * c;
  if (tot <= 0) return hipSuccess;
  hipLaunchKernelGGL(maxpool_t2_kernel, dim3(blocks_for(tot, 256)), dim3(256), 0, s, x, n, t, c, y);
  return hipGetLastError();
}

hipError_t bn_relu_avgpool4_launch(const float* x, int n, int t, int c, const float* scale,
                                   const float* shift, float* y, hipStream_t s) {
  const int64_t tot = (int64_t)n * (t / 4) * c;
  if (tot <= 0) return hipSuccess;
  hipLaunchKernelGGL(bn_relu_avgpool4_kernel, dim3(blocks_for(tot, 256)), dim3(256), 0, s, x, n, t,
                     c, scale, shift, y);
  return hipGetLastError();
}

hipError_t bilstm_launch(const float* seq, int n, int T, int D, const float* wf, const float* wb,
                         const float* bf, const float* bb, float* out, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (D != 128) return hipErrorInvalidValue;
  dim3 grid(blocks_for(n, LSTM_ROWS), 2);
  hipLaunchKernelGGL(bilstm_kernel<128>, grid, dim3(256), 0, s, seq, n, T, wf, wb, bf, bb, out);
  return hipGetLastError();
}

hipError_t bilstm_h3_launch(const float* seq, int n, int T, int D, const uint16_t* wfh,
                            const uint16_t* wfl, const uint16_t* wbh, const uint16_t* wbl,
                            const float* bf, const float* bb, float* out, int* range_flag,
                            float ws_fwd, float ws_bwd, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (D != 128) return hipErrorInvalidValue;
  // 64 clips per workgroup (one workgroup of 8 waves per CU, 256 VGPRs) wherever the batch still
  // gives every CU a workgroup per direction: half the per-step weight stream per clip, bit-identical
  // (the same MFMA sequence per clip).  Measured (A/B, one box): SI LSTM 7.56 -> 6.89 ms per 3 steps,
  // OD 18.4 -> 17.0.  Small batches (the batch-1 real-time call) keep 32-clip workgroups, two per CU.
  if (n >= 8192) {
    hipLaunchKernelGGL((bilstm_h3_kernel<128, 2>), dim3(blocks_for(n, 2 * LSTM_ROWS), 2), dim3(512), 0, s,
                       seq, n, T, wfh, wfl, wbh, wbl, bf, bb, out, range_flag, ws_fwd, ws_bwd);
    return hipGetLastError();
  }
  hipLaunchKernelGGL((bilstm_h3_kernel<128, 1>), dim3(blocks_for(n, LSTM_ROWS), 2), dim3(512), 0, s,
                     seq, n, T, wfh, wfl, wbh, wbl, bf, bb, out, range_flag, ws_fwd, ws_bwd);
  return hipGetLastError();
}

size_t bilstm_h3_split_ws_bytes() {
  return 256 + (size_t)LSTM_SPLIT_TILES * 2 * 2 * 2 * LSTM_SPLIT_ROWS * LSTM_U * 2;
}
int bilstm_h3_split_max_clips() { return LSTM_SPLIT_TILES * LSTM_SPLIT_ROWS; }

hipError_t bilstm_h3_split_launch(const float* seq, int n, int T, int D, const uint16_t* wfh,
                                  const uint16_t* wfl, const uint16_t* wbh, const uint16_t* wbl,
                                  const float* bf, const float* bb, float* out, int* range_flag,
                                  float ws_fwd, float ws_bwd, void* ws, int* timeout_flag,
                                  int spin, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (D != 128 || n > LSTM_SPLIT_TILES * LSTM_SPLIT_ROWS || T < 1) return hipErrorInvalidValue;
  if (spin == 0) spin = LSTM_SPLIT_SPIN;   // < 0: the deterministic give-up test hook
  const int tiles = (n + LSTM_SPLIT_ROWS - 1) / LSTM_SPLIT_ROWS;
  int* sync = static_cast<int*>(ws);
  _Float16* xbuf = reinterpret_cast<_Float16*>(static_cast<char*>(ws) + 256);
  const hipError_t e = hipMemsetAsync(sync, 0, 64 * sizeof(int), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((bilstm_h3_split_kernel<128>), dim3(8, 2, tiles), dim3(256), 0, s, seq, n, T, wfh, wfl,
                     wbh, wbl, bf, bb, out, range_flag, ws_fwd, ws_bwd, sync, xbuf, timeout_flag, spin);
  return hipGetLastError();
}

void bilstm_h3_split_weights(const float* wcat, int D, uint16_t* hi, uint16_t* lo, float ws) {
  // MFMA fragment order: gate column j = 256 g + 32 w + n (w: the wave owning it), k = 16 ks + 8 hf +
  // e -> ((g * 8 + w) * KST + ks) * 512 + (n + 32 hf) * 8 + e, i.e. the B fragment of lane
  // n + 32 hf for that gate / wave / k-step (bilstm_h3_kernel)
  const int K = 256 + D, KST = K / 16;
  for (int j = 0; j < 1024; ++j)
    for (int k = 0; k < K; ++k) {
      const float v = wcat[(size_t)k * 1024 + j] * ws;   // exact power-of-two scale
      const _Float16 h = (_Float16)v;
      const _Float16 l = (_Float16)(v - (float)h);   // not rescaled (bilstm_h3_kernel)
      const int g = j / 256, w = (j % 256) / 32, n = j % 32;
      const int ks = k / 16, hf = (k % 16) / 8, e = k % 8;
      const size_t at = ((size_t)(g * 8 + w) * KST + ks) * 512 + (size_t)(n + 32 * hf) * 8 + e;
      memcpy(&hi[at], &h, 2);
      memcpy(&lo[at], &l, 2);
    }
}

hipError_t od_head_launch(const float* h, int n, int k, const float* w, const float* b, float* probs,
                          int32_t* argmax, const int32_t* lens, int clip_len, uint8_t* silent,
                          const float* ssim, float ssim_threshold, hipStream_t s) {
  if (k < 2 || k > OD_HEAD_MAX_K) return hipErrorInvalidValue;
  if (n <= 0) return hipSuccess;
  if (k == 2)
    hipLaunchKernelGGL(od_head_kernel, dim3(blocks_for((int64_t)n * 64, 256)), dim3(256), 0, s, h, n,
                       w, b, probs, argmax, lens, clip_len, silent, ssim, ssim_threshold);
  else
    hipLaunchKernelGGL(od_head_k_kernel, dim3(blocks_for((int64_t)n * 64, 256)), dim3(256), 0, s, h, n, k,
                       w, b, probs, argmax, lens, clip_len, silent, ssim, ssim_threshold);
  return hipGetLastError();
}

hipError_t si_head_launch(const float* logits, int n, int k, int ld, int head, float* probs,
                          int32_t* argmax, const uint8_t* silent, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(si_head_kernel, dim3(blocks_for((int64_t)n * 64, 256)), dim3(256), 0, s,
                     logits, n, k, ld, head, probs, argmax, silent);
  return hipGetLastError();
}
