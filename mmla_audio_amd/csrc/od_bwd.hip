// Adapting OD-NET to a room: the float32 training kernels of OverlapDetector.continue_train_model
// (overlap_detector.py:480-509) that the inference path does not have.  The forward convolutions and the
// stride-1 data gradients are conv.hip's conv_launch (a data gradient is a convolution of dy with the
// flipped, transposed kernel that odb_conv_transpose writes); the BiLSTM is si_bwd.hip's.  Here:
//
//   batch statistics   BatchNorm in training mode: per channel over B * H * W, two passes (mean, then the
//                      centred squares), the moving statistics advanced on the way
//   weight gradient    dW[tap][ci][co] = sum_p a[p (+) tap][ci] dy[p][co] on v_mfma_f32_32x32x2_f32: a GEMM
//                      whose reduction runs over the pixels.  Channels-last rows give both operands straight
//                      from global memory in the MFMA's layout (lanes 0..31 = 32 consecutive channels of one
//                      pixel, lanes 32..63 the next pixel's), so nothing is staged in LDS; a = elu(bn(x)) is
//                      recomputed from x on the way, as conv.hip's prologue computes it
//   BN + ELU backward, max-pool backward by the stored winner, the stride-2 shortcut's data gradient, the
//   mean over H, the head (dropout mask, LeakyReLU, Dense(2), softmax, weighted loss), Adadelta
//   training from scratch (mmla_od_train): the keep-bits of a batch from Philox4x32-10 (philox.h, site 2) as
//   mask bytes, and tf.keras.metrics.AUC(): integer TP / FP counts per threshold, one thread per threshold,
//   then the trapezoid sum in double
//
// Determinism: no floating-point atomics.  Every sum over pixels is split into slabs whose count depends
// on the shape alone; a workgroup reduces its slab in a fixed order (serial per thread, then an LDS tree,
// or the MFMA's own order) and a second launch adds the slabs in slab order, in float64.
//
// Bounds: every index is derived from the launch's own sizes; perm entries are clamped, a label selects one
// of two lanes by its lowest bit, mask bytes are read as zero / non-zero.
#include "od_bwd.h"

#include "philox.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr float BN_EPS = 1e-3f;
constexpr float LEAKY = 0.3f;                  // float32(0.3)
constexpr float KEEP_SCALE = 1.0f / 0.75f;     // float32(1 / (1 - rate))
constexpr uint32_t DROP_RATE = 0x40000000u;    // the rate 0.25 as a 32-bit fraction
constexpr int C = ODB_MAX_C;

inline dim3 grid1(int64_t n, int nt) { return dim3((unsigned)((n + nt - 1) / nt)); }

__device__ inline float elu_(float v) { return v > 0.0f ? v : expm1f(v); }     // conv.hip's prologue
__device__ inline float elu_grad_(float v) { return v > 0.0f ? 1.0f : expf(v); }

// ---- gather -------------------------------------------------------------------------------------------

__global__ void gather_kernel(const uint8_t* __restrict__ img, const int32_t* __restrict__ labels,
                              const uint8_t* __restrict__ mask, const int32_t* __restrict__ order, int i0,
                              int nb, int n, int img_bytes, float* __restrict__ xb, int32_t* __restrict__ lb,
                              uint8_t* __restrict__ mb) {
  const int s = blockIdx.y;
  if (s >= nb) return;
  const int row = order ? min(max(order[i0 + s], 0), n - 1) : min(i0 + s, n - 1);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < img_bytes) xb[(size_t)s * img_bytes + i] = (float)img[(size_t)row * img_bytes + i];
  if (i < ODB_HEAD_D) mb[(size_t)s * ODB_HEAD_D + i] = mask ? (mask[(size_t)row * ODB_HEAD_D + i] != 0) : 1;
  if (i == 0) lb[s] = labels[row];
}

// ---- per-channel reductions over the rows of [n_pos, c] --------------------------------------------------
// workgroup = one slab of rows; thread = (channel, row split r of R = 256 / c); the R partials meet in an
// LDS tree; part[slab][q][channel]

constexpr int RD_NT = 256;
enum { RD_SUM = 0, RD_VAR = 1, RD_BNB = 2 };

template <int MODE>
__global__ void __launch_bounds__(RD_NT) colreduce_kernel(const float* __restrict__ x,
                                                          const float* __restrict__ dy,
                                                          const float* __restrict__ stat, int64_t n_pos, int c,
                                                          int64_t slab_len, float* __restrict__ part) {
  __shared__ float red[RD_NT][2];
  const int tid = threadIdx.x;
  const int ch = tid % c, r = tid / c, R = RD_NT / c;
  const int64_t p0 = (int64_t)blockIdx.x * slab_len;
  const int64_t p1 = min(n_pos, p0 + slab_len);
  float mean = 0.0f, istd = 0.0f, sc = 0.0f, sh = 0.0f;
  if (MODE != RD_SUM) mean = stat[ch];
  if (MODE == RD_BNB) {
    istd = stat[C + ch];
    sc = stat[2 * C + ch];
    sh = stat[3 * C + ch];
  }
  float s0 = 0.0f, s1 = 0.0f;
  for (int64_t p = p0 + r; p < p1; p += R) {
    const size_t at = (size_t)p * c + ch;
    const float v = x[at];
    if (MODE == RD_SUM) {
      s0 += v;
    } else if (MODE == RD_VAR) {
      const float d = v - mean;
      s0 = fmaf(d, d, s0);
    } else {
      const float g = dy[at] * elu_grad_(fmaf(v, sc, sh));
      s0 += g;
      s1 = fmaf(g, (v - mean) * istd, s1);
    }
  }
  red[tid][0] = s0;
  red[tid][1] = s1;
  for (int h = R >> 1; h >= 1; h >>= 1) {
    __syncthreads();
    if (r < h) {
      red[tid][0] += red[tid + h * c][0];
      red[tid][1] += red[tid + h * c][1];
    }
  }
  if (r == 0) {
    part[((size_t)blockIdx.x * 2) * C + ch] = red[tid][0];
    part[((size_t)blockIdx.x * 2 + 1) * C + ch] = red[tid][1];
  }
}

enum { FIN_MEAN = 0, FIN_VAR = 1, FIN_BNB = 2, FIN_DB = 3 };

// one workgroup, thread = channel: the slabs added in slab order
template <int MODE>
__global__ void __launch_bounds__(C) finalize_kernel(const float* __restrict__ part, int S, int64_t n_pos, int c,
                                                     float* __restrict__ stat, float* __restrict__ bn,
                                                     float* __restrict__ out) {
  const int ch = threadIdx.x;
  if (ch >= c) return;
  double a0 = 0.0, a1 = 0.0;
  for (int s = 0; s < S; ++s) {
    a0 += (double)part[((size_t)s * 2) * C + ch];
    a1 += (double)part[((size_t)s * 2 + 1) * C + ch];
  }
  const double n = (double)n_pos;
  if (MODE == FIN_MEAN) {
    stat[ch] = (float)(a0 / n);
  } else if (MODE == FIN_VAR) {
    const float mean = stat[ch];
    const float var = (float)(a0 / n);
    const float istd = 1.0f / sqrtf(var + BN_EPS);
    const float scale = bn[ch] * istd;
    stat[C + ch] = istd;
    stat[2 * C + ch] = scale;
    stat[3 * C + ch] = bn[c + ch] - mean * scale;
    const float unbiased = (float)(a0 / (double)max(n_pos - 1, (int64_t)1));
    bn[2 * c + ch] = 0.99f * bn[2 * c + ch] + 0.01f * mean;
    bn[3 * c + ch] = 0.99f * bn[3 * c + ch] + 0.01f * unbiased;
  } else if (MODE == FIN_BNB) {
    out[ch] = (float)a1;
    out[c + ch] = (float)a0;
    stat[4 * C + ch] = (float)(a0 / n);
    stat[5 * C + ch] = (float)(a1 / n);
  } else {
    out[ch] = (float)a0;
  }
}

__global__ void bn_moving_kernel(const float* __restrict__ bn, int c, float* __restrict__ stat) {
  const int ch = threadIdx.x;
  if (ch >= c) return;
  const float mean = bn[2 * c + ch];
  const float istd = 1.0f / sqrtf(bn[3 * c + ch] + BN_EPS);
  const float scale = bn[ch] * istd;
  stat[ch] = mean;
  stat[C + ch] = istd;
  stat[2 * C + ch] = scale;
  stat[3 * C + ch] = bn[c + ch] - mean * scale;
}

__global__ void bn_elu_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                  const float* __restrict__ stat, const float* add, float* dx, int64_t n,
                                  int c) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int ch = (int)(i % c);
  const float mean = stat[ch], istd = stat[C + ch], sc = stat[2 * C + ch], sh = stat[3 * C + ch];
  const float mg = stat[4 * C + ch], mgx = stat[5 * C + ch];
  const float v = x[i];
  const float g = dy[i] * elu_grad_(fmaf(v, sc, sh));
  const float xh = (v - mean) * istd;
  const float d = sc * (g - mg - xh * mgx);
  dx[i] = add ? d + add[i] : d;
}

// ---- weight gradient on the f32 MFMA ----------------------------------------------------------------------
// workgroup = one slab of output pixels x four (tap, 32 input channels) combinations, one per wave; a wave
// holds the NTL tiles of 32 output channels of its combination.  Per pair of pixels a lane loads one value of
// a (pixel = lane >> 5, channel = lane & 31) and NTL of dy, then issues NTL MFMAs.  No LDS, no barrier.

constexpr int WG_NT = 256;

template <int NTL, bool PRO>
__global__ void __launch_bounds__(WG_NT) wgrad_kernel(OdbConv g, const float* __restrict__ x,
                                                      const float* __restrict__ scale,
                                                      const float* __restrict__ shift,
                                                      const float* __restrict__ dy, int slab_len,
                                                      float* __restrict__ part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ci_tiles = (g.cin + 31) / 32;
  const int taps = g.kh * g.kw;
  const int combo = blockIdx.y * 4 + wave;
  if (combo >= taps * ci_tiles) return;   // whole waves leave together
  const int tap = combo / ci_tiles, cit = combo - tap * ci_tiles;
  const int tdy = tap / g.kw, tdx = tap - tdy * g.kw;
  const int col = lane & 31, half = lane >> 5;
  const int ci = cit * 32 + col;
  const bool ci_ok = ci < g.cin;
  float sc = 0.0f, sh = 0.0f;
  if (PRO && ci_ok) {
    sc = scale[ci];
    sh = shift[ci];
  }
  const int64_t P = (int64_t)g.B * g.ho * g.wo;
  const int64_t p0 = (int64_t)blockIdx.x * slab_len;
  const int64_t p1 = min(P, p0 + slab_len);
  const int hw = g.ho * g.wo;

  f32x16 acc[NTL];
#pragma unroll
  for (int t = 0; t < NTL; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;

  for (int64_t pb = p0; pb < p1; pb += 2) {
    const int64_t p = pb + half;
    float av = 0.0f;
    float bv[NTL];
#pragma unroll
    for (int t = 0; t < NTL; ++t) bv[t] = 0.0f;
    if (p < p1) {
      const int n = (int)(p / hw);
      const int rem = (int)(p - (int64_t)n * hw);
      const int ho = rem / g.wo, wo = rem - ho * g.wo;
      const int hi = ho * g.stride + tdy - g.pad_h, wi = wo * g.stride + tdx - g.pad_w;
      if (ci_ok && hi >= 0 && hi < g.h && wi >= 0 && wi < g.w) {
        const float v = x[(((size_t)n * g.h + hi) * g.w + wi) * g.cin + ci];
        av = PRO ? elu_(fmaf(v, sc, sh)) : v;
      }
#pragma unroll
      for (int t = 0; t < NTL; ++t) {
        const int co = t * 32 + col;
        if (co < g.cout) bv[t] = dy[(size_t)p * g.cout + co];
      }
    }
#pragma unroll
    for (int t = 0; t < NTL; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[t], acc[t], 0, 0, 0);
  }

  // acc register r of a lane holds row (r & 3) + 8 (r >> 2) + 4 (lane >> 5), column lane & 31
  float* __restrict__ out = part + ((size_t)blockIdx.x * taps + tap) * g.cin * g.cout;
#pragma unroll
  for (int t = 0; t < NTL; ++t) {
    const int co = t * 32 + col;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int cir = cit * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      if (cir < g.cin && co < g.cout) out[(size_t)cir * g.cout + co] = acc[t][r];
    }
  }
}

__global__ void slab_sum_kernel(const float* __restrict__ part, int S, int n, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double a = 0.0;
  for (int s = 0; s < S; ++s) a += (double)part[(size_t)s * n + i];
  out[i] = (float)a;
}

// ---- kernel copies ----------------------------------------------------------------------------------------

__global__ void conv_transpose_kernel(OdbConv g, int cin_pad, const float* __restrict__ w,
                                      float* __restrict__ wt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int taps = g.kh * g.kw;
  if (i >= taps * g.cout * cin_pad) return;
  const int ci = i % cin_pad, co = (i / cin_pad) % g.cout, tapf = i / (cin_pad * g.cout);
  const int tap = taps - 1 - tapf;   // (kh - 1 - dy) kw + (kw - 1 - dx) = taps - 1 - (dy kw + dx)
  wt[i] = ci < g.cin ? w[((size_t)tap * g.cin + ci) * g.cout + co] : 0.0f;
}

__global__ void pad_cols_kernel(const float* __restrict__ in, int rows, int cols, int cols_pad,
                                float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * cols_pad) return;
  const int col = i % cols_pad, row = i / cols_pad;
  out[i] = col < cols ? in[(size_t)row * cols + col] : 0.0f;
}

__global__ void shortcut_bwd_data_kernel(OdbConv g, int cin_pad, const float* __restrict__ dy,
                                         const float* __restrict__ wt, float* __restrict__ dx) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)g.B * g.h * g.w * g.cin) return;
  const int ci = (int)(i % g.cin);
  const int64_t p = i / g.cin;
  const int ww = (int)(p % g.w), hh = (int)((p / g.w) % g.h), b = (int)(p / ((int64_t)g.w * g.h));
  float acc = 0.0f;
  if (!(hh & 1) && !(ww & 1)) {
    const float* __restrict__ dr = dy + (((size_t)b * g.ho + hh / 2) * g.wo + ww / 2) * g.cout;
#pragma unroll 4
    for (int co = 0; co < g.cout; ++co) acc = fmaf(dr[co], wt[(size_t)co * cin_pad + ci], acc);
  }
  dx[i] = acc;
}

// ---- pools ------------------------------------------------------------------------------------------------

__global__ void pool_winner_kernel(const float* __restrict__ x, uint8_t* __restrict__ idx, int B, int h, int w,
                                   int c) {
  const int ho = (h + 1) / 2, wo = (w + 1) / 2;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * ho * wo * c) return;
  const int ch = (int)(i % c);
  const int64_t p = i / c;
  const int ow = (int)(p % wo), oh = (int)((p / wo) % ho), b = (int)(p / ((int64_t)wo * ho));
  float best = 0.0f;
  int arg = -1;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int hh = 2 * oh + (k >> 1), ww = 2 * ow + (k & 1);
    if (hh < h && ww < w) {
      const float v = x[(((size_t)b * h + hh) * w + ww) * c + ch];
      if (arg < 0 || v > best) {
        best = v;
        arg = k;
      }
    }
  }
  idx[i] = (uint8_t)arg;   // (2 oh, 2 ow) is always inside: arg >= 0
}

__global__ void pool_bwd_kernel(const float* __restrict__ dy, const uint8_t* __restrict__ idx,
                                float* __restrict__ dx, int B, int h, int w, int c) {
  const int ho = (h + 1) / 2, wo = (w + 1) / 2;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * h * w * c) return;
  const int ch = (int)(i % c);
  const int64_t p = i / c;
  const int ww = (int)(p % w), hh = (int)((p / w) % h), b = (int)(p / ((int64_t)w * h));
  const size_t o = (((size_t)b * ho + hh / 2) * wo + ww / 2) * c + ch;
  dx[i] = idx[o] == (uint8_t)((hh & 1) * 2 + (ww & 1)) ? dy[o] : 0.0f;
}

__global__ void mean_h_kernel(const float* __restrict__ x, float* __restrict__ seq, int B, int h, int w, int c) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // over [B, w, c]
  if (i >= (int64_t)B * w * c) return;
  const int64_t wc = (int64_t)w * c;
  const int b = (int)(i / wc);
  const float* __restrict__ xr = x + (size_t)b * h * wc + (i - b * wc);
  float acc = 0.0f;
  for (int hh = 0; hh < h; ++hh) acc += xr[(size_t)hh * wc];
  seq[i] = acc / (float)h;
}

__global__ void mean_h_bwd_kernel(const float* __restrict__ dxs, float* __restrict__ dx, int B, int h, int w,
                                  int c) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // over [B, h, w, c]
  const int64_t wc = (int64_t)w * c;
  if (i >= (int64_t)B * h * wc) return;
  const int b = (int)(i / (h * wc));
  const size_t at = (size_t)b * wc + (size_t)(i % wc);
  dx[i] = (dxs[at] + dxs[(size_t)B * wc + at]) / (float)h;
}

// ---- head -------------------------------------------------------------------------------------------------
// weighted_categorical_crossentropy (overlap_detector.py:62-79) on softmax(Dense(LeakyReLU(Dropout(emb)))):
// p <- p / sum p, clip to [1e-7, 1 - 1e-7], -w_c log p_c; the gradient at the logits is zero for a sample
// whose p_c is outside the clip range.  One workgroup, thread = sample (B <= 64).

__device__ inline float head_in(const OdbHead& a, int s, int d, float* slope) {
  float v = a.emb[(size_t)s * ODB_HEAD_D + d];
  float k = 1.0f;
  if (a.mask) k = a.mask[(size_t)s * ODB_HEAD_D + d] ? KEEP_SCALE : 0.0f;
  v *= k;
  const float l = v > 0.0f ? 1.0f : LEAKY;
  *slope = l * k;
  return v * l;
}

__global__ void __launch_bounds__(ODB_MAX_BATCH) head_loss_kernel(OdbHead a) {
  __shared__ float loss[ODB_MAX_BATCH];
  __shared__ int hit[ODB_MAX_BATCH];
  const int s = threadIdx.x;
  const float lo = 1e-7f, hi = 1.0f - 1e-7f;
  float l = 0.0f;
  int h = 0;
  if (s < a.B) {
    float z0 = a.b[0], z1 = a.b[1], slope;
    for (int d = 0; d < ODB_HEAD_D; ++d) {
      const float v = head_in(a, s, d, &slope);
      z0 = fmaf(v, a.w[2 * d], z0);
      z1 = fmaf(v, a.w[2 * d + 1], z1);
    }
    const float m = fmaxf(z0, z1);
    const float e0 = expf(z0 - m), e1 = expf(z1 - m);
    const float p0 = e0 / (e0 + e1), p1 = e1 / (e0 + e1);
    const float q0 = p0 / (p0 + p1), q1 = p1 / (p0 + p1);
    const int c = a.labels[s] & 1;
    const float pc = c ? q1 : q0, wc = c ? a.cw[1] : a.cw[0];
    const bool inside = pc >= lo && pc <= hi;
    l = wc * (float)(-log((double)fminf(fmaxf(pc, lo), hi)));
    h = (q1 > q0 ? 1 : 0) == c ? 1 : 0;
    if (a.probs) {
      a.probs[2 * s] = p0;
      a.probs[2 * s + 1] = p1;
    }
    if (a.dz) {
      a.dz[2 * s] = inside ? wc * (q0 - (c == 0 ? 1.0f : 0.0f)) / a.bsz : 0.0f;
      a.dz[2 * s + 1] = inside ? wc * (q1 - (c == 1 ? 1.0f : 0.0f)) / a.bsz : 0.0f;
    }
  }
  loss[s] = l;
  hit[s] = h;
  __syncthreads();
  if (s == 0) {
    double lsum = 0.0;
    int hits = 0;
    for (int q = 0; q < a.B && q < ODB_MAX_BATCH; ++q) {
      lsum += (double)loss[q];
      hits += hit[q];
    }
    a.acc[0] += lsum;
    a.acc[1] += (double)hits;
  }
}

__global__ void head_bwd_kernel(OdbHead a, float* __restrict__ gw, float* __restrict__ gb,
                                float* __restrict__ demb) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int nw = ODB_HEAD_D * 2;
  float slope;
  if (i < nw) {
    const int d = i >> 1, k = i & 1;
    float acc = 0.0f;
    for (int b = 0; b < a.B; ++b) acc = fmaf(head_in(a, b, d, &slope), a.dz[2 * b + k], acc);
    gw[i] = acc;
  } else if (i < nw + 2) {
    const int k = i - nw;
    float acc = 0.0f;
    for (int b = 0; b < a.B; ++b) acc += a.dz[2 * b + k];
    gb[k] = acc;
  } else if (i < nw + 2 + a.B * ODB_HEAD_D) {
    const int q = i - nw - 2;
    const int b = q / ODB_HEAD_D, d = q % ODB_HEAD_D;
    (void)head_in(a, b, d, &slope);
    demb[q] = fmaf(a.dz[2 * b], a.w[2 * d], a.dz[2 * b + 1] * a.w[2 * d + 1]) * slope;
  }
}

// The K-class head (2 < K <= ODB_MAX_K).  The per-class values live in registers: every loop over the classes
// is unrolled to ODB_MAX_K and cut at K.  A label outside [0, K - 1] (a device-pointer caller's broken
// contract) is clamped into it.

__device__ inline int clamp_label(int l, int K) { return l < 0 ? 0 : l > K - 1 ? K - 1 : l; }

__global__ void __launch_bounds__(ODB_MAX_BATCH) head_loss_k_kernel(OdbHead a) {
  __shared__ float loss[ODB_MAX_BATCH];
  __shared__ int hit[ODB_MAX_BATCH];
  const int s = threadIdx.x, K = a.K;
  const float lo = 1e-7f, hi = 1.0f - 1e-7f;
  float l = 0.0f;
  int h = 0;
  if (s < a.B) {
    float z[ODB_MAX_K], slope;
#pragma unroll
    for (int k = 0; k < ODB_MAX_K; ++k) z[k] = k < K ? a.b[k] : 0.0f;
    for (int d = 0; d < ODB_HEAD_D; ++d) {
      const float v = head_in(a, s, d, &slope);
#pragma unroll
      for (int k = 0; k < ODB_MAX_K; ++k)
        if (k < K) z[k] = fmaf(v, a.w[K * d + k], z[k]);
    }
    float m = z[0];
#pragma unroll
    for (int k = 1; k < ODB_MAX_K; ++k)
      if (k < K) m = fmaxf(m, z[k]);
    float se = 0.0f, sp = 0.0f;
#pragma unroll
    for (int k = 0; k < ODB_MAX_K; ++k)
      if (k < K) {
        z[k] = expf(z[k] - m);
        se += z[k];
      }
#pragma unroll
    for (int k = 0; k < ODB_MAX_K; ++k)
      if (k < K) {
        z[k] = z[k] / se;   // p_k
        sp += z[k];
      }
    const int c = clamp_label(a.labels[s], K);
    float pc = 0.0f, wc = 0.0f, qbest = 0.0f;
    int best = 0;
#pragma unroll
    for (int k = 0; k < ODB_MAX_K; ++k)
      if (k < K) {
        if (a.probs) a.probs[K * s + k] = z[k];
        z[k] = z[k] / sp;   // q_k
        if (k == c) {
          pc = z[k];
          wc = a.cw[k];
        }
        if (k == 0 || z[k] > qbest) {
          qbest = z[k];
          best = k;
        }
      }
    const bool inside = pc >= lo && pc <= hi;
    l = wc * (float)(-log((double)fminf(fmaxf(pc, lo), hi)));
    h = best == c ? 1 : 0;
    if (a.dz) {
#pragma unroll
      for (int k = 0; k < ODB_MAX_K; ++k)
        if (k < K) a.dz[K * s + k] = inside ? wc * (z[k] - (k == c ? 1.0f : 0.0f)) / a.bsz : 0.0f;
    }
  }
  loss[s] = l;
  hit[s] = h;
  __syncthreads();
  if (s == 0) {
    double lsum = 0.0;
    int hits = 0;
    for (int q = 0; q < a.B && q < ODB_MAX_BATCH; ++q) {
      lsum += (double)loss[q];
      hits += hit[q];
    }
    a.acc[0] += lsum;
    a.acc[1] += (double)hits;
  }
}

__global__ void head_bwd_k_kernel(OdbHead a, float* __restrict__ gw, float* __restrict__ gb,
                                  float* __restrict__ demb) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int K = a.K, nw = ODB_HEAD_D * K;
  float slope;
  if (i < nw) {
    const int d = i / K, k = i % K;
    float acc = 0.0f;
    for (int b = 0; b < a.B; ++b) acc = fmaf(head_in(a, b, d, &slope), a.dz[K * b + k], acc);
    gw[i] = acc;
  } else if (i < nw + K) {
    const int k = i - nw;
    float acc = 0.0f;
    for (int b = 0; b < a.B; ++b) acc += a.dz[K * b + k];
    gb[k] = acc;
  } else if (i < nw + K + a.B * ODB_HEAD_D) {
    const int q = i - nw - K;
    const int b = q / ODB_HEAD_D, d = q % ODB_HEAD_D;
    (void)head_in(a, b, d, &slope);
    float acc = 0.0f;
    for (int k = 0; k < K; ++k) acc = fmaf(a.dz[K * b + k], a.w[K * d + k], acc);
    demb[q] = acc * slope;
  }
}

// ---- Adadelta, bookkeeping ---------------------------------------------------------------------------------

__global__ void adadelta_kernel(float* __restrict__ w, float* __restrict__ acc_g, float* __restrict__ acc_d,
                                const float* __restrict__ g, const uint8_t* __restrict__ trainable, int64_t n,
                                const float* __restrict__ lrs, int ep) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !trainable[i]) return;
  const float rho = 0.95f, eps = 1e-7f, lr = lrs[ep];
  const float gv = g[i];
  const float a = rho * acc_g[i] + (1.0f - rho) * (gv * gv);
  const float d = acc_d[i];
  const float u = sqrtf(d + eps) / sqrtf(a + eps) * gv;
  acc_g[i] = a;
  w[i] -= lr * u;
  acc_d[i] = rho * d + (1.0f - rho) * (u * u);
}

__global__ void end_epoch_kernel(double* st, int n_train, int n_val, const float* lrs, int ep, float* row) {
  row[0] = (float)(st[3] / n_train);
  row[1] = (float)(st[4] / n_train);
  row[2] = n_val > 0 ? (float)(st[5] / n_val) : __builtin_nanf("");
  row[3] = n_val > 0 ? (float)(st[6] / n_val) : __builtin_nanf("");
  row[4] = lrs[ep];
  for (int i = 0; i < 8; ++i) st[i] = 0.0;
}

__global__ void loss_out_kernel(const double* st, int n, float* loss) { loss[0] = (float)(st[0] / n); }

__global__ void fill_kernel(float* p, int64_t n, float v) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// ---- keep-bits and the AUC metric of a fit from scratch ----------------------------------------------------

// thread = (sample, four elements): one Philox block
__global__ void drop_mask_kernel(uint64_t seed, uint32_t epoch, const int32_t* __restrict__ sid, int n,
                                 uint8_t* __restrict__ mask) {
  constexpr int Q = ODB_HEAD_D / 4;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)n * Q) return;
  const int s = (int)(i / Q), q = (int)(i % Q);
  const U4 r = philox_drop_words(seed, epoch, (uint32_t)sid[s], (uint32_t)q, 2u);
  uint8_t* out = mask + (size_t)s * ODB_HEAD_D + 4 * q;
#pragma unroll
  for (int k = 0; k < 4; ++k) out[k] = r.v[k] >= DROP_RATE ? 1 : 0;
}

constexpr int AUC_NT = 256;

// workgroup = one slab of rows, thread = one threshold
__global__ void __launch_bounds__(AUC_NT) auc_count_kernel(const float* __restrict__ probs,
                                                           const int32_t* __restrict__ labels, int64_t n,
                                                           int64_t slab_len, OdbAucThr thr, int add,
                                                           uint32_t* __restrict__ counts) {
  const int t = threadIdx.x;
  if (t >= ODB_AUC_T) return;
  const float th = thr.t[t];
  const int64_t r0 = (int64_t)blockIdx.x * slab_len, r1 = min(n, r0 + slab_len);
  uint32_t tp = 0, fp = 0;
  for (int64_t r = r0; r < r1; ++r) {
    const int c = labels[r] & 1;
    const bool pos0 = probs[2 * r] > th, pos1 = probs[2 * r + 1] > th;
    tp += (c ? pos1 : pos0) ? 1u : 0u;   // the entry whose one-hot label is 1
    fp += (c ? pos0 : pos1) ? 1u : 0u;
  }
  uint32_t* out = counts + ((size_t)blockIdx.x * ODB_AUC_T + t) * 2;
  out[0] = add ? out[0] + tp : tp;
  out[1] = add ? out[1] + fp : fp;
}

// K classes (2 < K <= ODB_MAX_K): the label's entry counts towards TP, the K - 1 others towards FP
__global__ void __launch_bounds__(AUC_NT) auc_count_k_kernel(const float* __restrict__ probs,
                                                             const int32_t* __restrict__ labels, int64_t n, int K,
                                                             int64_t slab_len, OdbAucThr thr, int add,
                                                             uint32_t* __restrict__ counts) {
  const int t = threadIdx.x;
  if (t >= ODB_AUC_T) return;
  const float th = thr.t[t];
  const int64_t r0 = (int64_t)blockIdx.x * slab_len, r1 = min(n, r0 + slab_len);
  uint32_t tp = 0, fp = 0;
  for (int64_t r = r0; r < r1; ++r) {
    const int c = clamp_label(labels[r], K);
    for (int k = 0; k < K; ++k) {
      const uint32_t pos = probs[K * r + k] > th ? 1u : 0u;
      tp += k == c ? pos : 0u;
      fp += k == c ? 0u : pos;
    }
  }
  uint32_t* out = counts + ((size_t)blockIdx.x * ODB_AUC_T + t) * 2;
  out[0] = add ? out[0] + tp : tp;
  out[1] = add ? out[1] + fp : fp;
}

__global__ void __launch_bounds__(AUC_NT) auc_final_kernel(uint32_t* counts, int slabs, int64_t n, int64_t n_neg,
                                                           int clear, float* __restrict__ out) {
  __shared__ double rec[ODB_AUC_T], fpr[ODB_AUC_T];
  const int t = threadIdx.x;
  if (t < ODB_AUC_T) {
    uint64_t tp = 0, fp = 0;
    for (int q = 0; q < slabs; ++q) {
      uint32_t* at = counts + ((size_t)q * ODB_AUC_T + t) * 2;
      tp += at[0];
      fp += at[1];
      if (clear) at[0] = at[1] = 0u;
    }
    rec[t] = n > 0 ? (double)tp / (double)n : 0.0;
    fpr[t] = n > 0 ? (double)fp / (double)n_neg : 0.0;
  }
  __syncthreads();
  if (t != 0) return;
  double auc = 0.0;
  for (int q = 0; q + 1 < ODB_AUC_T; ++q) auc += (fpr[q] - fpr[q + 1]) * (rec[q] + rec[q + 1]) / 2.0;
  out[0] = n > 0 ? (float)auc : __builtin_nanf("");
}

inline bool bn_width_ok(int c) { return c == 16 || c == 32 || c == 64 || c == 128; }

// slabs of a per-channel reduction over n_pos rows
inline void red_slabs(int64_t n_pos, int* S, int64_t* len) {
  int64_t s = (n_pos + 511) / 512;
  s = s < 1 ? 1 : s > ODB_RED_SLABS ? ODB_RED_SLABS : s;
  *len = (n_pos + s - 1) / s;
  if (*len < 1) *len = 1;
  *S = (int)((n_pos + *len - 1) / *len);
  if (*S < 1) *S = 1;
}

inline void wg_slabs(int64_t P, int* S, int* len) {
  int64_t s = (P + 255) / 256;
  s = s < 1 ? 1 : s > ODB_WG_SLABS ? ODB_WG_SLABS : s;
  int64_t l = (P + s - 1) / s;
  l = (l + 1) & ~(int64_t)1;
  if (l < 2) l = 2;
  *len = (int)l;
  *S = (int)((P + l - 1) / l);
  if (*S < 1) *S = 1;
}

}  // namespace

#define ODB_LAUNCH(kernel, grid, block, ...)                            \
  do {                                                                  \
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, __VA_ARGS__);    \
    const hipError_t e_ = hipGetLastError();                            \
    if (e_ != hipSuccess) return e_;                                    \
  } while (0)

hipError_t odb_gather(const uint8_t* img, const int32_t* labels, const uint8_t* mask, const int32_t* order,
                      int i0, int nb, int n, int img_bytes, float* xb, int32_t* lb, uint8_t* mb,
                      hipStream_t stream) {
  const int span = img_bytes > ODB_HEAD_D ? img_bytes : ODB_HEAD_D;
  ODB_LAUNCH(gather_kernel, dim3((span + 255) / 256, nb), dim3(256), img, labels, mask, order, i0, nb, n,
             img_bytes, xb, lb, mb);
  return hipSuccess;
}

hipError_t odb_bn_batch(const float* x, int64_t n_pos, int c, float* bn, float* stat, float* part,
                        hipStream_t stream) {
  if (!bn_width_ok(c) || n_pos < 1) return hipErrorInvalidValue;
  int S;
  int64_t len;
  red_slabs(n_pos, &S, &len);
  ODB_LAUNCH(colreduce_kernel<RD_SUM>, dim3(S), dim3(RD_NT), x, nullptr, stat, n_pos, c, len, part);
  ODB_LAUNCH(finalize_kernel<FIN_MEAN>, dim3(1), dim3(C), part, S, n_pos, c, stat, bn, nullptr);
  ODB_LAUNCH(colreduce_kernel<RD_VAR>, dim3(S), dim3(RD_NT), x, nullptr, stat, n_pos, c, len, part);
  ODB_LAUNCH(finalize_kernel<FIN_VAR>, dim3(1), dim3(C), part, S, n_pos, c, stat, bn, nullptr);
  return hipSuccess;
}

hipError_t odb_bn_moving(const float* bn, int c, float* stat, hipStream_t stream) {
  if (!bn_width_ok(c)) return hipErrorInvalidValue;
  ODB_LAUNCH(bn_moving_kernel, dim3(1), dim3(C), bn, c, stat);
  return hipSuccess;
}

hipError_t odb_bn_elu_bwd(const float* x, const float* dy, int64_t n_pos, int c, float* stat, float* part,
                          const float* add, float* dx, float* dbn, hipStream_t stream) {
  if (!bn_width_ok(c) || n_pos < 1) return hipErrorInvalidValue;
  int S;
  int64_t len;
  red_slabs(n_pos, &S, &len);
  ODB_LAUNCH(colreduce_kernel<RD_BNB>, dim3(S), dim3(RD_NT), x, dy, stat, n_pos, c, len, part);
  ODB_LAUNCH(finalize_kernel<FIN_BNB>, dim3(1), dim3(C), part, S, n_pos, c, stat, nullptr, dbn);
  ODB_LAUNCH(bn_elu_bwd_kernel, grid1(n_pos * c, 256), dim3(256), x, dy, stat, add, dx, n_pos * c, c);
  return hipSuccess;
}

hipError_t odb_bias_grad(const float* dy, int64_t n_pos, int c, float* part, float* db, hipStream_t stream) {
  if (!bn_width_ok(c) || n_pos < 1) return hipErrorInvalidValue;
  int S;
  int64_t len;
  red_slabs(n_pos, &S, &len);
  ODB_LAUNCH(colreduce_kernel<RD_SUM>, dim3(S), dim3(RD_NT), dy, nullptr, nullptr, n_pos, c, len, part);
  ODB_LAUNCH(finalize_kernel<FIN_DB>, dim3(1), dim3(C), part, S, n_pos, c, nullptr, nullptr, db);
  return hipSuccess;
}

int odb_wgrad_slabs(int64_t P) {
  int S, len;
  wg_slabs(P, &S, &len);
  return S;
}

size_t odb_wgrad_part_floats(const OdbConv& g) {
  return (size_t)odb_wgrad_slabs((int64_t)g.B * g.ho * g.wo) * g.kh * g.kw * g.cin * g.cout;
}

hipError_t odb_conv_wgrad(const OdbConv& g, const float* x, const float* scale, const float* shift,
                          const float* dy, float* part, float* dw, hipStream_t stream) {
  const int64_t P = (int64_t)g.B * g.ho * g.wo;
  if (P < 1 || g.cin < 1 || g.cout < 1 || g.cout > ODB_MAX_C || g.cin > ODB_MAX_C) return hipErrorInvalidValue;
  int S, len;
  wg_slabs(P, &S, &len);
  const int combos = g.kh * g.kw * ((g.cin + 31) / 32);
  const dim3 grid(S, (combos + 3) / 4);
  const int ntl = (g.cout + 31) / 32;
  const bool pro = scale != nullptr;
#define ODB_WG_CASE(N)                                                                                    \
  if (ntl == N) {                                                                                         \
    if (pro)                                                                                              \
      ODB_LAUNCH((wgrad_kernel<N, true>), grid, dim3(WG_NT), g, x, scale, shift, dy, len, part);          \
    else                                                                                                  \
      ODB_LAUNCH((wgrad_kernel<N, false>), grid, dim3(WG_NT), g, x, scale, shift, dy, len, part);         \
  }
  ODB_WG_CASE(1)
  ODB_WG_CASE(2)
  ODB_WG_CASE(3)
  ODB_WG_CASE(4)
#undef ODB_WG_CASE
  const int n = g.kh * g.kw * g.cin * g.cout;
  ODB_LAUNCH(slab_sum_kernel, grid1(n, 256), dim3(256), part, S, n, dw);
  return hipSuccess;
}

hipError_t odb_conv_transpose(const OdbConv& g, int cin_pad, const float* w, float* wt, hipStream_t stream) {
  if (cin_pad < g.cin) return hipErrorInvalidValue;
  ODB_LAUNCH(conv_transpose_kernel, grid1((int64_t)g.kh * g.kw * g.cout * cin_pad, 256), dim3(256), g, cin_pad,
             w, wt);
  return hipSuccess;
}

hipError_t odb_pad_cols(const float* in, int rows, int cols, int cols_pad, float* out, hipStream_t stream) {
  if (cols_pad < cols) return hipErrorInvalidValue;
  ODB_LAUNCH(pad_cols_kernel, grid1((int64_t)rows * cols_pad, 256), dim3(256), in, rows, cols, cols_pad, out);
  return hipSuccess;
}

hipError_t odb_shortcut_bwd_data(const OdbConv& g, int cin_pad, const float* dy, const float* wt, float* dx,
                                 hipStream_t stream) {
  if (g.stride != 2 || g.kh != 1 || g.kw != 1 || g.ho != (g.h + 1) / 2 || g.wo != (g.w + 1) / 2 ||
      cin_pad < g.cin)
    return hipErrorInvalidValue;
  ODB_LAUNCH(shortcut_bwd_data_kernel, grid1((int64_t)g.B * g.h * g.w * g.cin, 256), dim3(256), g, cin_pad, dy,
             wt, dx);
  return hipSuccess;
}

hipError_t odb_pool_winner(const float* x, uint8_t* idx, int B, int h, int w, int c, hipStream_t stream) {
  const int64_t n = (int64_t)B * ((h + 1) / 2) * ((w + 1) / 2) * c;
  ODB_LAUNCH(pool_winner_kernel, grid1(n, 256), dim3(256), x, idx, B, h, w, c);
  return hipSuccess;
}

hipError_t odb_pool_bwd(const float* dy, const uint8_t* idx, float* dx, int B, int h, int w, int c,
                        hipStream_t stream) {
  ODB_LAUNCH(pool_bwd_kernel, grid1((int64_t)B * h * w * c, 256), dim3(256), dy, idx, dx, B, h, w, c);
  return hipSuccess;
}

hipError_t odb_mean_h(const float* x, float* seq, int B, int h, int w, int c, hipStream_t stream) {
  ODB_LAUNCH(mean_h_kernel, grid1((int64_t)B * w * c, 256), dim3(256), x, seq, B, h, w, c);
  return hipSuccess;
}

hipError_t odb_mean_h_bwd(const float* dxs, float* dx, int B, int h, int w, int c, hipStream_t stream) {
  ODB_LAUNCH(mean_h_bwd_kernel, grid1((int64_t)B * h * w * c, 256), dim3(256), dxs, dx, B, h, w, c);
  return hipSuccess;
}

hipError_t odb_head_loss(const OdbHead& a, hipStream_t stream) {
  if (a.B < 1 || a.B > ODB_MAX_BATCH || a.K < 2 || a.K > ODB_MAX_K) return hipErrorInvalidValue;
  if (a.K == 2)
    ODB_LAUNCH(head_loss_kernel, dim3(1), dim3(ODB_MAX_BATCH), a);
  else
    ODB_LAUNCH(head_loss_k_kernel, dim3(1), dim3(ODB_MAX_BATCH), a);
  return hipSuccess;
}

hipError_t odb_head_bwd(const OdbHead& a, float* gw, float* gb, float* demb, hipStream_t stream) {
  if (a.B < 1 || a.B > ODB_MAX_BATCH || !a.dz || a.K < 2 || a.K > ODB_MAX_K) return hipErrorInvalidValue;
  const dim3 grid = grid1((int64_t)ODB_HEAD_D * a.K + a.K + (int64_t)a.B * ODB_HEAD_D, 256);
  if (a.K == 2)
    ODB_LAUNCH(head_bwd_kernel, grid, dim3(256), a, gw, gb, demb);
  else
    ODB_LAUNCH(head_bwd_k_kernel, grid, dim3(256), a, gw, gb, demb);
  return hipSuccess;
}

hipError_t odb_adadelta(float* w, float* acc_g, float* acc_d, const float* g, const uint8_t* trainable,
                        int64_t n, const float* lrs, int ep, hipStream_t stream) {
  ODB_LAUNCH(adadelta_kernel, grid1(n, 256), dim3(256), w, acc_g, acc_d, g, trainable, n, lrs, ep);
  return hipSuccess;
}

hipError_t odb_end_epoch(double* st, int n_train, int n_val, const float* lrs, int ep, float* row,
                         hipStream_t stream) {
  ODB_LAUNCH(end_epoch_kernel, dim3(1), dim3(1), st, n_train, n_val, lrs, ep, row);
  return hipSuccess;
}

hipError_t odb_loss_out(const double* st, int n, float* loss, hipStream_t stream) {
  ODB_LAUNCH(loss_out_kernel, dim3(1), dim3(1), st, n, loss);
  return hipSuccess;
}

hipError_t odb_fill(float* p, int64_t n, float v, hipStream_t stream) {
  if (n < 1) return hipSuccess;
  ODB_LAUNCH(fill_kernel, grid1(n, 256), dim3(256), p, n, v);
  return hipSuccess;
}

hipError_t odb_drop_mask(uint64_t seed, uint32_t epoch, const int32_t* sid, int n, uint8_t* mask,
                         hipStream_t stream) {
  if (n < 1) return hipErrorInvalidValue;
  ODB_LAUNCH(drop_mask_kernel, grid1((int64_t)n * (ODB_HEAD_D / 4), 256), dim3(256), seed, epoch, sid, n, mask);
  return hipSuccess;
}

OdbAucThr odb_auc_thresholds() {
  OdbAucThr thr;
  thr.t[0] = (float)(0.0 - 1e-7);
  for (int i = 0; i < ODB_AUC_T - 2; ++i) thr.t[i + 1] = (float)((double)(i + 1) / 199.0);
  thr.t[ODB_AUC_T - 1] = (float)(1.0 + 1e-7);
  return thr;
}

int odb_auc_slabs(int64_t n) {
  const int64_t s = (n + 4095) / 4096;
  return (int)(s < 1 ? 1 : s > ODB_AUC_SLABS ? ODB_AUC_SLABS : s);
}

hipError_t odb_auc_count(const float* probs, const int32_t* labels, int64_t n, int K, const OdbAucThr& thr, int add,
                         uint32_t* counts, hipStream_t stream) {
  if (n < 1 || K < 2 || K > ODB_MAX_K) return hipErrorInvalidValue;
  const int S = odb_auc_slabs(n);
  const int64_t len = (n + S - 1) / S;   // ceil: slabs * len >= n, and every slab starts inside the rows
  if (K == 2)
    ODB_LAUNCH(auc_count_kernel, dim3(S), dim3(AUC_NT), probs, labels, n, len, thr, add, counts);
  else
    ODB_LAUNCH(auc_count_k_kernel, dim3(S), dim3(AUC_NT), probs, labels, n, K, len, thr, add, counts);
  return hipSuccess;
}

hipError_t odb_auc_final(uint32_t* counts, int slabs, int64_t n, int K, int clear, float* out, hipStream_t stream) {
  if (slabs < 1 || slabs > ODB_AUC_SLABS || K < 2 || K > ODB_MAX_K) return hipErrorInvalidValue;
  ODB_LAUNCH(auc_final_kernel, dim3(1), dim3(AUC_NT), counts, slabs, n, n * (int64_t)(K - 1), clear, out);
  return hipSuccess;
}
