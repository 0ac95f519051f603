// Training the SI base model from scratch (speaker_identification.py:221-250, res_model :115-219): the
// layers that `train` runs differently from the fine-tune of si_bwd.hip.  Keras calls the network with
// training=True there, so BatchNorm normalises with the statistics of the batch and the two Dropout
// layers are live; the head is the 630-way softmax of TIMIT.
//
// BatchNorm: the sums over the B * T positions are split into S = min(256, ceil(n_pos / 64)) slabs of
// consecutive rows, one workgroup per (32 channels, slab); inside a workgroup 16 threads per channel walk
// the slab's rows in ascending order and their partials are added in LDS in a fixed binary tree.  The
// consumer of a sum adds the S slab partials in slab order -- every workgroup that needs the sum repeats
// that same serial addition, so all of them see the same bits and no launch exists only to finalise.  S
// depends on the shape alone: the same inputs give the same bits, and no atomics are used.
//
// Dropout: no mask array.  A keep-bit is a word of Philox4x32-10 (philox.h) keyed by the
// fit's seed and counted by (element / 4, sample id, epoch, site), recomputed wherever it is needed: in
// the forward and backward of the avg-pool (site 0) and in the head (site 1).  sbb_drop_mask writes the
// same bits out as bytes for the tests.
//
// Head: one workgroup per sample; lanes stride over the classes, the logits stay in LDS, and the running
// maximum (with its first index) and the sum of exponentials are reduced over the workgroup in a fixed
// tree.
#include "si_base.h"

#include <algorithm>

#include "philox.h"

namespace {

constexpr float BN_EPS = 1e-3f;
constexpr float BN_KEEP = 0.99f, BN_NEW = 0.01f;
constexpr float SCALE_A = 1.0f / 0.75f, SCALE_B = 1.0f / 0.8f;   // float32(1 / (1 - rate))

inline dim3 grid1(int64_t n, int nt) { return dim3((unsigned)((n + nt - 1) / nt)); }

// the four words of elements 4 q .. 4 q + 3 of one sample at one site
__device__ inline U4 drop_words(const SbbDrop& d, int sample, uint32_t q, uint32_t site) {
  return philox_drop_words(d.seed, d.epoch, (uint32_t)d.sid[sample], q, site);
}

__global__ void ids_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ order, int i0, int nb,
                           int n, int32_t* __restrict__ sid) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nb) return;
  const int row = order ? min(max(order[i0 + s], 0), n - 1) : i0 + s;
  sid[s] = ids ? ids[row] : row;
}

__global__ void drop_mask_kernel(SbbDrop d, int n, uint8_t* __restrict__ mask_a, uint8_t* __restrict__ mask_b) {
  constexpr int QA = SBB_MAP / 4, QB = SBB_EMB / 4;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)n * (QA + QB)) return;
  const int s = (int)(i / (QA + QB)), q = (int)(i % (QA + QB));
  const bool a = q < QA;
  const uint32_t qq = a ? q : q - QA;
  const U4 r = drop_words(d, s, qq, a ? 0u : 1u);
  const uint32_t rate = a ? SBB_RATE_A : SBB_RATE_B;
  uint8_t* out = a ? mask_a + (size_t)s * SBB_MAP + 4 * qq : mask_b + (size_t)s * SBB_EMB + 4 * qq;
#pragma unroll
  for (int k = 0; k < 4; ++k) out[k] = r.v[k] >= rate ? 1 : 0;
}

// ---- BN (batch statistics) + ReLU -----------------------------------------------------------------------
// one workgroup: 32 channels x 16 row splits of one slab

constexpr int BN_NT = 512, BN_C = 32, BN_P = BN_NT / BN_C;

__device__ inline float slab_sum(const float* __restrict__ part, int S, int c, int ch) {
  float t = 0.0f;
  for (int q = 0; q < S; ++q) t += part[(size_t)q * c + ch];
  return t;
}

// the tree over the 16 row splits of red[tid]; the result is valid in the threads with sp == 0
__device__ inline void split_tree(float (*red)[2], int tid, int sp) {
  for (int h = BN_P >> 1; h >= 1; h >>= 1) {
    __syncthreads();
    if (sp < h) {
      red[tid][0] += red[tid + h * BN_C][0];
      red[tid][1] += red[tid + h * BN_C][1];
    }
  }
}

// MODE 0: part_out[slab] = sum x.  MODE 1: mean from part_in, part_out[slab] = sum (x - mean)^2, stat = mean
template <int MODE>
__global__ void __launch_bounds__(BN_NT) bnb_part_kernel(const float* __restrict__ x, int n_pos, int c, int rows,
                                                         int S, const float* __restrict__ part_in,
                                                         float* __restrict__ part_out, float* __restrict__ stat) {
  __shared__ float red[BN_NT][2];
  __shared__ float mean_s[BN_C];
  const int tid = threadIdx.x;
  const int cl = tid % BN_C, sp = tid / BN_C;
  const int ch = blockIdx.x * BN_C + cl, slab = blockIdx.y;
  float mean = 0.0f;
  if (MODE == 1) {
    if (sp == 0) {
      mean_s[cl] = slab_sum(part_in, S, c, ch) / (float)n_pos;
      if (slab == 0) stat[ch] = mean_s[cl];
    }
    __syncthreads();
    mean = mean_s[cl];
  }
  const int p1 = min((slab + 1) * rows, n_pos);
  float acc = 0.0f;
  for (int p = slab * rows + sp; p < p1; p += BN_P) {
    const float v = x[(size_t)p * c + ch] - mean;
    acc = MODE == 1 ? fmaf(v, v, acc) : acc + v;
  }
  red[tid][0] = acc;
  red[tid][1] = 0.0f;
  split_tree(red, tid, sp);
  if (sp == 0) part_out[(size_t)slab * c + ch] = red[tid][0];
}

__global__ void __launch_bounds__(BN_NT) bnb_apply_kernel(const float* __restrict__ x, float* bn,
                                                          float* __restrict__ y, int n_pos, int c, int rows, int S,
                                                          const float* __restrict__ part_sq, float* stat) {
  __shared__ float ms[BN_C], is[BN_C];
  const int tid = threadIdx.x;
  const int cl = tid % BN_C, sp = tid / BN_C;
  const int ch = blockIdx.x * BN_C + cl, slab = blockIdx.y;
  if (sp == 0) {
    const float mean = stat[ch];
    const float var = slab_sum(part_sq, S, c, ch) / (float)n_pos;
    const float istd = 1.0f / sqrtf(var + BN_EPS);
    ms[cl] = mean;
    is[cl] = istd;
    if (slab == 0) {   // the moving statistics: nobody reads them in this launch
      stat[c + ch] = istd;
      bn[2 * c + ch] = BN_KEEP * bn[2 * c + ch] + BN_NEW * mean;
      bn[3 * c + ch] = BN_KEEP * bn[3 * c + ch] + BN_NEW * var;
    }
  }
  __syncthreads();
  const float mean = ms[cl], istd = is[cl], gamma = bn[ch], beta = bn[c + ch];
  const int p1 = min((slab + 1) * rows, n_pos);
  for (int p = slab * rows + sp; p < p1; p += BN_P) {
    const size_t at = (size_t)p * c + ch;
    y[at] = fmaxf((x[at] - mean) * istd * gamma + beta, 0.0f);
  }
}

// part[0][slab] = sum g xhat, part[1][slab] = sum g
__global__ void __launch_bounds__(BN_NT) bnb_bwd_part_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                             const float* __restrict__ dy,
                                                             const float* __restrict__ stat, int n_pos, int c,
                                                             int rows, float* __restrict__ part) {
  __shared__ float red[BN_NT][2];
  const int tid = threadIdx.x;
  const int cl = tid % BN_C, sp = tid / BN_C;
  const int ch = blockIdx.x * BN_C + cl, slab = blockIdx.y;
  const float mean = stat[ch], istd = stat[c + ch];
  const int p1 = min((slab + 1) * rows, n_pos);
  float sg = 0.0f, sb = 0.0f;
  for (int p = slab * rows + sp; p < p1; p += BN_P) {
    const size_t at = (size_t)p * c + ch;
    const float g = y[at] > 0.0f ? dy[at] : 0.0f;
    sg = fmaf(g, (x[at] - mean) * istd, sg);
    sb += g;
  }
  red[tid][0] = sg;
  red[tid][1] = sb;
  split_tree(red, tid, sp);
  if (sp == 0) {
    part[(size_t)slab * c + ch] = red[tid][0];
    part[(size_t)(SBB_SLABS + slab) * c + ch] = red[tid][1];
  }
}

__global__ void __launch_bounds__(BN_NT) bnb_bwd_dx_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                           const float* __restrict__ dy, const float* __restrict__ bn,
                                                           const float* __restrict__ stat,
                                                           const float* __restrict__ part, const float* add,
                                                           float* dx, float* __restrict__ dbn, int n_pos, int c,
                                                           int rows, int S) {
  __shared__ float mgx_s[BN_C], mg_s[BN_C];
  const int tid = threadIdx.x;
  const int cl = tid % BN_C, sp = tid / BN_C;
  const int ch = blockIdx.x * BN_C + cl, slab = blockIdx.y;
  if (sp == 0) {
    const float sgx = slab_sum(part, S, c, ch), sg = slab_sum(part + (size_t)SBB_SLABS * c, S, c, ch);
    mgx_s[cl] = sgx / (float)n_pos;
    mg_s[cl] = sg / (float)n_pos;
    if (slab == 0) {
      dbn[ch] = sgx;
      dbn[c + ch] = sg;
    }
  }
  __syncthreads();
  const float mean = stat[ch], istd = stat[c + ch], gi = bn[ch] * istd, mgx = mgx_s[cl], mg = mg_s[cl];
  const int p1 = min((slab + 1) * rows, n_pos);
  for (int p = slab * rows + sp; p < p1; p += BN_P) {
    const size_t at = (size_t)p * c + ch;
    const float g = y[at] > 0.0f ? dy[at] : 0.0f;
    const float v = gi * (g - mg - (x[at] - mean) * istd * mgx);
    dx[at] = add ? add[at] + v : v;
  }
}

// ---- Dropout(0.25) + AveragePooling1D(4) ----------------------------------------------------------------
// thread = (sample, output step, four channels): four counters, all sixteen words used

__global__ void drop_avgpool4_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int B, SbbDrop d) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;   // over [B, 8, 32]
  if (i >= B * 8 * 32) return;
  const int c4 = i % 32, tq = (i / 32) % 8, b = i / 256;
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int t = 4 * tq + j;
    const U4 r = drop_words(d, b, (uint32_t)(t * 32 + c4), 0u);
    const float4 v = *reinterpret_cast<const float4*>(x + ((size_t)b * 32 + t) * 128 + 4 * c4);
    const float xv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] += r.v[k] >= SBB_RATE_A ? xv[k] * SCALE_A : 0.0f;
  }
  float* out = y + ((size_t)b * 8 + tq) * 128 + 4 * c4;
#pragma unroll
  for (int k = 0; k < 4; ++k) out[k] = acc[k] * 0.25f;
}

__global__ void drop_avgpool4_bwd_kernel(const float* __restrict__ dxs, float* __restrict__ dx, int B, SbbDrop d) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;   // over [B, 32, 32]
  if (i >= B * 32 * 32) return;
  const int c4 = i % 32, t = (i / 32) % 32, b = i / 1024;
  const U4 r = drop_words(d, b, (uint32_t)(t * 32 + c4), 0u);
  const size_t at = ((size_t)b * 8 + t / 4) * 128 + 4 * c4;
  float* out = dx + ((size_t)b * 32 + t) * 128 + 4 * c4;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float g = (dxs[at + k] + dxs[(size_t)B * 8 * 128 + at + k]) * 0.25f;
    out[k] = r.v[k] >= SBB_RATE_A ? g * SCALE_A : 0.0f;
  }
}

// ---- Dropout(0.2) + Dense(512 -> K) + the loss on the logits --------------------------------------------

constexpr int HD_NT = 256, HD_D = SBB_EMB, HD_KMAX = 1024;

__global__ void __launch_bounds__(HD_NT) head_loss_kernel(SbbHead a, SbbDrop d) {
  __shared__ float e[HD_D];
  __shared__ float zs[HD_KMAX];
  __shared__ float rf[HD_NT];
  __shared__ int ri[HD_NT];
  const int tid = threadIdx.x, s = blockIdx.x, K = a.K;
  if (tid < HD_D / 4) {
    U4 r{{~0u, ~0u, ~0u, ~0u}};
    if (a.drop) r = drop_words(d, s, (uint32_t)tid, 1u);
    const float keep = a.drop ? SCALE_B : 1.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const size_t at = (size_t)s * HD_D + 4 * tid + k;
      const float m = r.v[k] >= SBB_RATE_B ? keep : 0.0f;
      const float v = a.emb[at] * m;
      e[4 * tid + k] = v;
      a.embd[at] = v;
      a.dmul[at] = m;
    }
  }
  __syncthreads();
  float best = -INFINITY;
  int arg = 0x7fffffff;
  for (int k = tid; k < K; k += HD_NT) {
    float z = a.b[k];
    for (int q = 0; q < HD_D; ++q) z = fmaf(e[q], a.w[(size_t)q * K + k], z);
    zs[k] = z;
    if (z > best) {   // ascending k: the first maximum stays
      best = z;
      arg = k;
    }
  }
  rf[tid] = best;
  ri[tid] = arg;
  for (int h = HD_NT >> 1; h >= 1; h >>= 1) {
    __syncthreads();
    if (tid < h) {
      const float ob = rf[tid + h];
      const int oa = ri[tid + h];
      if (ob > rf[tid] || (ob == rf[tid] && oa < ri[tid])) {
        rf[tid] = ob;
        ri[tid] = oa;
      }
    }
  }
  __syncthreads();
  const float zmax = rf[0];
  const int first = ri[0];
  __syncthreads();
  float part = 0.0f;
  for (int k = tid; k < K; k += HD_NT) part += expf(zs[k] - zmax);
  rf[tid] = part;
  for (int h = HD_NT >> 1; h >= 1; h >>= 1) {
    __syncthreads();
    if (tid < h) rf[tid] += rf[tid + h];
  }
  __syncthreads();
  const float S = rf[0];
  const int lab = min(max(a.labels[s], 0), K - 1);
  if (a.dz)
    for (int k = tid; k < K; k += HD_NT)
      a.dz[(size_t)s * K + k] = (expf(zs[k] - zmax) / S - (k == lab ? 1.0f : 0.0f)) / a.bsz;
  if (tid == 0) {
    a.loss[s] = (float)(log((double)S) + ((double)zmax - (double)zs[lab]));
    a.hit[s] = first == lab ? 1 : 0;
  }
}

// acc[0] += sum of loss[0..B), acc[1] += hits: 256 strided partials in float64, then a fixed tree
__global__ void __launch_bounds__(HD_NT) head_acc_kernel(const float* __restrict__ loss,
                                                         const int32_t* __restrict__ hit, int B, double* acc) {
  __shared__ double rl[HD_NT];
  __shared__ int rh[HD_NT];
  const int tid = threadIdx.x;
  double l = 0.0;
  int hs = 0;
  for (int s = tid; s < B; s += HD_NT) {
    l += (double)loss[s];
    hs += hit[s];
  }
  rl[tid] = l;
  rh[tid] = hs;
  for (int h = HD_NT >> 1; h >= 1; h >>= 1) {
    __syncthreads();
    if (tid < h) {
      rl[tid] += rl[tid + h];
      rh[tid] += rh[tid + h];
    }
  }
  if (tid == 0) {
    acc[0] += rl[0];
    acc[1] += (double)rh[0];
  }
}

__global__ void head_bwd_kernel(SbbHead a, float* __restrict__ gw, float* __restrict__ gb,
                                float* __restrict__ demb) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int K = a.K;
  const int64_t nw = (int64_t)HD_D * K;
  if (i < nw) {
    const int q = (int)(i / K), k = (int)(i % K);
    float acc = 0.0f;
    for (int b = 0; b < a.B; ++b) acc = fmaf(a.embd[(size_t)b * HD_D + q], a.dz[(size_t)b * K + k], acc);
    gw[i] = acc;
  } else if (i < nw + K) {
    const int k = (int)(i - nw);
    float acc = 0.0f;
    for (int b = 0; b < a.B; ++b) acc += a.dz[(size_t)b * K + k];
    gb[k] = acc;
  } else if (i < nw + K + (int64_t)a.B * HD_D) {
    const int64_t q = i - nw - K;
    const int b = (int)(q / HD_D), dd = (int)(q % HD_D);
    float acc = 0.0f;
    for (int k = 0; k < K; ++k) acc = fmaf(a.dz[(size_t)b * K + k], a.w[(size_t)dd * K + k], acc);
    demb[q] = acc * a.dmul[q];
  }
}

// slabs of a reduction over n_pos rows, and the rows of each
inline int bn_slabs(int n_pos) { return std::min(SBB_SLABS, (n_pos + 63) / 64); }

}  // namespace

#define SBB_LAUNCH(kernel, grid, block, ...)                            \
  do {                                                                  \
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, __VA_ARGS__);    \
    const hipError_t err_ = hipGetLastError();                          \
    if (err_ != hipSuccess) return err_;                                \
  } while (0)

hipError_t sbb_ids(const int32_t* ids, const int32_t* order, int i0, int nb, int n, int32_t* sid,
                   hipStream_t stream) {
  SBB_LAUNCH(ids_kernel, grid1(nb, 256), dim3(256), ids, order, i0, nb, n, sid);
  return hipSuccess;
}

hipError_t sbb_drop_mask(const SbbDrop& d, int n, uint8_t* mask_a, uint8_t* mask_b, hipStream_t stream) {
  SBB_LAUNCH(drop_mask_kernel, grid1((int64_t)n * (SBB_MAP + SBB_EMB) / 4, 256), dim3(256), d, n, mask_a, mask_b);
  return hipSuccess;
}

hipError_t sbb_bn_relu_fwd(const float* x, float* bn, float* y, int n_pos, int c, float* stat, float* part,
                           hipStream_t stream) {
  if (c < BN_C || c > SBB_MAX_C || c % BN_C || n_pos < 1) return hipErrorInvalidValue;
  const int S = bn_slabs(n_pos), rows = (n_pos + S - 1) / S;
  const dim3 grid(c / BN_C, S);
  float* part_sq = part + (size_t)SBB_SLABS * SBB_MAX_C;
  SBB_LAUNCH(bnb_part_kernel<0>, grid, dim3(BN_NT), x, n_pos, c, rows, S, (const float*)nullptr, part, stat);
  SBB_LAUNCH(bnb_part_kernel<1>, grid, dim3(BN_NT), x, n_pos, c, rows, S, (const float*)part, part_sq, stat);
  SBB_LAUNCH(bnb_apply_kernel, grid, dim3(BN_NT), x, bn, y, n_pos, c, rows, S, (const float*)part_sq, stat);
  return hipSuccess;
}

hipError_t sbb_bn_relu_bwd(const float* x, const float* y, const float* dy, const float* bn,
                           const float* stat, float* part, const float* add, float* dx, float* dbn, int n_pos,
                           int c, hipStream_t stream) {
  if (c < BN_C || c > SBB_MAX_C || c % BN_C || n_pos < 1) return hipErrorInvalidValue;
  const int S = bn_slabs(n_pos), rows = (n_pos + S - 1) / S;
  const dim3 grid(c / BN_C, S);
  SBB_LAUNCH(bnb_bwd_part_kernel, grid, dim3(BN_NT), x, y, dy, stat, n_pos, c, rows, part);
  SBB_LAUNCH(bnb_bwd_dx_kernel, grid, dim3(BN_NT), x, y, dy, bn, stat, (const float*)part, add, dx, dbn, n_pos, c,
             rows, S);
  return hipSuccess;
}

hipError_t sbb_drop_avgpool4_fwd(const float* x, float* y, int B, const SbbDrop& d, hipStream_t stream) {
  SBB_LAUNCH(drop_avgpool4_fwd_kernel, grid1((int64_t)B * 8 * 32, 256), dim3(256), x, y, B, d);
  return hipSuccess;
}

hipError_t sbb_drop_avgpool4_bwd(const float* dxs, float* dx, int B, const SbbDrop& d, hipStream_t stream) {
  SBB_LAUNCH(drop_avgpool4_bwd_kernel, grid1((int64_t)B * 32 * 32, 256), dim3(256), dxs, dx, B, d);
  return hipSuccess;
}

hipError_t sbb_head_loss(const SbbHead& a, const SbbDrop& d, hipStream_t stream) {
  if (a.K < 1 || a.K > HD_KMAX || a.B < 1) return hipErrorInvalidValue;
  SBB_LAUNCH(head_loss_kernel, dim3(a.B), dim3(HD_NT), a, d);
  SBB_LAUNCH(head_acc_kernel, dim3(1), dim3(HD_NT), (const float*)a.loss, (const int32_t*)a.hit, a.B, a.acc);
  return hipSuccess;
}

hipError_t sbb_head_bwd(const SbbHead& a, float* gw, float* gb, float* demb, hipStream_t stream) {
  SBB_LAUNCH(head_bwd_kernel, grid1((int64_t)HD_D * a.K + a.K + (int64_t)a.B * HD_D, 256), dim3(256), a, gw, gb,
             demb);
  return hipSuccess;
}
