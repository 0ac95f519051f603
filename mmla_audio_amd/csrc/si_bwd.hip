// Speaker registration, stage 2 of transfer_learning (speaker_identification.py:438-454): the whole
// SI network trainable under RMSprop(1e-6), batch 8.  This file is the float32 training forward (it
// keeps what the backward needs) and the backward of every layer kind of SI-NET.
//
// Plain FMA, no MFMA: at batch 8 a step is ~1.1 GFLOP spread over ~170 launches, the largest of them
// 25 MFLOP; what a step costs is launch rate and the latency of short dependent loops, not arithmetic
// rate, and float32 FMA keeps every sum's order explicit.
//
// Determinism: no floating-point atomics anywhere.  A sum over the B * T positions of a layer (conv
// weight and bias gradients, BN gamma / beta gradients; the LSTM's 384-input gate sums) is split over P threads that each walk their
// positions in ascending order, and the P partials are added in LDS in a fixed binary tree; wave-level
// sums (the LSTM's transposed products) use the xor butterfly, whose order is fixed too.  Every other
// output is one thread's serial loop.  The same inputs give the same bits on every run.
//
// Layouts: activations channels-last [B, T, C] (the network's input [B, 256, 39] is already that);
// parameters and gradients in the packed blob's Keras layouts.  A lane indexes the fastest dimension
// (cout, cin or the LSTM column), so weight and gradient accesses are coalesced and the activation
// operand is a wave-wide broadcast.  The data gradient of a conv reads a [k, cout, cin] transpose of
// its kernel (sib_conv_transpose) for the same reason.
#include "si_bwd.h"

namespace {

constexpr float BN_EPS = 1e-3f;

__device__ inline float sigmoidf_(float z) { return 1.0f / (1.0f + expf(-z)); }

inline dim3 grid1(int64_t n, int nt) { return dim3((unsigned)((n + nt - 1) / nt)); }

// ---- gather -------------------------------------------------------------------------------------------

__global__ void gather_kernel(const float* __restrict__ x, const int32_t* __restrict__ labels,
                              const int32_t* __restrict__ order, int i0, int nb, int n, int row_floats,
                              float* __restrict__ xb, int32_t* __restrict__ lb) {
  const int s = blockIdx.y;
  if (s >= nb) return;
  const int row = order ? min(max(order[i0 + s], 0), n - 1) : i0 + s;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < row_floats) xb[(size_t)s * row_floats + i] = x[(size_t)row * row_floats + i];
  if (i == 0) lb[s] = labels[row];
}

// ---- Conv1D -------------------------------------------------------------------------------------------

__global__ void conv_fwd_kernel(SibConv g, const float* __restrict__ x, const float* __restrict__ w,
                                const float* __restrict__ bias, const float* res, float* y) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)g.B * g.tout * g.cout) return;
  const int co = (int)(i % g.cout);
  const int64_t p = i / g.cout;
  const int t = (int)(p % g.tout), b = (int)(p / g.tout);
  float acc = bias[co];
  for (int j = 0; j < g.k; ++j) {
    const int ti = t * g.stride + j - g.pad_l;
    if (ti < 0 || ti >= g.tin) continue;
    const float* __restrict__ xr = x + ((size_t)b * g.tin + ti) * g.cin;
    const float* __restrict__ wr = w + (size_t)j * g.cin * g.cout + co;
#pragma unroll 4
    for (int ci = 0; ci < g.cin; ++ci) acc = fmaf(xr[ci], wr[(size_t)ci * g.cout], acc);
  }
  if (res) acc += res[i];
  y[i] = acc;
}

__global__ void conv_transpose_kernel(SibConv g, const float* __restrict__ w, float* __restrict__ wt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= g.k * g.cin * g.cout) return;
  const int ci = i % g.cin, co = (i / g.cin) % g.cout, j = i / (g.cin * g.cout);
  wt[i] = w[((size_t)j * g.cin + ci) * g.cout + co];
}

__global__ void conv_bwd_data_kernel(SibConv g, const float* __restrict__ dy, const float* __restrict__ wt,
                                     const float* add, float* dx) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)g.B * g.tin * g.cin) return;
  const int ci = (int)(i % g.cin);
  const int64_t p = i / g.cin;
  const int ti = (int)(p % g.tin), b = (int)(p / g.tin);
  float acc = add ? add[i] : 0.0f;
  for (int j = 0; j < g.k; ++j) {
    const int num = ti + g.pad_l - j;
    if (num < 0 || num % g.stride != 0) continue;
    const int to = num / g.stride;
    if (to >= g.tout) continue;
    const float* __restrict__ dr = dy + ((size_t)b * g.tout + to) * g.cout;
    const float* __restrict__ wr = wt + (size_t)j * g.cout * g.cin + ci;
#pragma unroll 4
    for (int co = 0; co < g.cout; ++co) acc = fmaf(dr[co], wr[(size_t)co * g.cin], acc);
  }
  dx[i] = acc;
}

// one workgroup: tap j = blockIdx.y, input channels [4 blockIdx.x, +4), every output channel;
// thread = (co, split), split sp walks positions sp, sp + P, ... (P = 1024 / cout: the walk is a chain
// of dependent loads, so it is kept short); the P partials meet in an LDS tree
constexpr int WG_NT = 1024, WG_CT = 4;

__global__ void __launch_bounds__(WG_NT) conv_bwd_weight_kernel(
    SibConv g, const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ w,
    float l2x2, float* __restrict__ dw, float* __restrict__ db) {
  __shared__ float red[WG_NT][WG_CT + 1];
  const int tid = threadIdx.x;
  const int co = tid % g.cout, sp = tid / g.cout, P = WG_NT / g.cout;
  const int j = blockIdx.y, ci0 = blockIdx.x * WG_CT;
  const int nq = min(WG_CT, g.cin - ci0);
  float acc[WG_CT] = {0.0f, 0.0f, 0.0f, 0.0f};
  float accb = 0.0f;
  const int n_pos = g.B * g.tout;
#pragma unroll 4
  for (int p = sp; p < n_pos; p += P) {
    const int b = p / g.tout, t = p % g.tout;
    const float dv = dy[(size_t)p * g.cout + co];
    accb += dv;
    const int ti = t * g.stride + j - g.pad_l;
    const bool in = ti >= 0 && ti < g.tin;   // the padding contributes 0 (row 0 is read in its place)
    const float dvx = in ? dv : 0.0f;
    const float* __restrict__ xr = x + ((size_t)b * g.tin + (in ? ti : 0)) * g.cin + ci0;
#pragma unroll
    for (int q = 0; q < WG_CT; ++q)
      if (q < nq) acc[q] = fmaf(xr[q], dvx, acc[q]);
  }
#pragma unroll
  for (int q = 0; q < WG_CT; ++q) red[tid][q] = acc[q];
  red[tid][WG_CT] = accb;
  for (int h = P >> 1; h >= 1; h >>= 1) {
    __syncthreads();
    if (sp < h) {
#pragma unroll
      for (int q = 0; q <= WG_CT; ++q) red[tid][q] += red[tid + h * g.cout][q];
    }
  }
  if (sp == 0) {
    for (int q = 0; q < nq; ++q) {
      const size_t at = ((size_t)j * g.cin + ci0 + q) * g.cout + co;
      dw[at] = fmaf(l2x2, w[at], red[tid][q]);
    }
    if (blockIdx.x == 0 && blockIdx.y == 0) db[co] = red[tid][WG_CT];
  }
}

// ---- BN (moving statistics) + ReLU ---------------------------------------------------------------------

__global__ void bn_relu_fwd_kernel(const float* __restrict__ x, const float* __restrict__ bn,
                                   float* __restrict__ y, int64_t n, int c) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int ch = (int)(i % c);
  const float inv = 1.0f / sqrtf(bn[3 * c + ch] + BN_EPS);
  const float v = (x[i] - bn[2 * c + ch]) * inv * bn[ch] + bn[c + ch];
  y[i] = fmaxf(v, 0.0f);
}

// one workgroup: 32 channels x 16 position splits
constexpr int BN_NT = 512, BN_C = 32, BN_P = BN_NT / BN_C;

__global__ void __launch_bounds__(BN_NT) bn_relu_bwd_kernel(
    const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ dy,
    const float* __restrict__ bn, const float* add, float* dx, float* __restrict__ dbn, int n_pos, int c) {
  __shared__ float red[BN_NT][2];
  const int tid = threadIdx.x;
  const int cl = tid % BN_C, sp = tid / BN_C;
  const int ch = blockIdx.x * BN_C + cl;   // c is a multiple of 32 (the launcher checks)
  const float inv = 1.0f / sqrtf(bn[3 * c + ch] + BN_EPS);
  const float mean = bn[2 * c + ch], gi = bn[ch] * inv;
  float sg = 0.0f, sb = 0.0f;
  for (int p = sp; p < n_pos; p += BN_P) {
    const size_t at = (size_t)p * c + ch;
    const float d = y[at] > 0.0f ? dy[at] : 0.0f;
    sg = fmaf(d, (x[at] - mean) * inv, sg);
    sb += d;
    dx[at] = add ? fmaf(d, gi, add[at]) : d * gi;
  }
  red[tid][0] = sg;
  red[tid][1] = sb;
  for (int h = BN_P >> 1; h >= 1; h >>= 1) {
    __syncthreads();
    if (sp < h) {
      red[tid][0] += red[tid + h * BN_C][0];
      red[tid][1] += red[tid + h * BN_C][1];
    }
  }
  if (sp == 0) {
    dbn[ch] = red[tid][0];
    dbn[c + ch] = red[tid][1];
  }
}

// ---- pools --------------------------------------------------------------------------------------------

__global__ void maxpool_fwd_kernel(const float* __restrict__ x, float* __restrict__ y,
                                   uint8_t* __restrict__ idx, int64_t n, int c) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // over [B * th, c]
  if (i >= n) return;
  const int64_t p = i / c;
  const int ch = (int)(i % c);
  const float a = x[(2 * p) * c + ch], b = x[(2 * p + 1) * c + ch];
  const bool second = b > a;
  y[i] = second ? b : a;
  idx[i] = second ? 1 : 0;
}

__global__ void maxpool_bwd_kernel(const float* __restrict__ dy, const uint8_t* __restrict__ idx,
                                   float* __restrict__ dx, int64_t n, int c) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t p = i / c;
  const int ch = (int)(i % c);
  const float d = dy[i];
  const bool second = idx[i] != 0;
  dx[(2 * p) * c + ch] = second ? 0.0f : d;
  dx[(2 * p + 1) * c + ch] = second ? d : 0.0f;
}

__global__ void avgpool4_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n, int c) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // over [B * tq, c]
  if (i >= n) return;
  const int64_t p = i / c;
  const int ch = (int)(i % c);
  const float* xr = x + (4 * p) * c + ch;
  y[i] = (xr[0] + xr[c] + xr[2 * c] + xr[3 * c]) * 0.25f;
}

__global__ void avgpool4_bwd_kernel(const float* __restrict__ dxs, float* __restrict__ dx, int B) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // over [B, 32, 128]
  const int64_t n = (int64_t)B * 32 * SIB_LSTM_D;
  if (i >= n) return;
  const int ch = (int)(i % SIB_LSTM_D);
  const int64_t p = i / SIB_LSTM_D;
  const int t = (int)(p % 32), b = (int)(p / 32);
  const size_t at = ((size_t)b * SIB_LSTM_T + t / 4) * SIB_LSTM_D + ch;
  dx[i] = (dxs[at] + dxs[(size_t)B * SIB_LSTM_T * SIB_LSTM_D + at]) * 0.25f;
}

// ---- BiLSTM -------------------------------------------------------------------------------------------
// Buffers are indexed by processing step s of a.T: the forward direction reads x[s], the backward one
// x[T - 1 - s].

constexpr int LS_NB = 8;    // samples per workgroup
constexpr int LS_IN = SIB_LSTM_D + SIB_LSTM_U;

__device__ inline int step_time(int dir, int s, int T) { return dir ? T - 1 - s : s; }

// workgroup = 64 units of one direction x 4 splits of the 384 inputs; thread (u, q) sums its 96 inputs
// into the four gate columns of unit u for up to 8 samples, the 4 partials are added in LDS in order
// 0..3 by the q = 0 threads, which then run the cell
constexpr int LS_NT = 256, LS_Q = 4, LS_UB = LS_NT / LS_Q, LS_DQ = LS_IN / LS_Q;

__global__ void __launch_bounds__(LS_NT) lstm_fwd_step_kernel(SibLstm a, int s) {
  __shared__ float xin[LS_NB][LS_IN];
  __shared__ float part[LS_Q - 1][4 * LS_NB][LS_UB];
  const int dir = blockIdx.y, b0 = blockIdx.z * LS_NB;
  const int nb = min(LS_NB, a.B - b0);
  const int ul = threadIdx.x % LS_UB, q4 = threadIdx.x / LS_UB;
  const int u = blockIdx.x * LS_UB + ul;
  const int t = step_time(dir, s, a.T);
  const size_t BU = (size_t)a.B * SIB_LSTM_U;
  for (int i = threadIdx.x; i < LS_NB * LS_IN; i += LS_NT) {
    const int b = i / LS_IN, d = i % LS_IN;
    float v = 0.0f;
    if (b < nb) {
      if (d < SIB_LSTM_D)
        v = a.seq[((size_t)(b0 + b) * a.T + t) * SIB_LSTM_D + d];
      else if (s > 0)
        v = a.hs[((size_t)dir * a.T + s - 1) * BU + (size_t)(b0 + b) * SIB_LSTM_U + d - SIB_LSTM_D];
    }
    xin[b][d] = v;
  }
  __syncthreads();
  float acc[4][LS_NB];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float bv = q4 == 0 ? a.bias[dir][q * SIB_LSTM_U + u] : 0.0f;
#pragma unroll
    for (int b = 0; b < LS_NB; ++b) acc[q][b] = bv;
  }
#pragma unroll 4
  for (int d = q4 * LS_DQ; d < (q4 + 1) * LS_DQ; ++d) {
    const float* __restrict__ wrow = d < SIB_LSTM_D ? a.wk[dir] + (size_t)d * SIB_LSTM_G
                                                    : a.wr[dir] + (size_t)(d - SIB_LSTM_D) * SIB_LSTM_G;
    float wv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) wv[q] = wrow[q * SIB_LSTM_U + u];
#pragma unroll
    for (int b = 0; b < LS_NB; ++b) {
      const float xv = xin[b][d];
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q][b] = fmaf(xv, wv[q], acc[q][b]);
    }
  }
  if (q4 > 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int b = 0; b < LS_NB; ++b) part[q4 - 1][q * LS_NB + b][ul] = acc[q][b];
  }
  __syncthreads();
  if (q4 > 0) return;
#pragma unroll
  for (int r = 0; r < LS_Q - 1; ++r)
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int b = 0; b < LS_NB; ++b) acc[q][b] += part[r][q * LS_NB + b][ul];
#pragma unroll
  for (int b = 0; b < LS_NB; ++b) {
    if (b < nb) {
      const size_t row = ((size_t)dir * a.T + s) * a.B + b0 + b;
      const float gi = sigmoidf_(acc[0][b]), gf = sigmoidf_(acc[1][b]);
      const float gg = tanhf(acc[2][b]), go = sigmoidf_(acc[3][b]);
      const float cp = s > 0 ? a.cs[(row - a.B) * SIB_LSTM_U + u] : 0.0f;
      const float cv = fmaf(gf, cp, gi * gg);
      const float hv = go * tanhf(cv);
      float* gr = a.gates + row * SIB_LSTM_G + u;
      gr[0] = gi;
      gr[SIB_LSTM_U] = gf;
      gr[2 * SIB_LSTM_U] = gg;
      gr[3 * SIB_LSTM_U] = go;
      a.cs[row * SIB_LSTM_U + u] = cv;
      a.hs[row * SIB_LSTM_U + u] = hv;
      if (s == a.T - 1) a.emb[(size_t)(b0 + b) * 2 * SIB_LSTM_U + dir * SIB_LSTM_U + u] = hv;
    }
  }
}

// thread = (dir, b, u): the gates' pre-activation gradients of step s from dh, dc; dc carried on
__global__ void lstm_bwd_gates_kernel(SibLstm a, int s) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int n = 2 * a.B * SIB_LSTM_U;
  if (i >= n) return;
  const int u = i % SIB_LSTM_U, b = (i / SIB_LSTM_U) % a.B, dir = i / (SIB_LSTM_U * a.B);
  const bool last = s == a.T - 1;
  const float dh = last ? a.demb[(size_t)b * 2 * SIB_LSTM_U + dir * SIB_LSTM_U + u] : a.dh[i];
  float dc = last ? 0.0f : a.dc[i];
  const size_t row = ((size_t)dir * a.T + s) * a.B + b;
  const float* gr = a.gates + row * SIB_LSTM_G + u;
  const float gi = gr[0], gf = gr[SIB_LSTM_U], gg = gr[2 * SIB_LSTM_U], go = gr[3 * SIB_LSTM_U];
  const float tc = tanhf(a.cs[row * SIB_LSTM_U + u]);
  const float cp = s > 0 ? a.cs[(row - a.B) * SIB_LSTM_U + u] : 0.0f;
  dc = fmaf(dh * go, 1.0f - tc * tc, dc);
  float* zr = a.dz + row * SIB_LSTM_G + u;
  zr[0] = dc * gg * gi * (1.0f - gi);
  zr[SIB_LSTM_U] = dc * cp * gf * (1.0f - gf);
  zr[2 * SIB_LSTM_U] = dc * gi * (1.0f - gg * gg);
  zr[3 * SIB_LSTM_U] = dh * tc * go * (1.0f - go);
  a.dc[i] = dc * gf;
}

// wave = one row of [kernel; recurrent_kernel] (row < 128: dx of the step's input, else dh of the step
// before): the 1024-column dot product with dz for up to 8 samples, lanes over columns
__global__ void __launch_bounds__(256) lstm_bwd_mm_kernel(SibLstm a, int s, int n_rows) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n_rows) return;   // whole waves leave together
  const int dir = blockIdx.y, b0 = blockIdx.z * LS_NB;
  const int nb = min(LS_NB, a.B - b0);
  const float* __restrict__ wrow = r < SIB_LSTM_D ? a.wk[dir] + (size_t)r * SIB_LSTM_G
                                                  : a.wr[dir] + (size_t)(r - SIB_LSTM_D) * SIB_LSTM_G;
  const float* __restrict__ dz = a.dz + (((size_t)dir * a.T + s) * a.B + b0) * SIB_LSTM_G;
  float acc[LS_NB];
#pragma unroll
  for (int b = 0; b < LS_NB; ++b) acc[b] = 0.0f;
  for (int it = 0; it < SIB_LSTM_G / 64; ++it) {
    const int j = it * 64 + lane;
    const float wv = wrow[j];
#pragma unroll
    for (int b = 0; b < LS_NB; ++b)
      if (b < nb) acc[b] = fmaf(wv, dz[(size_t)b * SIB_LSTM_G + j], acc[b]);
  }
#pragma unroll
  for (int b = 0; b < LS_NB; ++b)
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc[b] += __shfl_xor(acc[b], m, 64);
  if (lane == 0) {
    const int t = step_time(dir, s, a.T);
    for (int b = 0; b < nb; ++b) {
      if (r < SIB_LSTM_D)
        a.dxs[(((size_t)dir * a.B + b0 + b) * a.T + t) * SIB_LSTM_D + r] = acc[b];
      else
        a.dh[((size_t)dir * a.B + b0 + b) * SIB_LSTM_U + r - SIB_LSTM_D] = acc[b];
    }
  }
}

// thread = one entry of [kernel; recurrent_kernel; bias] of one direction: the sum over steps, samples
__global__ void __launch_bounds__(256) lstm_bwd_w_kernel(SibLstm a) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  const int r = blockIdx.y, dir = blockIdx.z;
  float acc = 0.0f;
  for (int s = 0; s < a.T; ++s) {
    if (r >= SIB_LSTM_D && r < LS_IN && s == 0) continue;   // h before the first step is 0
    const int t = step_time(dir, s, a.T);
    for (int b = 0; b < a.B; ++b) {
      const size_t row = ((size_t)dir * a.T + s) * a.B + b;
      float in = 1.0f;
      if (r < SIB_LSTM_D)
        in = a.seq[((size_t)b * a.T + t) * SIB_LSTM_D + r];
      else if (r < LS_IN)
        in = a.hs[(row - a.B) * SIB_LSTM_U + r - SIB_LSTM_D];
      acc = fmaf(in, a.dz[row * SIB_LSTM_G + j], acc);
    }
  }
  if (r < SIB_LSTM_D)
    a.dwk[dir][(size_t)r * SIB_LSTM_G + j] = acc;
  else if (r < LS_IN)
    a.dwr[dir][(size_t)(r - SIB_LSTM_D) * SIB_LSTM_G + j] = acc;
  else
    a.dbias[dir][j] = acc;
}

// ---- Dense + sigmoid + categorical_crossentropy ---------------------------------------------------------
// The statement of si_train.hip: p = s_c / sum_k s_k, -log(clip(p, 1e-7, 1 - 1e-7)); the gradient at the
// logits is zero for a sample whose p is outside the clip range.  One workgroup; thread = (sample of
// a chunk of 32, class), the 32 lanes of a sample are half a wave.

constexpr int HD_NT = 1024, HD_K = 32, HD_D = 512;

__global__ void __launch_bounds__(HD_NT) head_loss_kernel(SibHead a) {
  __shared__ float loss[HD_NT / HD_K];
  __shared__ int hit[HD_NT / HD_K];
  const int k = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int K = a.K;
  const float lo = 1e-7f, hi = 1.0f - 1e-7f;
  double lsum = 0.0;
  int hits = 0;
  for (int s0 = 0; s0 < a.B; s0 += HD_NT / HD_K) {
    const int s = s0 + sl;
    const bool live = s < a.B && k < K;
    float z = 0.0f;
    if (live) {
      z = a.b[k];
      const float* __restrict__ e = a.emb + (size_t)s * HD_D;
      for (int d = 0; d < HD_D; ++d) z = fmaf(e[d], a.w[(size_t)d * K + k], z);
    }
    const float sig = sigmoidf_(z);
    float S = k < K ? sig : 0.0f;
    float best = k < K ? sig : -1.0f;
    int arg = k;
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) {
      S += __shfl_xor(S, m, 32);
      const float ob = __shfl_xor(best, m, 32);
      const int oa = __shfl_xor(arg, m, 32);
      if (ob > best || (ob == best && oa < arg)) {
        best = ob;
        arg = oa;
      }
    }
    int c = 0;
    if (s < a.B) c = a.labels[s] & (HD_K - 1);   // a lane index for the shuffle below
    const float sc = __shfl(sig, c, 32);
    const float p = sc / S;
    const bool inside = p >= lo && p <= hi;
    if (a.dz && live)
      a.dz[(size_t)s * K + k] =
          inside ? sig * (1.0f - sig) * (1.0f / S - (k == c ? 1.0f / sc : 0.0f)) / a.bsz : 0.0f;
    if (k == 0) {
      loss[sl] = s < a.B ? (float)(-log((double)fminf(fmaxf(p, lo), hi))) : 0.0f;
      hit[sl] = s < a.B && arg == c ? 1 : 0;
    }
    __syncthreads();
    if (threadIdx.x == 0)
      for (int q = 0; q < HD_NT / HD_K; ++q) {
        lsum += (double)loss[q];
        hits += hit[q];
      }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    a.acc[0] += lsum;
    a.acc[1] += (double)hits;
  }
}

__global__ void head_bwd_kernel(SibHead a, float* __restrict__ gw, float* __restrict__ gb,
                                float* __restrict__ demb) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int K = a.K, nw = HD_D * K;
  if (i < nw) {
    const int d = i / K, k = i % K;
    float acc = 0.0f;
    for (int b = 0; b < a.B; ++b) acc = fmaf(a.emb[(size_t)b * HD_D + d], a.dz[(size_t)b * K + k], acc);
    gw[i] = acc;
  } else if (i < nw + K) {
    const int k = i - nw;
    float acc = 0.0f;
    for (int b = 0; b < a.B; ++b) acc += a.dz[(size_t)b * K + k];
    gb[k] = acc;
  } else if (i < nw + K + a.B * HD_D) {
    const int q = i - nw - K;
    const int b = q / HD_D, d = q % HD_D;
    float acc = 0.0f;
    for (int k = 0; k < K; ++k) acc = fmaf(a.dz[(size_t)b * K + k], a.w[(size_t)d * K + k], acc);
    demb[q] = acc;
  }
}

// ---- L2 penalty, RMSprop, bookkeeping -------------------------------------------------------------------

constexpr int L2_NT = 1024;

__global__ void __launch_bounds__(L2_NT) l2_kernel(SibL2 a, double* __restrict__ r) {
  __shared__ double red[L2_NT];
  double tot = 0.0;
  for (int q = 0; q < a.n_t; ++q) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < a.n[q]; i += L2_NT) {
      const double v = (double)a.w[q][i];
      acc = fma(v, v, acc);
    }
    tot = fma((double)a.lambda[q], acc, tot);
  }
  red[threadIdx.x] = tot;
  for (int h = L2_NT >> 1; h >= 1; h >>= 1) {
    __syncthreads();
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
  }
  if (threadIdx.x == 0) r[0] = red[0];
}

__global__ void rmsprop_kernel(float* __restrict__ w, float* __restrict__ rms, const float* __restrict__ g,
                               const uint8_t* __restrict__ trainable, int64_t n, float lr) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !trainable[i]) return;
  const float gv = g[i];
  const float rv = 0.9f * rms[i] + 0.1f * (gv * gv);
  rms[i] = rv;
  w[i] -= (lr * gv) / (sqrtf(rv) + 1e-7f);
}

__global__ void fold_batch_kernel(double* st, int nb) {
  st[3] += st[0] + st[2] * (double)nb;
  st[4] += st[1];
  st[0] = 0.0;
  st[1] = 0.0;
}

__global__ void end_epoch_kernel(double* st, int n_train, int n_val, float* row) {
  row[0] = (float)(st[3] / n_train);
  row[1] = (float)(st[4] / n_train);
  row[2] = n_val > 0 ? (float)(st[5] / n_val + st[2]) : __builtin_nanf("");
  row[3] = n_val > 0 ? (float)(st[6] / n_val) : __builtin_nanf("");
  for (int i = 0; i < SIB_ST; ++i) st[i] = 0.0;
}

__global__ void loss_pair_kernel(const double* st, int n, float* loss) {
  loss[0] = (float)(st[0] / n);
  loss[1] = (float)st[2];
}

}  // namespace

#define SIB_LAUNCH(kernel, grid, block, ...)                            \
  do {                                                                  \
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, __VA_ARGS__);    \
    return hipGetLastError();                                           \
  } while (0)

hipError_t sib_gather(const float* x, const int32_t* labels, const int32_t* order, int i0, int nb, int n,
                      int row_floats, float* xb, int32_t* lb, hipStream_t stream) {
  SIB_LAUNCH(gather_kernel, dim3((row_floats + 255) / 256, nb), dim3(256), x, labels, order, i0, nb, n,
             row_floats, xb, lb);
}

hipError_t sib_conv_fwd(const SibConv& g, const float* x, const float* w, const float* bias,
                        const float* res, float* y, hipStream_t stream) {
  SIB_LAUNCH(conv_fwd_kernel, grid1((int64_t)g.B * g.tout * g.cout, 256), dim3(256), g, x, w, bias, res, y);
}

hipError_t sib_conv_transpose(const SibConv& g, const float* w, float* wt, hipStream_t stream) {
  SIB_LAUNCH(conv_transpose_kernel, grid1((int64_t)g.k * g.cin * g.cout, 256), dim3(256), g, w, wt);
}

hipError_t sib_conv_bwd_data(const SibConv& g, const float* dy, const float* wt, const float* add,
                             float* dx, hipStream_t stream) {
  SIB_LAUNCH(conv_bwd_data_kernel, grid1((int64_t)g.B * g.tin * g.cin, 256), dim3(256), g, dy, wt, add, dx);
}

hipError_t sib_conv_bwd_weight(const SibConv& g, const float* x, const float* dy, const float* w,
                               float l2x2, float* dw, float* db, hipStream_t stream) {
  if (g.cout < 1 || g.cout > WG_NT || WG_NT % g.cout != 0 || ((WG_NT / g.cout) & (WG_NT / g.cout - 1)))
    return hipErrorInvalidValue;
  SIB_LAUNCH(conv_bwd_weight_kernel, dim3((g.cin + WG_CT - 1) / WG_CT, g.k), dim3(WG_NT), g, x, dy, w,
             l2x2, dw, db);
}

hipError_t sib_bn_relu_fwd(const float* x, const float* bn, float* y, int n_pos, int c,
                           hipStream_t stream) {
  SIB_LAUNCH(bn_relu_fwd_kernel, grid1((int64_t)n_pos * c, 256), dim3(256), x, bn, y, (int64_t)n_pos * c, c);
}

hipError_t sib_bn_relu_bwd(const float* x, const float* y, const float* dy, const float* bn,
                           const float* add, float* dx, float* dbn, int n_pos, int c,
                           hipStream_t stream) {
  if (c % BN_C) return hipErrorInvalidValue;
  SIB_LAUNCH(bn_relu_bwd_kernel, dim3(c / BN_C), dim3(BN_NT), x, y, dy, bn, add, dx, dbn, n_pos, c);
}

hipError_t sib_maxpool_fwd(const float* x, float* y, uint8_t* idx, int B, int th, int c,
                           hipStream_t stream) {
  const int64_t n = (int64_t)B * th * c;
  SIB_LAUNCH(maxpool_fwd_kernel, grid1(n, 256), dim3(256), x, y, idx, n, c);
}

hipError_t sib_maxpool_bwd(const float* dy, const uint8_t* idx, float* dx, int B, int th, int c,
                           hipStream_t stream) {
  const int64_t n = (int64_t)B * th * c;
  SIB_LAUNCH(maxpool_bwd_kernel, grid1(n, 256), dim3(256), dy, idx, dx, n, c);
}

hipError_t sib_avgpool4_fwd(const float* x, float* y, int B, int tq, int c, hipStream_t stream) {
  const int64_t n = (int64_t)B * tq * c;
  SIB_LAUNCH(avgpool4_fwd_kernel, grid1(n, 256), dim3(256), x, y, n, c);
}

hipError_t sib_avgpool4_bwd(const float* dxs, float* dx, int B, hipStream_t stream) {
  SIB_LAUNCH(avgpool4_bwd_kernel, grid1((int64_t)B * 32 * SIB_LSTM_D, 256), dim3(256), dxs, dx, B);
}

hipError_t sib_lstm_fwd(const SibLstm& a, hipStream_t stream) {
  const dim3 grid(SIB_LSTM_U / LS_UB, 2, (a.B + LS_NB - 1) / LS_NB);
  for (int s = 0; s < a.T; ++s) {
    hipLaunchKernelGGL(lstm_fwd_step_kernel, grid, dim3(LS_NT), 0, stream, a, s);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t sib_lstm_bwd(const SibLstm& a, hipStream_t stream) {
  for (int s = a.T - 1; s >= 0; --s) {
    hipLaunchKernelGGL(lstm_bwd_gates_kernel, grid1((int64_t)2 * a.B * SIB_LSTM_U, 256), dim3(256), 0, stream,
                       a, s);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int n_rows = s > 0 ? LS_IN : SIB_LSTM_D;   // nothing precedes the first step
    hipLaunchKernelGGL(lstm_bwd_mm_kernel, dim3((n_rows + 3) / 4, 2, (a.B + LS_NB - 1) / LS_NB), dim3(256), 0,
                       stream, a, s, n_rows);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  SIB_LAUNCH(lstm_bwd_w_kernel, dim3(SIB_LSTM_G / 256, LS_IN + 1, 2), dim3(256), a);
}

hipError_t sib_head_loss(const SibHead& a, hipStream_t stream) {
  if (a.K < 1 || a.K > HD_K) return hipErrorInvalidValue;
  SIB_LAUNCH(head_loss_kernel, dim3(1), dim3(HD_NT), a);
}

hipError_t sib_head_bwd(const SibHead& a, float* gw, float* gb, float* demb, hipStream_t stream) {
  SIB_LAUNCH(head_bwd_kernel, grid1((int64_t)HD_D * a.K + a.K + (int64_t)a.B * HD_D, 256), dim3(256), a, gw,
             gb, demb);
}

hipError_t sib_l2(const SibL2& a, double* r, hipStream_t stream) {
  SIB_LAUNCH(l2_kernel, dim3(1), dim3(L2_NT), a, r);
}

hipError_t sib_rmsprop(float* w, float* rms, const float* g, const uint8_t* trainable, int64_t n,
                       float lr, hipStream_t stream) {
  SIB_LAUNCH(rmsprop_kernel, grid1(n, 256), dim3(256), w, rms, g, trainable, n, lr);
}

hipError_t sib_fold_batch(double* st, int nb, hipStream_t stream) {
  SIB_LAUNCH(fold_batch_kernel, dim3(1), dim3(1), st, nb);
}

hipError_t sib_end_epoch(double* st, int n_train, int n_val, float* row, hipStream_t stream) {
  SIB_LAUNCH(end_epoch_kernel, dim3(1), dim3(1), st, n_train, n_val, row);
}

hipError_t sib_loss_pair(const double* st, int n, float* loss, hipStream_t stream) {
  SIB_LAUNCH(loss_pair_kernel, dim3(1), dim3(1), st, n, loss);
}
