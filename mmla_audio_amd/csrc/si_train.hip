// Speaker registration, stage 1 of transfer_learning (speaker_identification.py:401-432): fit
// Dense(K, sigmoid) on the frozen base's 512-float embeddings with categorical_crossentropy and
// RMSprop(1e-4), batch 16, as ONE launch.  Restart r is one workgroup of 512 threads that runs every
// epoch and every step itself; nothing but the batch's embedding rows (resident in L2: n x 2 KB) is
// read from memory per step, and nothing is written before the fit ends except one history row per
// epoch.  Float32 throughout (plain FMA: a step is 16 x 512 x K MACs, its cost is barriers and LDS
// latency, not arithmetic rate); only the reported loss goes through float64: one lane per sample
// takes the correctly rounded f32 log, and the epoch's total of those f32 losses is summed in f64.
//
// On chip, per workgroup:
//   LDS   w[512][33]     the head, row stride 33 (odd: thread d updating row d and the forward's
//                        lanes reading 32 classes of one row are both free of bank conflicts)
//         e[16][512]     the chunk's embedding rows (a batch is walked in chunks of 16 samples)
//         part[16][16][32] forward partial sums, dz[16][32], bias[32], per-sample loss / hit
//   VGPR  thread d holds row d of the RMSprop accumulator and of the batch gradient (32 + 32)
// A chunk, four barriers:
//   1 load    thread d copies e[s][d] of the chunk's rows (coalesced 2 KB rows)
//   2 forward thread (j, k) = (t / 32, t % 32) sums e[s][32 j .. 32 j + 32) . w[.][k] for the 16
//             samples (32 + 128 LDS reads for 512 FMAs) -> part[j][s][k]
//   3 z, loss thread (s, k) adds the 16 partials in fixed order + bias -> sigmoid; the 32 lanes of a
//             sample reduce S = sum_k s_k and the first-index argmax with xor shuffles (every lane
//             gets the same bits), fetch s_c by shuffle, and write dz[s][k], loss[s], hit[s]
//   4 grad    thread d: g[d][k] += e[s][d] dz[s][k] (dz read as broadcast float4); threads < K: gb
// and after a batch's last chunk thread d applies RMSprop to row d in place.  No atomics, every sum
// in a fixed order: bit-reproducible, and restart r never sees how many restarts run beside it.
#include "../../include/mmla.h"
#include "si_train.h"

namespace {

constexpr int NT = 512;
constexpr int D = MMLA_SI_EMBED;
constexpr int KM = MMLA_SI_TRAIN_MAX_CLASSES;
constexpr int LDW = KM + 1;
constexpr int SB = 16;   // samples per chunk
static_assert(NT == D && NT == SB * KM && KM == 32 && D % 128 == 0, "thread maps of the phases");

struct Smem {
  float e[SB][D];
  float part[SB][SB][KM];   // [d-group j][sample][class]
  float dz[SB][KM];
  float w[D * LDW];
  float bias[KM];
  float loss[SB];
  int hit[SB];
};

__global__ void __launch_bounds__(NT, 1) si_train_kernel(SiTrainArgs a) {
  __shared__ __attribute__((aligned(16))) Smem sm;
  const int t = threadIdx.x, r = blockIdx.x;
  const int K = a.k;
  const int k = t & 31, j = t >> 5;
  const float lo = 1e-7f, hi = 1.0f - 1e-7f;   // clip bounds, formed in f32

  float g[KM], rms[KM];
#pragma unroll
  for (int c = 0; c < KM; ++c) {
    g[c] = 0.0f;
    rms[c] = 0.0f;
  }
  float gb = 0.0f, rms_b = 0.0f;   // threads < K: the bias
  for (int c = 0; c < LDW; ++c)
    sm.w[t * LDW + c] = c < K ? a.w0[((size_t)r * D + t) * K + c] : 0.0f;
  if (t < KM) sm.bias[t] = t < K ? a.b0[(size_t)r * K + t] : 0.0f;

  double lsum = 0.0;   // thread 0: the running loss total and hit count of the pass
  int hits = 0;

  // one chunk of nb <= 16 samples: rows order[i0 + s] (order null: i0 + s) of src
  auto chunk = [&](const float* __restrict__ src, const int32_t* __restrict__ lab,
                   const int32_t* __restrict__ order, int i0, int nb, float bsz, bool train) {
    // a perm entry is clamped into the set: host-pointer calls were checked, a device-pointer caller
    // who breaks the contract gets a wrong fit, not a read outside emb
    auto row_of = [&](int s) { return order ? min(max(order[i0 + s], 0), a.n_train - 1) : i0 + s; };
#pragma unroll 4
    for (int s = 0; s < SB; ++s) {
      float v = 0.0f;
      if (s < nb) v = src[(size_t)row_of(s) * D + t];
      sm.e[s][t] = v;
    }
    __syncthreads();
    {
      float acc[SB];
#pragma unroll
      for (int s = 0; s < SB; ++s) acc[s] = 0.0f;
#pragma unroll 2
      for (int q = 0; q < 8; ++q) {
        const int d = j * 32 + q * 4;
        const float w0 = sm.w[d * LDW + k], w1 = sm.w[(d + 1) * LDW + k];
        const float w2 = sm.w[(d + 2) * LDW + k], w3 = sm.w[(d + 3) * LDW + k];
#pragma unroll
        for (int s = 0; s < SB; ++s) {
          const float4 ev = *reinterpret_cast<const float4*>(&sm.e[s][d]);
          acc[s] = fmaf(ev.x, w0, acc[s]);
          acc[s] = fmaf(ev.y, w1, acc[s]);
          acc[s] = fmaf(ev.z, w2, acc[s]);
          acc[s] = fmaf(ev.w, w3, acc[s]);
        }
      }
#pragma unroll
      for (int s = 0; s < SB; ++s) sm.part[j][s][k] = acc[s];
    }
    __syncthreads();
    {
      const int s = j;   // this thread's sample; its 32 lanes are one half of a wave
      float z = sm.bias[k];
#pragma unroll
      for (int q = 0; q < SB; ++q) z += sm.part[q][s][k];
      const float sig = 1.0f / (1.0f + expf(-z));
      const bool live = k < K && s < nb;
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
      if (s < nb) c = lab[row_of(s)] & (KM - 1);   // a lane index for the shuffle below
      const float sc = __shfl(sig, c, 32);
      const float p = sc / S;
      const bool inside = p >= lo && p <= hi;   // clip_by_value passes the gradient inside only
      if (train) {
        float v = 0.0f;
        if (live && inside) v = sig * (1.0f - sig) * (1.0f / S - (k == c ? 1.0f / sc : 0.0f)) / bsz;
        sm.dz[s][k] = v;
      }
      if (k == 0) {
        // the f32 log of the f32 p, correctly rounded (through f64: logf is a 1-ulp routine, and
        // -log(1 - 2^-23), the loss of a clipped sample, sits 2^-70 off a rounding midpoint)
        sm.loss[s] = s < nb ? (float)(-log((double)fminf(fmaxf(p, lo), hi))) : 0.0f;
        sm.hit[s] = s < nb && arg == c ? 1 : 0;
      }
    }
    __syncthreads();
    if (t == 0)
      for (int s = 0; s < nb; ++s) {
        lsum += (double)sm.loss[s];
        hits += sm.hit[s];
      }
    if (!train) return;
    for (int s = 0; s < nb; ++s) {
      const float ev = sm.e[s][t];
#pragma unroll
      for (int q = 0; q < KM / 4; ++q) {
        if (q * 4 < K) {
          const float4 dv = *reinterpret_cast<const float4*>(&sm.dz[s][q * 4]);
          g[q * 4] = fmaf(ev, dv.x, g[q * 4]);
          g[q * 4 + 1] = fmaf(ev, dv.y, g[q * 4 + 1]);
          g[q * 4 + 2] = fmaf(ev, dv.z, g[q * 4 + 2]);
          g[q * 4 + 3] = fmaf(ev, dv.w, g[q * 4 + 3]);
        }
      }
    }
    if (t < K)
      for (int s = 0; s < nb; ++s) gb += sm.dz[s][t];
  };

  for (int ep = 0; ep < a.epochs; ++ep) {
    const int32_t* order = a.perm + ((size_t)r * a.epochs + ep) * a.n_train;
    lsum = 0.0;
    hits = 0;
    for (int b0 = 0; b0 < a.n_train; b0 += a.batch) {
      const int bsz = min(a.batch, a.n_train - b0);
      for (int c0 = 0; c0 < bsz; c0 += SB) {
        chunk(a.emb, a.labels, order, b0 + c0, min(SB, bsz - c0), (float)bsz, true);
        if (c0 + SB < bsz) __syncthreads();   // the gradient phase still reads e and dz
      }
      // RMSprop (Keras: rho 0.9, momentum 0, epsilon 1e-7 outside the root), row t and the bias
#pragma unroll
      for (int c = 0; c < KM; ++c) {
        if (c < K) {
          const float gv = g[c];
          const float rv = 0.9f * rms[c] + 0.1f * (gv * gv);
          rms[c] = rv;
          sm.w[t * LDW + c] -= (a.lr * gv) / (sqrtf(rv) + 1e-7f);
          g[c] = 0.0f;
        }
      }
      if (t < K) {
        rms_b = 0.9f * rms_b + 0.1f * (gb * gb);
        sm.bias[t] -= (a.lr * gb) / (sqrtf(rms_b) + 1e-7f);
        gb = 0.0f;
      }
      __syncthreads();
    }
    const float tr_loss = (float)(lsum / a.n_train), tr_acc = (float)((double)hits / a.n_train);
    lsum = 0.0;
    hits = 0;
    for (int v0 = 0; v0 < a.n_val; v0 += SB)
      chunk(a.val_emb, a.val_labels, nullptr, v0, min(SB, a.n_val - v0), 1.0f, false);
    if (t == 0 && a.history) {
      float* h = a.history + ((size_t)r * a.epochs + ep) * 4;
      h[0] = tr_loss;
      h[1] = tr_acc;
      h[2] = a.n_val > 0 ? (float)(lsum / a.n_val) : __builtin_nanf("");
      h[3] = a.n_val > 0 ? (float)((double)hits / a.n_val) : __builtin_nanf("");
    }
  }
  for (int c = 0; c < K; ++c) a.w[((size_t)r * D + t) * K + c] = sm.w[t * LDW + c];
  if (t < K) a.b[(size_t)r * K + t] = sm.bias[t];
}

}  // namespace

hipError_t si_train_launch(const SiTrainArgs& a, int n_restarts, hipStream_t stream) {
  hipLaunchKernelGGL(si_train_kernel, dim3(n_restarts), dim3(NT), 0, stream, a);
  return hipGetLastError();
}
