// Training the SI base model from scratch (speaker_identification.py:221-250): what separates `train`
// from the fine-tune of si_bwd.h -- BatchNorm on batch statistics, the two Dropout layers with keep-bits
// generated on the device, and a softmax head of up to MMLA_SI_BASE_MAX_CLASSES classes.  See
// si_base.hip.  All float32, activations channels-last [B, T, C]; every launcher enqueues on `stream`
// and returns the launch status; none synchronises.  No floating-point atomics: a sum over positions is
// split into slabs whose count depends on the shape alone, and the partials are added in slab order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int SBB_MAX_C = 128;                 // widest BatchNorm of SI-NET
constexpr int SBB_SLABS = 256;                 // most slabs of a per-channel reduction
constexpr int SBB_STAT = 2 * SBB_MAX_C;        // per-BatchNorm scratch kept for the backward: mean, istd
constexpr int SBB_PART = 2 * SBB_SLABS * SBB_MAX_C;   // floats of the slab partials (two sums)
constexpr int SBB_MAP = 32 * 128;              // dropout site 0: the [32, 128] map in front of the avg-pool
constexpr int SBB_EMB = 512;                   // dropout site 1: the embedding
constexpr uint32_t SBB_RATE_A = 0x40000000u;   // 0.25 as a 32-bit fraction
constexpr uint32_t SBB_RATE_B = 0x33333333u;   // 0.2

// where the keep-bits of one pass come from: Philox4x32-10, key = the halves of seed, counter =
// (element / 4, sid[sample of the batch], epoch, site), word = element % 4; kept iff word >= rate
struct SbbDrop {
  uint64_t seed;
  uint32_t epoch;
  const int32_t* sid;   // [B] rows of the training set
};

// sid[s] = ids ? ids[row(s)] : row(s), row(s) = order ? clamp(order[i0 + s], 0, n - 1) : i0 + s
hipError_t sbb_ids(const int32_t* ids, const int32_t* order, int i0, int nb, int n, int32_t* sid,
                   hipStream_t stream);
// the keep-bits as bytes (1 kept, 0 dropped): mask_a [n, 32, 128] of site 0, mask_b [n, 512] of site 1
hipError_t sbb_drop_mask(const SbbDrop& d, int n, uint8_t* mask_a, uint8_t* mask_b, hipStream_t stream);

// y = relu(gamma (x - mean) istd + beta) over the n_pos rows of x [n_pos, c], mean and biased variance of
// the batch in two passes (the mean, then the centred squares), istd = 1 / sqrt(var + 1e-3); stat keeps
// mean, istd ([2, c]); bn (gamma, beta, moving_mean, moving_variance) gets moving <- 0.99 moving + 0.01
// batch, the variance NOT Bessel-corrected.  part: SBB_PART floats.  c a multiple of 32, <= 128.
// 3 launches
hipError_t sbb_bn_relu_fwd(const float* x, float* bn, float* y, int n_pos, int c, float* stat, float* part,
                           hipStream_t stream);
// g = dy [y > 0]; dbn[0..2c) = dgamma = sum g xhat, dbeta = sum g;
// dx = gamma istd (g - mean(g) - xhat mean(g xhat)) (+ add, nullable; may alias dx).  2 launches
hipError_t sbb_bn_relu_bwd(const float* x, const float* y, const float* dy, const float* bn,
                           const float* stat, float* part, const float* add, float* dx, float* dbn, int n_pos,
                           int c, hipStream_t stream);

// Dropout(0.25) of x [B, 32, 128] (kept x float32(1 / 0.75)) then the mean over groups of four steps
// -> y [B, 8, 128]
hipError_t sbb_drop_avgpool4_fwd(const float* x, float* y, int B, const SbbDrop& d, hipStream_t stream);
// dx [B, 32, 128] from the two directions' input gradients dxs [2, B, 8, 128], through the same mask
hipError_t sbb_drop_avgpool4_bwd(const float* dxs, float* dx, int B, const SbbDrop& d, hipStream_t stream);

// Dropout(0.2) of the embedding (training; kept x float32(1 / 0.8)), Dense(512 -> K), and the loss on the
// logits: logsumexp(z) - z[label], no clip; dz = (softmax - onehot) / bsz; a hit when the first maximum
// is the label.  A label is clamped into [0, K).
struct SbbHead {
  const float* emb;        // [B, 512]
  const float* w;          // [512, K]
  const float* b;          // [K]
  const int32_t* labels;   // [B]
  float* embd;             // [B, 512] the embedding after dropout (training) or as it is
  float* dmul;             // [B, 512] what it was multiplied by: 0, 1 / 0.8, or 1 without dropout
  float* dz;               // [B, K] gradient at the logits (nullable: evaluation only)
  float* loss;             // [B] scratch
  int32_t* hit;            // [B] scratch
  double* acc;             // [2]: += sum of the samples' losses, += hits
  int B, K;
  float bsz;               // the divisor of the batch mean
  int drop;                // 1: training mode
};
hipError_t sbb_head_loss(const SbbHead& a, const SbbDrop& d, hipStream_t stream);   // 2 launches
// gw [512, K], gb [K], demb [B, 512] (the gradient in front of the dropout)
hipError_t sbb_head_bwd(const SbbHead& a, float* gw, float* gb, float* demb, hipStream_t stream);
