// Adapting OD-NET to a room (OverlapDetector.continue_train_model): the float32 training pieces that
// conv.hip (every forward convolution and every stride-1 data gradient) and si_bwd.hip (the BiLSTM)
// do not already have.  See od_bwd.hip.  Activations are channels-last [B, H, W, C]; parameters and
// gradients keep the Keras layouts of the packed blob (Conv2D [kh, kw, cin, cout], BN = gamma, beta,
// moving_mean, moving_variance).  Every launcher enqueues on `stream` and returns the launch status;
// none synchronises, none uses a floating-point atomic: a sum over pixels is split into slabs whose
// count depends on the shape alone, and the slabs' partial sums are added in slab order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int ODB_MAX_C = 128;          // widest layer
constexpr int ODB_RED_SLABS = 256;      // most slabs of a per-channel reduction
constexpr int ODB_WG_SLABS = 128;       // most slabs of a weight gradient
constexpr int ODB_HEAD_D = 512;         // BiLSTM output width
constexpr int ODB_MAX_BATCH = 64;       // = MMLA_OD_TRAIN_MAX_BATCH
constexpr int ODB_MAX_K = 8;            // = MMLA_OD_MAX_CLASSES

// one Conv2D: x [B, h, w, cin] -> y [B, ho, wo, cout], y[ho][wo] = sum x[ho s + dy - pad_h][wo s + dx - pad_w]
struct OdbConv {
  int B, h, w, cin, ho, wo, cout, kh, kw, stride, pad_h, pad_w;
};

// per-BatchNorm scratch of one step: mean, istd, scale, shift, then mean(g), mean(g xhat) of the
// backward pass; each [ODB_MAX_C]
constexpr int ODB_STAT = 6 * ODB_MAX_C;

// xb[s] = float(img[row(s)]), lb[s] = labels[row(s)], mb[s] = mask ? mask[row(s)] != 0 : 1;
// row(s) = order ? clamp(order[i0 + s], 0, n - 1) : i0 + s;  img rows of img_bytes, mask rows of 512
hipError_t odb_gather(const uint8_t* img, const int32_t* labels, const uint8_t* mask, const int32_t* order,
                      int i0, int nb, int n, int img_bytes, float* xb, int32_t* lb, uint8_t* mb,
                      hipStream_t stream);

// training mode: stat = batch mean, 1 / sqrt(biased var + 1e-3), scale = gamma istd, shift = beta - mean scale
// over the n_pos rows of x [n_pos, c]; bn (gamma, beta, moving_mean, moving_variance) gets
// moving <- 0.99 moving + 0.01 batch (the variance Bessel-corrected).  part: [ODB_RED_SLABS, 2, ODB_MAX_C].
// c in {16, 32, 64, 128}.  4 launches
hipError_t odb_bn_batch(const float* x, int64_t n_pos, int c, float* bn, float* stat, float* part,
                        hipStream_t stream);
// inference mode: scale / shift from the moving statistics
hipError_t odb_bn_moving(const float* bn, int c, float* stat, hipStream_t stream);

// g = dy elu'(scale x + shift); dgamma = sum g xhat, dbeta = sum g -> dbn[0..2c);
// dx = scale (g - mean(g) - xhat mean(g xhat)) (+ add, nullable, may alias dx).  3 launches
hipError_t odb_bn_elu_bwd(const float* x, const float* dy, int64_t n_pos, int c, float* stat, float* part,
                          const float* add, float* dx, float* dbn, hipStream_t stream);

// db[c] = sum over the n_pos rows of dy [n_pos, c].  2 launches
hipError_t odb_bias_grad(const float* dy, int64_t n_pos, int c, float* part, float* db, hipStream_t stream);

// slabs of a weight gradient over P output pixels, and the floats of its partial results
int odb_wgrad_slabs(int64_t P);
size_t odb_wgrad_part_floats(const OdbConv& g);
// dw[tap][ci][co] = sum_p a[p (+) tap][ci] dy[p][co], a = scale ? elu(scale x + shift) : x, padding taps 0;
// f32 MFMA over slabs of pixels, then the slabs added in order.  2 launches
hipError_t odb_conv_wgrad(const OdbConv& g, const float* x, const float* scale, const float* shift,
                          const float* dy, float* part, float* dw, hipStream_t stream);

// wt[kh - 1 - dy][kw - 1 - dx][co][ci] = w[dy][dx][ci][co], rows padded with 0 to cin_pad: the kernel of
// the data gradient as a forward convolution (padding kh - 1 - pad_h, kw - 1 - pad_w)
hipError_t odb_conv_transpose(const OdbConv& g, int cin_pad, const float* w, float* wt, hipStream_t stream);
// out [rows, cols_pad] = in [rows, cols], 0 beyond
hipError_t odb_pad_cols(const float* in, int rows, int cols, int cols_pad, float* out, hipStream_t stream);
// the 1 x 1 stride-2 shortcut: dx [B, h, w, cin] = dy [B, ho, wo, cout] . wt [cout, cin_pad] at the even
// positions, 0 elsewhere
hipError_t odb_shortcut_bwd_data(const OdbConv& g, int cin_pad, const float* dy, const float* wt, float* dx,
                                 hipStream_t stream);

// 2 x 2 'same' max-pool: idx [B, ho, wo, c] = which candidate (2 dy + dx) of x [B, h, w, c] wins; the first
// in row-major order on a tie, the padding never
hipError_t odb_pool_winner(const float* x, uint8_t* idx, int B, int h, int w, int c, hipStream_t stream);
// dx [B, h, w, c] = dy of the window it won, else 0
hipError_t odb_pool_bwd(const float* dy, const uint8_t* idx, float* dx, int B, int h, int w, int c,
                        hipStream_t stream);

// seq [B, w, c] = mean over h of x [B, h, w, c]; dx = (dxs[0] + dxs[1]) / h of the BiLSTM's two directions
hipError_t odb_mean_h(const float* x, float* seq, int B, int h, int w, int c, hipStream_t stream);
hipError_t odb_mean_h_bwd(const float* dxs, float* dx, int B, int h, int w, int c, hipStream_t stream);

// Dropout mask x 1 / 0.75 (training), LeakyReLU(float32(0.3)), Dense(K), softmax, the weighted loss.
// 2 <= K <= ODB_MAX_K (else hipErrorInvalidValue).  K == 2 runs the two-class kernels, whose sums keep their
// order; any other K the K-class ones: logits z_k = b_k then fmaf over d ascending, q = p / sum p (k ascending),
// a hit when the first-index argmax of q is the label, demb = slope * sum_k dz_k w[d][k] with k ascending
struct OdbHead {
  const float* emb;        // [B, 512]
  const uint8_t* mask;     // [B, 512], nullable: inference mode (no dropout, no scale)
  const float* w;          // [512, K]
  const float* b;          // [K]
  const int32_t* labels;   // [B]; K == 2: bit 0 is used, else clamped into [0, K - 1]
  float cw[ODB_MAX_K];     // [K]
  float* dz;               // [B, K] gradient at the logits (nullable)
  double* acc;             // [2]: += sum of the samples' losses, += hits
  int B;
  float bsz;
  float* probs;            // [B, K] the softmax outputs (nullable)
  int K;
};
hipError_t odb_head_loss(const OdbHead& a, hipStream_t stream);
// gw [512, K], gb [K], demb [B, 512]
hipError_t odb_head_bwd(const OdbHead& a, float* gw, float* gb, float* demb, hipStream_t stream);

// Keras Adadelta (rho 0.95, epsilon 1e-7) over the flat blob, lr = lrs[ep]; entries with trainable[i] == 0 skipped
hipError_t odb_adadelta(float* w, float* acc_g, float* acc_d, const float* g, const uint8_t* trainable,
                        int64_t n, const float* lrs, int ep, hipStream_t stream);

// history row = loss, acc, val_loss, val_acc (NaN when n_val == 0), lr from st (si_bwd.h's layout); st cleared
hipError_t odb_end_epoch(double* st, int n_train, int n_val, const float* lrs, int ep, float* row,
                         hipStream_t stream);
// loss[0] = st[0] / n
hipError_t odb_loss_out(const double* st, int n, float* loss, hipStream_t stream);
hipError_t odb_fill(float* p, int64_t n, float v, hipStream_t stream);

// ---- training from scratch (OverlapDetector.train_model): device keep-bits and the AUC metric --------------

// mask [n, 512] bytes: element d of the sample with id sid[s] is kept (1) iff word d % 4 of Philox4x32-10
// (philox.h), key = the halves of seed, counter = (d / 4, sid[s], epoch, 2), is >= 0x40000000 (rate 0.25)
hipError_t odb_drop_mask(uint64_t seed, uint32_t epoch, const int32_t* sid, int n, uint8_t* mask,
                         hipStream_t stream);

// tf.keras.metrics.AUC() at its defaults: 200 thresholds, float32(-1e-7), float32((i + 1) / 199.0) (the
// quotient in double), float32(1 + 1e-7); a prediction is positive iff p > thr
constexpr int ODB_AUC_T = 200;
constexpr int ODB_AUC_SLABS = 256;                     // most slabs of one count
constexpr int ODB_AUC_COUNTS = 2 * ODB_AUC_T;          // words of one slab's counts: TP, FP per threshold
struct OdbAucThr {
  float t[ODB_AUC_T];
};
OdbAucThr odb_auc_thresholds();
// slabs of a count over n samples: min(ODB_AUC_SLABS, ceil(n / 4096))
int odb_auc_slabs(int64_t n);
// counts [slabs, 200, 2] (uint32): over the K n entries of probs [n, K] against the one-hot rows of labels
// (K == 2: bit 0; else clamped into [0, K - 1]), TP (the label's entry) and FP (the K - 1 others) per
// threshold; add != 0: added to what counts holds, else written.  Integer counts and no atomics: one thread
// per threshold walks its slab's rows.  2 <= K <= ODB_MAX_K
hipError_t odb_auc_count(const float* probs, const int32_t* labels, int64_t n, int K, const OdbAucThr& thr, int add,
                         uint32_t* counts, hipStream_t stream);
// out[0] = float32 of sum_t (fpr[t] - fpr[t + 1]) (recall[t] + recall[t + 1]) / 2 in double from the slabs'
// integer sums; the K n entries hold n positives and (K - 1) n negatives, so recall = TP / n and
// fpr = FP / ((K - 1) n).  n == 0: NaN.  clear != 0: counts zeroed afterwards
hipError_t odb_auc_final(uint32_t* counts, int slabs, int64_t n, int K, int clear, float* out, hipStream_t stream);
