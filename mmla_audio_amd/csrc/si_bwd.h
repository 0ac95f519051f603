// Speaker registration, stage 2 of transfer_learning: the float32 training forward of SI-NET and the
// backward of every layer kind it has, plus RMSprop over the packed parameter blob.  See si_bwd.hip.
// Activations are channels-last [B, T, C]; parameters keep the Keras layouts of the packed blob
// (Conv1D [k, cin, cout], LSTM [in, 4u] gates i,f,c,o, Dense [512, K]).  Every launcher enqueues on
// `stream` and returns the launch status; none synchronises.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int SIB_LSTM_U = 256;    // LSTM units per direction
constexpr int SIB_LSTM_D = 128;    // LSTM input width
constexpr int SIB_LSTM_T = 8;      // LSTM steps of SI-NET (SibLstm::T; OD-NET runs 1..19, od_bwd.h)
constexpr int SIB_LSTM_G = 4 * SIB_LSTM_U;

struct SibConv {
  int B, tin, tout, cin, cout, k, stride, pad_l;
};

// xb[s] = x[row(s)], lb[s] = labels[row(s)], row(s) = order ? clamp(order[i0 + s], 0, n - 1) : i0 + s
hipError_t sib_gather(const float* x, const int32_t* labels, const int32_t* order, int i0, int nb, int n,
                      int row_floats, float* xb, int32_t* lb, hipStream_t stream);

// y = conv(x) + bias (+ res, nullable)
hipError_t sib_conv_fwd(const SibConv& g, const float* x, const float* w, const float* bias,
                        const float* res, float* y, hipStream_t stream);
// wt [k, cout, cin] = transpose of w [k, cin, cout]
hipError_t sib_conv_transpose(const SibConv& g, const float* w, float* wt, hipStream_t stream);
// dx = (add, nullable; may alias dx) + dy (*) wt
hipError_t sib_conv_bwd_data(const SibConv& g, const float* dy, const float* wt, const float* add,
                             float* dx, hipStream_t stream);
// dw = sum over the B * tout positions of x (x) dy + l2x2 * w; db = sum of dy
hipError_t sib_conv_bwd_weight(const SibConv& g, const float* x, const float* dy, const float* w,
                               float l2x2, float* dw, float* db, hipStream_t stream);

// bn = gamma, beta, moving_mean, moving_variance, each [c], consecutive (the packed order)
hipError_t sib_bn_relu_fwd(const float* x, const float* bn, float* y, int n_pos, int c,
                           hipStream_t stream);
// dx = (add, nullable; may alias dx) + dL/dx; dbn[0..2c) = dgamma, dbeta
hipError_t sib_bn_relu_bwd(const float* x, const float* y, const float* dy, const float* bn,
                           const float* add, float* dx, float* dbn, int n_pos, int c,
                           hipStream_t stream);

// max over time pairs, x [B, 2 th, c] -> y [B, th, c], idx = which of the pair won (first on a tie)
hipError_t sib_maxpool_fwd(const float* x, float* y, uint8_t* idx, int B, int th, int c,
                           hipStream_t stream);
hipError_t sib_maxpool_bwd(const float* dy, const uint8_t* idx, float* dx, int B, int th, int c,
                           hipStream_t stream);
// mean over groups of four steps, x [B, 4 tq, c] -> y [B, tq, c]
hipError_t sib_avgpool4_fwd(const float* x, float* y, int B, int tq, int c, hipStream_t stream);
// dx [B, 32, 128] from the two directions' input gradients dxs [2, B, 8, 128]
hipError_t sib_avgpool4_bwd(const float* dxs, float* dx, int B, hipStream_t stream);

struct SibLstm {
  const float* wk[2];     // [128, 1024]
  const float* wr[2];     // [256, 1024]
  const float* bias[2];   // [1024]
  const float* seq;       // [B, T, 128]
  float* gates;           // [2, T, B, 1024] post-activation i, f, g, o by processing step
  float* cs;              // [2, T, B, 256]
  float* hs;              // [2, T, B, 256]
  float* emb;             // [B, 512] = h_fwd(after x[T - 1]), h_bwd(after x[0])
  // backward
  const float* demb;      // [B, 512]
  float* dz;              // [2, T, B, 1024] gradient at the gates' pre-activations
  float* dh;              // [2, B, 256] scratch
  float* dc;              // [2, B, 256] scratch
  float* dxs;             // [2, B, T, 128]
  float* dwk[2];          // gradients, the layouts of wk, wr, bias
  float* dwr[2];
  float* dbias[2];
  int B;
  int T;                  // steps, >= 1 (SI-NET: SIB_LSTM_T)
};
hipError_t sib_lstm_fwd(const SibLstm& a, hipStream_t stream);   // T launches
hipError_t sib_lstm_bwd(const SibLstm& a, hipStream_t stream);   // 2 T + 1 launches

struct SibHead {
  const float* emb;        // [B, 512]
  const float* w;          // [512, K]
  const float* b;          // [K]
  const int32_t* labels;   // [B]
  float* dz;               // [B, K] gradient at the logits (nullable: evaluation only)
  double* acc;             // [2]: += sum of the samples' losses, += hits
  int B, K;
  float bsz;               // the divisor of the batch mean
};
hipError_t sib_head_loss(const SibHead& a, hipStream_t stream);
// gw [512, K], gb [K], demb [B, 512]
hipError_t sib_head_bwd(const SibHead& a, float* gw, float* gb, float* demb, hipStream_t stream);

// r[0] = sum_i lambda[i] * sum(w_i^2) over n_t <= 8 tensors (float64 accumulation, fixed tree)
struct SibL2 {
  const float* w[8];
  int n[8];
  float lambda[8];
  int n_t;
};
hipError_t sib_l2(const SibL2& a, double* r, hipStream_t stream);

// Keras RMSprop (rho 0.9, momentum 0, epsilon 1e-7 outside the root) over the flat blob; entries with
// trainable[i] == 0 (the moving statistics) are skipped
hipError_t sib_rmsprop(float* w, float* rms, const float* g, const uint8_t* trainable, int64_t n,
                       float lr, hipStream_t stream);

// bookkeeping of the fit, all on the device: st = {batch data-loss sum, batch hits, R, epoch total,
// epoch hits, val data-loss sum, val hits}
constexpr int SIB_ST = 8;
// epoch total += batch sum + R * nb; epoch hits += batch hits; batch sums cleared
hipError_t sib_fold_batch(double* st, int nb, hipStream_t stream);
// history row = total / n_train, hits / n_train, val sum / n_val + R, val hits / n_val (NaN when
// n_val == 0); everything cleared
hipError_t sib_end_epoch(double* st, int n_train, int n_val, float* row, hipStream_t stream);
// loss[0] = batch sum / n, loss[1] = R
hipError_t sib_loss_pair(const double* st, int n, float* loss, hipStream_t stream);
