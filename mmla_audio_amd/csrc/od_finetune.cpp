// libmmla: training OD-NET -- adapting it to a room (mmla_od_loss_grad, mmla_od_finetune) and training it from
// scratch (mmla_od_train on the same engine and fit body, with mmla_od_drop_mask, mmla_od_auc and
// mmla_od_augment, the entries of od_aug.hip and of od_bwd.hip's keep-bit and AUC kernels) (include/mmla.h).
// Which kernel runs which layer, forward and backward, over a copy of the packed OD blob in workspace
// slot S_ODFT; the context's loaded model is not touched.  Every forward convolution and every stride-1
// data gradient is conv.hip's conv_launch (exact f32 MFMA); the weight gradients, BatchNorm in training
// mode, the pools and the head are od_bwd.hip's; the BiLSTM is si_bwd.hip's with T = ceil(w / 8) steps.
// A training step is a fixed sequence of launches on the context's stream; the only host synchronisation
// of a fit is the read-back of one history row per epoch when early stopping is on.  The fit itself --
// checks, staging, the epoch loop, early stopping -- is fit_common.h's driver; this file gives it the steps.
#include <algorithm>
#include <cmath>

#include "conv.h"
#include "fit_common.h"
#include "internal.h"
#include "od_aug.h"
#include "od_bwd.h"
#include "si_base.h"
#include "si_bwd.h"

namespace mmla {
namespace {

constexpr int kMinH = 8, kMaxH = OD_H, kMinW = 8, kMaxW = OD_W;
constexpr int C = ODB_MAX_C;

// offsets (in floats) of the tensors of weights.od_spec(K, channels) in the packed blob
struct BlkOff {
  size_t bn_in, ca_w, ca_b, bn_mid, cb_w, cb_b, sc_w, sc_b;
  int cin, cout;
  bool pool;
};
struct OdOff {
  size_t stem_w, stem_b;
  BlkOff u[9];
  size_t lk[2], lr[2], lb[2], dw, db, total;
};

OdOff od_offsets(int K, int ch) {
  OdOff o{};
  size_t at = 0;
  auto take = [&](size_t n) {
    const size_t r = at;
    at += n;
    return r;
  };
  o.stem_w = take((size_t)ch * 16);   // [1,1,ch,16]: the blob's own rows, none for a channel it lacks
  o.stem_b = take(16);
  int cin = 16;
  for (int i = 0; i < 9; ++i) {
    BlkOff& u = o.u[i];
    u.cin = cin;
    u.cout = CH[i];
    u.pool = POOL[i];
    u.bn_in = take(4 * (size_t)cin);
    u.ca_w = take(9 * (size_t)cin * u.cout);
    u.ca_b = take(u.cout);
    u.bn_mid = take(4 * (size_t)u.cout);
    u.cb_w = take(4 * (size_t)u.cout * u.cout);
    u.cb_b = take(u.cout);
    if (u.pool) {
      u.sc_w = take((size_t)cin * u.cout);
      u.sc_b = take(u.cout);
    }
    cin = u.cout;
  }
  for (int d = 0; d < 2; ++d) {
    o.lk[d] = take((size_t)SIB_LSTM_D * SIB_LSTM_G);
    o.lr[d] = take((size_t)SIB_LSTM_U * SIB_LSTM_G);
    o.lb[d] = take(SIB_LSTM_G);
  }
  o.dw = take((size_t)ODB_HEAD_D * K);
  o.db = take(K);
  o.total = at;
  return o;
}

struct BlkAct {
  int h, w, ho, wo;        // the block's input and output sizes
  float *t1, *t2, *out;    // conv 1's output; conv 2's where a pool follows; the block's output
  uint8_t* idx;            // the pool's winner per output
  float *stat_in, *stat_mid;
};

struct Engine {
  mmla_ctx* c = nullptr;
  OdOff off;
  int cap = 0, h = 0, w = 0, T = 0, hl = 0;   // hl x T: the last block's output
  int K = 2;   // classes of the blob's head
  int ch = 3;  // channels of the blob's stem and of the images: 3, or 1 (imagetype='gray')
  float cw[ODB_MAX_K] = {1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f};
  float *W = nullptr, *G = nullptr, *acc_g = nullptr, *acc_d = nullptr, *wt = nullptr, *stem_w = nullptr,
        *stem_b = nullptr, *zero = nullptr, *part = nullptr, *stat_all = nullptr;
  uint8_t* trainable = nullptr;
  double* st = nullptr;
  float *xb = nullptr, *net0 = nullptr, *seq = nullptr, *emb = nullptr, *dzh = nullptr, *demb = nullptr;
  int32_t* lb = nullptr;
  uint8_t* mb = nullptr;
  // mmla_od_train: the batch's sample ids, its softmax outputs, the epoch's AUC counts (training, validation)
  bool auc = false;
  OdbAucThr thr{};
  int32_t* sid = nullptr;
  float* probs = nullptr;
  uint32_t* auc_n = nullptr;
  BlkAct ba[9];
  float* gbuf[3] = {nullptr, nullptr, nullptr};
  SibLstm lstm{};
};

OdbConv geom(int B, int h, int w, int cin, int cout, int kh, int kw, int stride) {
  const int ho = (h + stride - 1) / stride, wo = (w + stride - 1) / stride;
  // Keras 'same': the smaller half first ((4,1): 1 above, 2 below)
  const int ph = std::max((ho - 1) * stride + kh - h, 0) / 2, pw = std::max((wo - 1) * stride + kw - w, 0) / 2;
  return OdbConv{B, h, w, cin, ho, wo, cout, kh, kw, stride, ph, pw};
}

void set_dims(Engine& e, int h, int w) {
  e.h = h;
  e.w = w;
  for (int i = 0; i < 9; ++i) {
    BlkAct& a = e.ba[i];
    a.h = h;
    a.w = w;
    if (POOL[i]) {
      h = (h + 1) / 2;
      w = (w + 1) / 2;
    }
    a.ho = h;
    a.wo = w;
  }
  e.hl = h;
  e.T = w;
}

// the engine's buffers; the pass on a null base only measures (fit_common.h)
void carve(Engine& e, Carver& cv, bool train) {
  const size_t B = e.cap, n = e.off.total, T = e.T;
  const size_t pix = (size_t)e.h * e.w;
  e.W = cv.take<float>(n);
  e.G = cv.take<float>(n);
  e.acc_g = train ? cv.take<float>(n) : nullptr;
  e.acc_d = train ? cv.take<float>(n) : nullptr;
  e.trainable = train ? cv.take<uint8_t>(n) : nullptr;
  e.wt = cv.take<float>(9 * C * C);
  e.stem_w = cv.take<float>(3 * 32);
  e.stem_b = cv.take<float>(32);
  e.zero = cv.take<float>(C);
  e.st = cv.take<double>(SIB_ST);
  e.stat_all = cv.take<float>(18 * (size_t)ODB_STAT);
  e.xb = cv.take<float>(B * pix * 3);
  e.lb = cv.take<int32_t>(B);
  e.mb = cv.take<uint8_t>(B * ODB_HEAD_D);
  e.net0 = cv.take<float>(B * pix * 16);
  size_t part = (size_t)ODB_RED_SLABS * 2 * C;
  part = std::max(part, odb_wgrad_part_floats(geom((int)B, e.h, e.w, e.ch, 16, 1, 1, 1)));
  for (int i = 0; i < 9; ++i) {
    const BlkOff& u = e.off.u[i];
    BlkAct& a = e.ba[i];
    const size_t in = (size_t)a.h * a.w, out = (size_t)a.ho * a.wo;
    a.t1 = cv.take<float>(B * in * u.cout);
    a.t2 = u.pool ? cv.take<float>(B * in * u.cout) : nullptr;
    a.idx = u.pool ? cv.take<uint8_t>(B * out * u.cout) : nullptr;
    a.out = cv.take<float>(B * out * u.cout);
    a.stat_in = e.stat_all ? e.stat_all + (size_t)(2 * i) * ODB_STAT : nullptr;
    a.stat_mid = e.stat_all ? e.stat_all + (size_t)(2 * i + 1) * ODB_STAT : nullptr;
    part = std::max(part, odb_wgrad_part_floats(geom((int)B, a.h, a.w, u.cin, u.cout, 3, 3, 1)));
    part = std::max(part, odb_wgrad_part_floats(geom((int)B, a.h, a.w, u.cout, u.cout, 4, 1, 1)));
    if (u.pool) part = std::max(part, odb_wgrad_part_floats(geom((int)B, a.h, a.w, u.cin, u.cout, 1, 1, 2)));
  }
  e.part = cv.take<float>(part);
  e.seq = cv.take<float>(B * T * SIB_LSTM_D);
  e.emb = cv.take<float>(B * ODB_HEAD_D);
  e.dzh = cv.take<float>(B * e.K);
  e.demb = cv.take<float>(B * ODB_HEAD_D);
  for (int q = 0; q < 3; ++q) e.gbuf[q] = cv.take<float>(B * pix * 32);
  SibLstm& l = e.lstm;
  l.gates = cv.take<float>(2 * T * B * SIB_LSTM_G);
  l.cs = cv.take<float>(2 * T * B * SIB_LSTM_U);
  l.hs = cv.take<float>(2 * T * B * SIB_LSTM_U);
  l.dz = cv.take<float>(2 * T * B * SIB_LSTM_G);
  l.dh = cv.take<float>(2 * B * SIB_LSTM_U);
  l.dc = cv.take<float>(2 * B * SIB_LSTM_U);
  l.dxs = cv.take<float>(2 * B * T * SIB_LSTM_D);
  e.sid = cv.take<int32_t>(B);
  e.probs = cv.take<float>(B * e.K);
  e.auc_n = cv.take<uint32_t>(2 * ODB_AUC_COUNTS);
  if (cv.base) {
    wire_lstm(l, e.off, e.W, e.G);
    l.seq = e.seq;
    l.emb = e.emb;
    l.demb = e.demb;
    l.T = e.T;
  }
}

#define RUN(expr) HIPCHK(e.c, (expr))

// y = conv(act(x)) + bias (+ res): conv.hip on the blob's own kernel (cout is a multiple of 32 but for the
// stem, which runs on a padded copy)
hipError_t conv_fwd(const OdbConv& g, const float* x, const float* wt, const float* bias, int cout_pad,
                    const float* stat, int epi, const float* res, int hp, int wp, float* y, hipStream_t s) {
  ConvArgs a{};
  a.x = x;
  a.wt = wt;
  a.bias = bias;
  a.scale = stat ? stat + 2 * C : nullptr;
  a.shift = stat ? stat + 3 * C : nullptr;
  a.res = res;
  a.y = y;
  a.n = g.B;
  a.h = g.h;
  a.w = g.w;
  a.cin = g.cin;
  a.ho = g.ho;
  a.wo = g.wo;
  a.cout = g.cout;
  a.cout_pad = cout_pad;
  a.ldy = g.cout;
  a.kh = g.kh;
  a.kw = g.kw;
  a.stride = g.stride;
  a.pad_h = g.pad_h;
  a.pad_w = g.pad_w;
  a.hp = hp;
  a.wp = wp;
  a.pro = stat ? PRO_BN_ELU : PRO_NONE;
  a.epi = epi;
  return conv_launch(a, s);
}

inline int pad32(int c) { return (c + 31) / 32 * 32; }

// the data gradient of the stride-1 convolution g: da [B, h, w, cin] = dy (*) flipped, transposed kernel
int conv_bwd_data(Engine& e, const OdbConv& g, const float* w, const float* dy, float* da) {
  hipStream_t s = e.c->stream;
  const int cp = pad32(g.cin);
  RUN(odb_conv_transpose(g, cp, w, e.wt, s));
  const OdbConv t{g.B, g.h, g.w, g.cout, g.h, g.w, g.cin, g.kh, g.kw, 1, g.kh - 1 - g.pad_h, g.kw - 1 - g.pad_w};
  RUN(conv_fwd(t, dy, e.wt, e.zero, cp, nullptr, EPI_BIAS, nullptr, 0, 0, da, s));
  return MMLA_OK;
}

int batch_norm(Engine& e, bool train, const float* x, int64_t n_pos, int c, size_t bn, float* stat) {
  if (train)
    RUN(odb_bn_batch(x, n_pos, c, e.W + bn, stat, e.part, e.c->stream));
  else
    RUN(odb_bn_moving(e.W + bn, c, stat, e.c->stream));
  return MMLA_OK;
}

OdbHead head_args(const Engine& e, int B, const uint8_t* mask, float* dz, double* acc, float* probs) {
  OdbHead h{};
  h.emb = e.emb;
  h.mask = mask;
  h.w = e.W + e.off.dw;
  h.b = e.W + e.off.db;
  h.labels = e.lb;
  for (int k = 0; k < e.K; ++k) h.cw[k] = e.cw[k];
  h.dz = dz;
  h.acc = acc;
  h.B = B;
  h.bsz = (float)B;
  h.probs = probs;
  h.K = e.K;
  return h;
}

// forward of the B images in xb / lb / mb; train: batch statistics (the moving ones advance), dropout, the
// pools' winners and dz kept; else the moving statistics and no dropout.  acc: += loss sum, += hits
int forward(Engine& e, int B, bool train, double* acc) {
  hipStream_t s = e.c->stream;
  const float* W = e.W;
  RUN(odb_pad_cols(W + e.off.stem_w, e.ch, 16, 32, e.stem_w, s));
  RUN(odb_pad_cols(W + e.off.stem_b, 1, 16, 32, e.stem_b, s));
  RUN(conv_fwd(geom(B, e.h, e.w, e.ch, 16, 1, 1, 1), e.xb, e.stem_w, e.stem_b, 32, nullptr, EPI_BIAS, nullptr, 0, 0,
               e.net0, s));
  const float* net = e.net0;
  for (int i = 0; i < 9; ++i) {
    const BlkOff& u = e.off.u[i];
    const BlkAct& a = e.ba[i];
    const int64_t n_pos = (int64_t)B * a.h * a.w;
    CHK(batch_norm(e, train, net, n_pos, u.cin, u.bn_in, a.stat_in));
    RUN(conv_fwd(geom(B, a.h, a.w, u.cin, u.cout, 3, 3, 1), net, W + u.ca_w, W + u.ca_b, u.cout, a.stat_in,
                 EPI_BIAS, nullptr, 0, 0, a.t1, s));
    CHK(batch_norm(e, train, a.t1, n_pos, u.cout, u.bn_mid, a.stat_mid));
    const OdbConv g2 = geom(B, a.h, a.w, u.cout, u.cout, 4, 1, 1);
    if (u.pool) {
      RUN(conv_fwd(g2, a.t1, W + u.cb_w, W + u.cb_b, u.cout, a.stat_mid, EPI_BIAS, nullptr, 0, 0, a.t2, s));
      if (train) RUN(odb_pool_winner(a.t2, a.idx, B, a.h, a.w, u.cout, s));
      RUN(conv_fwd(geom(B, a.h, a.w, u.cin, u.cout, 1, 1, 2), net, W + u.sc_w, W + u.sc_b, u.cout, nullptr,
                   EPI_ADD_POOL, a.t2, a.h, a.w, a.out, s));
    } else {
      RUN(conv_fwd(g2, a.t1, W + u.cb_w, W + u.cb_b, u.cout, a.stat_mid, EPI_ADD, net, 0, 0, a.out, s));
    }
    net = a.out;
  }
  RUN(odb_mean_h(net, e.seq, B, e.hl, e.T, C, s));
  e.lstm.B = B;
  RUN(sib_lstm_fwd(e.lstm, s));
  RUN(odb_head_loss(head_args(e, B, train ? e.mb : nullptr, train ? e.dzh : nullptr, acc, e.auc ? e.probs : nullptr),
                    s));
  // Keras accumulates a metric over the batches of an epoch: the training-mode outputs, then the validation's
  if (e.auc) RUN(odb_auc_count(e.probs, e.lb, B, e.K, e.thr, 1, e.auc_n + (train ? 0 : ODB_AUC_COUNTS), s));
  return MMLA_OK;
}

// the gradient of the batch-mean loss at every trainable tensor -> G, after forward(train)
int backward(Engine& e, int B) {
  hipStream_t s = e.c->stream;
  const float* W = e.W;
  float* G = e.G;
  RUN(odb_head_bwd(head_args(e, B, e.mb, e.dzh, nullptr, nullptr), G + e.off.dw, G + e.off.db, e.demb, s));
  RUN(sib_lstm_bwd(e.lstm, s));
  float *cur = e.gbuf[0], *f1 = e.gbuf[1], *f2 = e.gbuf[2];
  RUN(odb_mean_h_bwd(e.lstm.dxs, cur, B, e.hl, e.T, C, s));
  for (int i = 8; i >= 0; --i) {
    const BlkOff& u = e.off.u[i];
    const BlkAct& a = e.ba[i];
    const float* inp = i ? e.ba[i - 1].out : e.net0;
    const int64_t n_in = (int64_t)B * a.h * a.w, n_out = (int64_t)B * a.ho * a.wo;
    const OdbConv g1 = geom(B, a.h, a.w, u.cin, u.cout, 3, 3, 1), g2 = geom(B, a.h, a.w, u.cout, u.cout, 4, 1, 1);
    const float* dt2 = cur;
    if (u.pool) {   // cur = d(shortcut) = d(pooled t2)
      const OdbConv gs = geom(B, a.h, a.w, u.cin, u.cout, 1, 1, 2);
      RUN(odb_conv_wgrad(gs, inp, nullptr, nullptr, cur, e.part, G + u.sc_w, s));
      RUN(odb_bias_grad(cur, n_out, u.cout, e.part, G + u.sc_b, s));
      RUN(odb_pool_bwd(cur, a.idx, f1, B, a.h, a.w, u.cout, s));
      dt2 = f1;
    }
    RUN(odb_conv_wgrad(g2, a.t1, a.stat_mid + 2 * C, a.stat_mid + 3 * C, dt2, e.part, G + u.cb_w, s));
    RUN(odb_bias_grad(dt2, n_in, u.cout, e.part, G + u.cb_b, s));
    CHK(conv_bwd_data(e, g2, W + u.cb_w, dt2, f2));
    RUN(odb_bn_elu_bwd(a.t1, f2, n_in, u.cout, a.stat_mid, e.part, nullptr, f1, G + u.bn_mid, s));
    RUN(odb_conv_wgrad(g1, inp, a.stat_in + 2 * C, a.stat_in + 3 * C, f1, e.part, G + u.ca_w, s));
    RUN(odb_bias_grad(f1, n_in, u.cout, e.part, G + u.ca_b, s));
    CHK(conv_bwd_data(e, g1, W + u.ca_w, f1, f2));
    if (!u.pool) {   // d net = d out (the identity shortcut) + the main path's, in place
      RUN(odb_bn_elu_bwd(inp, f2, n_in, u.cin, a.stat_in, e.part, cur, cur, G + u.bn_in, s));
      continue;
    }
    const OdbConv gs = geom(B, a.h, a.w, u.cin, u.cout, 1, 1, 2);
    const int cp = pad32(u.cin);
    RUN(odb_conv_transpose(gs, cp, W + u.sc_w, e.wt, s));
    RUN(odb_shortcut_bwd_data(gs, cp, cur, e.wt, f1, s));
    RUN(odb_bn_elu_bwd(inp, f2, n_in, u.cin, a.stat_in, e.part, f1, f1, G + u.bn_in, s));
    std::swap(cur, f1);
  }
  const OdbConv g0 = geom(B, e.h, e.w, e.ch, 16, 1, 1, 1);   // [ch, 16]: 16 entries for a one-channel stem
  RUN(odb_conv_wgrad(g0, e.xb, nullptr, nullptr, cur, e.part, G + e.off.stem_w, s));
  RUN(odb_bias_grad(cur, (int64_t)B * e.h * e.w, 16, e.part, G + e.off.stem_b, s));
  return MMLA_OK;
}

// the classes of a blob of n_floats (body + 513 K, 32 fewer for a one-channel stem: no two layouts share a
// size) and its channels into *ch, or 0
int blob_classes(int64_t n_floats, int* ch) {
  for (int c : {3, 1}) {
    const int64_t head = n_floats - od_body_floats() + (c == 1 ? 32 : 0);
    if (head >= 513 * 2 && head <= 513 * (int64_t)MMLA_OD_MAX_CLASSES && head % 513 == 0) {
      *ch = c;
      return (int)(head / 513);
    }
  }
  return 0;
}

// *K, *ch: the blob's classes and channels
int check_common(mmla_ctx* c, const char* who, int64_t n_floats, int32_t h, int32_t w, const float* class_w, int* K,
                 int* ch) {
  *K = blob_classes(n_floats, ch);
  if (!*K)
    return fail(c, MMLA_E_INVALID, "%s: n_floats %lld, the OD blob has %lld + 513 K with K in [2, %d] (32 fewer "
                "with a one-channel stem)", who, (long long)n_floats, (long long)od_body_floats(), MMLA_OD_MAX_CLASSES);
  if (h < kMinH || h > kMaxH || w < kMinW || w > kMaxW)
    return fail(c, MMLA_E_INVALID, "%s: image %d x %d outside [%d, %d] x [%d, %d]", who, h, w, kMinH, kMaxH, kMinW,
                kMaxW);
  if (!class_w) return fail(c, MMLA_E_INVALID, "%s: null pointer", who);
  for (int k = 0; k < *K; ++k)
    if (!std::isfinite(class_w[k]) || class_w[k] < 0.0f)
      return fail(c, MMLA_E_INVALID, "%s: class_w[%d] = %g is negative or not finite", who, k, class_w[k]);
  return MMLA_OK;
}

// how check_labels names the labels of K classes (null: "[0, K)")
const char* label_set(int K) { return K == 2 ? "{0, 1}" : nullptr; }

int prepare(Engine& e, bool train) {
  hipStream_t s = e.c->stream;
  const size_t wbytes = e.off.total * sizeof(float);
  HIPCHK(e.c, hipMemsetAsync(e.G, 0, wbytes, s));   // the moving-statistics slots stay 0
  HIPCHK(e.c, hipMemsetAsync(e.zero, 0, C * sizeof(float), s));
  HIPCHK(e.c, hipMemsetAsync(e.st, 0, SIB_ST * sizeof(double), s));
  if (e.auc) HIPCHK(e.c, hipMemsetAsync(e.auc_n, 0, 2 * ODB_AUC_COUNTS * sizeof(uint32_t), s));
  if (!train) return MMLA_OK;
  HIPCHK(e.c, hipMemsetAsync(e.acc_g, 0, wbytes, s));   // a new optimiser: every accumulator from 0
  HIPCHK(e.c, hipMemsetAsync(e.acc_d, 0, wbytes, s));
  return mark_trainable(e.c, e.trainable, e.off);
}

// the engine of a checked call: the blob's size, the class weights, every block's dimensions
Engine engine(mmla_ctx* c, int K, int ch, int cap, int h, int w, const float* class_w) {
  Engine e;
  e.c = c;
  e.cap = cap;
  e.K = K;
  e.ch = ch;
  e.off = od_offsets(K, ch);
  for (int k = 0; k < K; ++k) e.cw[k] = class_w[k];
  set_dims(e, h, w);
  return e;
}

// mmla_od_finetune and, with `scratch`, mmla_od_train: what fit_common.h's driver runs per step.  scratch: the
// keep-bits of every batch are generated on the device from drop_seed (site 2, by training-set row), and the
// AUC of the epoch's training-mode and validation outputs is counted into history columns 5 and 6
int od_fit(mmla_ctx* c, FitCall a, int32_t h, int32_t w, const float* class_w, const float* lr,
           const uint8_t* drop_mask, bool scratch, int64_t drop_seed) {
  if (!c) return MMLA_E_INVALID;
  const char* who = a.who;
  int K = 0, ch = 3;
  CHK(check_common(c, who, (int64_t)a.n_floats, h, w, class_w, &K, &ch));
  const int32_t epochs = a.epochs;
  const int64_t n_train = a.n_train;
  a.unit = "images";
  a.slot = S_ODFT;
  a.max_batch = MMLA_OD_TRAIN_MAX_BATCH;
  a.val_chunk = 16;
  a.n_classes = K;
  a.label_set = label_set(K);
  a.row_bytes = (size_t)h * w * ch;
  // rows after an early stop
  a.nan_fill = [](float* hist, size_t n, hipStream_t s) { return odb_fill(hist, (int64_t)n, __builtin_nanf(""), s); };
  CHK(fit_check(c, a));
  if (epochs > 0 && !lr) return fail(c, MMLA_E_INVALID, "%s: null pointer", who);
  for (int ep = 0; ep < epochs; ++ep)
    if (!std::isfinite(lr[ep]) || lr[ep] < 0.0f)
      return fail(c, MMLA_E_INVALID, "%s: lr[%d] = %g is negative or not finite", who, ep, lr[ep]);
  Engine e = engine(c, K, ch, a.cap(), h, w, class_w);
  e.auc = scratch;
  if (scratch) e.thr = odb_auc_thresholds();
  hipStream_t s = c->stream;
  const int img_bytes = (int)a.row_bytes, n = (int)n_train, nv = (int)a.n_val;
  const float* dlr = nullptr;
  const uint8_t* dmask = nullptr;   // [epochs, n_train, 512], indexed by epoch and sample
  return fit(
      c, a,
      [&](Carver& cv, Stager& st, FitBufs& d) -> int {
        carve(e, cv, true);
        d.blob = e.W;
        CHK(st.up(cv, lr, (size_t)epochs, &dlr));   // a host array in either mode
        CHK(d.stage_in(a, cv, st));
        CHK(st.in(cv, drop_mask, (size_t)epochs * n_train * ODB_HEAD_D, &dmask));
        d.stage_out(a, cv, st);
        return MMLA_OK;
      },
      [&]() -> int { return prepare(e, true); },
      [&](const FitBufs& d, int ep, const int32_t* order, int b0, int nb) -> int {
        const uint8_t* mask = dmask ? dmask + (size_t)ep * n_train * ODB_HEAD_D : nullptr;
        RUN(odb_gather(static_cast<const uint8_t*>(d.x), d.labels, mask, order, b0, nb, n, img_bytes, e.xb, e.lb, e.mb,
                       s));
        if (scratch) {   // the batch's keep-bits over the all-ones the gather left
          RUN(sbb_ids(nullptr, order, b0, nb, n, e.sid, s));
          RUN(odb_drop_mask((uint64_t)drop_seed, (uint32_t)ep, e.sid, nb, e.mb, s));
        }
        CHK(forward(e, nb, true, e.st));
        CHK(backward(e, nb));
        RUN(sib_fold_batch(e.st, nb, s));
        RUN(odb_adadelta(e.W, e.acc_g, e.acc_d, e.G, e.trainable, (int64_t)e.off.total, dlr, ep, s));
        return MMLA_OK;
      },
      [&](const FitBufs& d, int v0, int nb) -> int {
        RUN(odb_gather(static_cast<const uint8_t*>(d.val_x), d.val_labels, nullptr, nullptr, v0, nb, nv, img_bytes,
                       e.xb, e.lb, e.mb, s));
        return forward(e, nb, false, e.st + 5);
      },
      [&](int ep, float* row) -> int {
        RUN(odb_end_epoch(e.st, n, nv, dlr, ep, row, s));
        if (!scratch) return MMLA_OK;
        RUN(odb_auc_final(e.auc_n, 1, n, K, 1, row + 5, s));
        RUN(odb_auc_final(e.auc_n + ODB_AUC_COUNTS, 1, nv, K, 1, row + 6, s));   // NaN when n_val == 0
        return MMLA_OK;
      });
}

}  // namespace
}  // namespace mmla

using namespace mmla;

#undef RUN
#define RUN(expr) HIPCHK(c, (expr))

extern "C" {

int mmla_od_loss_grad(mmla_ctx* c, const float* packed, int64_t n_floats, const uint8_t* img_u8,
                      const int32_t* labels, int64_t n, int32_t h, int32_t w, const float* class_w,
                      const uint8_t* drop_mask, float* loss, float* grad, float* moving_out, uint32_t flags) {
  if (!c) return MMLA_E_INVALID;
  int K = 0, ch = 3;
  CHK(check_common(c, "od_loss_grad", n_floats, h, w, class_w, &K, &ch));
  if (n < 1 || n > MMLA_OD_TRAIN_MAX_BATCH)
    return fail(c, MMLA_E_INVALID, "od_loss_grad: n %lld outside [1, %d]", (long long)n, MMLA_OD_TRAIN_MAX_BATCH);
  if (!packed || !img_u8 || !labels || !loss || !grad) return fail(c, MMLA_E_INVALID, "od_loss_grad: null pointer");
  Stager st{c, (flags & MMLA_DEVICE_PTR) != 0};
  if (!st.dev) CHK(check_labels(c, "labels", labels, n, K, label_set(K)));
  HIPCHK(c, hipSetDevice(c->device));
  Engine e = engine(c, K, ch, (int)n, h, w, class_w);
  const size_t img_bytes = (size_t)h * w * ch;
  float* lp = nullptr;
  const uint8_t *dimg = nullptr, *dmask = nullptr;
  const int32_t* dl = nullptr;
  CHK(carve_slot(c, S_ODFT, [&](Carver& cv) -> int {
    carve(e, cv, false);
    lp = cv.take<float>(1);
    CHK(st.in(cv, img_u8, (size_t)n * img_bytes, &dimg));
    CHK(st.in(cv, labels, (size_t)n, &dl));
    return st.in(cv, drop_mask, (size_t)n * ODB_HEAD_D, &dmask);
  }));
  hipStream_t s = c->stream;
  const size_t wbytes = e.off.total * sizeof(float);
  HIPCHK(c, hipMemcpyAsync(e.W, packed, wbytes, st.kind_in(), s));
  CHK(prepare(e, false));
  RUN(odb_gather(dimg, dl, dmask, nullptr, 0, (int)n, (int)n, (int)img_bytes, e.xb, e.lb, e.mb, s));
  CHK(forward(e, (int)n, true, e.st));
  CHK(backward(e, (int)n));
  RUN(odb_loss_out(e.st, (int)n, lp, s));
  HIPCHK(c, hipMemcpyAsync(grad, e.G, wbytes, st.kind_out(), s));
  HIPCHK(c, hipMemcpyAsync(loss, lp, sizeof(float), st.kind_out(), s));
  // the forward advanced the copy's moving statistics and nothing else of it
  if (moving_out) HIPCHK(c, hipMemcpyAsync(moving_out, e.W, wbytes, st.kind_out(), s));
  return finish(c, st.dev);
}

int mmla_od_finetune(mmla_ctx* c, const float* packed, int64_t n_floats, const uint8_t* img_u8,
                     const int32_t* labels, int64_t n_train, const uint8_t* val_img, const int32_t* val_labels,
                     int64_t n_val, int32_t h, int32_t w, const float* class_w, int32_t epochs, int32_t batch,
                     const float* lr, const int32_t* perm, const uint8_t* drop_mask, int32_t patience,
                     float* packed_out, float* history, int32_t* epochs_run, uint32_t flags) {
  FitCall a = fit_call("od_finetune", packed, n_floats, img_u8, labels, n_train, val_img, val_labels, n_val, epochs,
                       batch, perm, packed_out, history, flags);
  a.hist_w = 5;   // ... and the epoch's lr
  a.callbacks = FIT_STOP;
  a.patience = patience;
  a.epochs_run = epochs_run;
  return od_fit(c, a, h, w, class_w, lr, drop_mask, false, 0);
}

int mmla_od_train(mmla_ctx* c, const float* packed, int64_t n_floats, const uint8_t* img_u8, const int32_t* labels,
                  int64_t n_train, const uint8_t* val_img, const int32_t* val_labels, int64_t n_val, int32_t h,
                  int32_t w, const float* class_w, int32_t epochs, int32_t batch, const float* lr,
                  const int32_t* perm, int64_t drop_seed, int32_t patience, int32_t ckpt_period, float* packed_out,
                  float* best_out, float* history, int32_t* epochs_run, int32_t* best_epoch, uint32_t flags) {
  FitCall a = fit_call("od_train", packed, n_floats, img_u8, labels, n_train, val_img, val_labels, n_val, epochs,
                       batch, perm, packed_out, history, flags);
  a.hist_w = 7;   // ... the epoch's lr, auc, val_auc
  a.callbacks = FIT_STOP | FIT_CKPT;
  a.patience = patience;
  a.ckpt_period = ckpt_period;
  a.best_out = best_out;
  a.epochs_run = epochs_run;
  a.best_epoch = best_epoch;
  return od_fit(c, a, h, w, class_w, lr, nullptr, true, drop_seed);
}

int mmla_od_drop_mask(mmla_ctx* c, int64_t drop_seed, int32_t epoch, const int32_t* sample_ids, int64_t n,
                      uint8_t* mask, uint32_t flags) {
  if (!c) return MMLA_E_INVALID;
  if (n < 1 || n > (1 << 20)) return fail(c, MMLA_E_INVALID, "od_drop_mask: n %lld outside [1, 2^20]", (long long)n);
  if (epoch < 0) return fail(c, MMLA_E_INVALID, "od_drop_mask: epoch %d < 0", epoch);
  if (!mask) return fail(c, MMLA_E_INVALID, "od_drop_mask: null pointer");
  Stager st{c, (flags & MMLA_DEVICE_PTR) != 0};
  if (!st.dev && sample_ids)
    for (int64_t i = 0; i < n; ++i)
      if (sample_ids[i] < 0)
        return fail(c, MMLA_E_INVALID, "od_drop_mask: sample_ids[%lld] = %d < 0", (long long)i, sample_ids[i]);
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  int32_t* sid = nullptr;
  const int32_t* dids = nullptr;
  uint8_t* dm = nullptr;
  CHK(carve_slot(c, S_ODFT, [&](Carver& cv) -> int {
    sid = cv.take<int32_t>(n);
    CHK(st.in(cv, sample_ids, (size_t)n, &dids));
    dm = st.out(cv, mask, (size_t)n * ODB_HEAD_D);
    return MMLA_OK;
  }));
  RUN(sbb_ids(dids, nullptr, 0, (int)n, (int)n, sid, s));
  RUN(odb_drop_mask((uint64_t)drop_seed, (uint32_t)epoch, sid, (int)n, dm, s));
  CHK(st.back(mask, dm, (size_t)n * ODB_HEAD_D));
  return finish(c, st.dev);
}

int mmla_od_auc(mmla_ctx* c, const float* probs, const int32_t* labels, int64_t n, float* auc_out, uint32_t flags) {
  return mmla_od_auc_k(c, probs, labels, n, 2, auc_out, flags);
}

int mmla_od_auc_k(mmla_ctx* c, const float* probs, const int32_t* labels, int64_t n, int32_t n_classes,
                  float* auc_out, uint32_t flags) {
  if (!c) return MMLA_E_INVALID;
  const int K = n_classes;
  if (K < 2 || K > MMLA_OD_MAX_CLASSES)
    return fail(c, MMLA_E_INVALID, "od_auc: n_classes %d outside [2, %d]", K, MMLA_OD_MAX_CLASSES);
  if (n < 1 || n > (1 << 24)) return fail(c, MMLA_E_INVALID, "od_auc: n %lld outside [1, 2^24]", (long long)n);
  if (!probs || !labels || !auc_out) return fail(c, MMLA_E_INVALID, "od_auc: null pointer");
  Stager st{c, (flags & MMLA_DEVICE_PTR) != 0};
  if (!st.dev) CHK(check_labels(c, "labels", labels, n, K, label_set(K)));
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const int S = odb_auc_slabs(n);
  const float* dp = nullptr;
  const int32_t* dl = nullptr;
  uint32_t* counts = nullptr;
  float* da = nullptr;
  CHK(carve_slot(c, S_ODFT, [&](Carver& cv) -> int {
    counts = cv.take<uint32_t>((size_t)S * ODB_AUC_COUNTS);
    CHK(st.in(cv, probs, (size_t)n * K, &dp));
    CHK(st.in(cv, labels, (size_t)n, &dl));
    da = st.out(cv, auc_out, 1);
    return MMLA_OK;
  }));
  RUN(odb_auc_count(dp, dl, n, K, odb_auc_thresholds(), 0, counts, s));
  RUN(odb_auc_final(counts, S, n, K, 0, da, s));
  CHK(st.back(auc_out, da, 1));
  return finish(c, st.dev);
}

int mmla_od_augment(mmla_ctx* c, const uint8_t* img, int64_t n, int32_t h, int32_t w, const int32_t* src,
                    const int32_t* levels, int64_t m, uint8_t* out, uint32_t flags) {
  if (!c) return MMLA_E_INVALID;
  if (h < ODA_MIN_H || h > ODA_MAX_H || h % 2)
    return fail(c, MMLA_E_INVALID, "od_augment: h %d is not an even size in [%d, %d]", h, ODA_MIN_H, ODA_MAX_H);
  if (w < ODA_MIN_W || w > ODA_MAX_W || w % 2 == 0)
    return fail(c, MMLA_E_INVALID, "od_augment: w %d is not an odd size in [%d, %d]", w, ODA_MIN_W, ODA_MAX_W);
  if (n < 1 || n > (1 << 24)) return fail(c, MMLA_E_INVALID, "od_augment: n %lld outside [1, 2^24]", (long long)n);
  if (m < 0 || m > (1 << 24)) return fail(c, MMLA_E_INVALID, "od_augment: m %lld outside [0, 2^24]", (long long)m);
  if (!img || (m > 0 && (!src || !levels || !out))) return fail(c, MMLA_E_INVALID, "od_augment: null pointer");
  Stager st{c, (flags & MMLA_DEVICE_PTR) != 0};
  if (!st.dev)
    for (int64_t k = 0; k < m; ++k) {
      if (src[k] < 0 || src[k] >= n)
        return fail(c, MMLA_E_INVALID, "od_augment: src[%lld] = %d outside [0, %lld)", (long long)k, src[k],
                    (long long)n);
      if (levels[k] < 0 || levels[k] > MMLA_OD_AUG_MAX_LEVELS)
        return fail(c, MMLA_E_INVALID, "od_augment: levels[%lld] = %d outside [0, %d]", (long long)k, levels[k],
                    MMLA_OD_AUG_MAX_LEVELS);
    }
  if (m == 0) return MMLA_OK;
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const size_t img_bytes = (size_t)h * w * 3;
  const uint8_t* di = nullptr;
  const int32_t *ds = nullptr, *dl = nullptr;
  uint8_t* dout = nullptr;
  CHK(carve_slot(c, S_ODFT, [&](Carver& cv) -> int {
    CHK(st.in(cv, img, (size_t)n * img_bytes, &di));
    CHK(st.in(cv, src, (size_t)m, &ds));
    CHK(st.in(cv, levels, (size_t)m, &dl));
    dout = st.out(cv, out, (size_t)m * img_bytes);
    return MMLA_OK;
  }));
  RUN(oda_augment(di, n, h, w, ds, dl, m, dout, s));
  CHK(st.back(out, dout, (size_t)m * img_bytes));
  return finish(c, st.dev);
}

}  // extern "C"
