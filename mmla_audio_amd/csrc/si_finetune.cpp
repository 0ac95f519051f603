// libmmla: speaker registration stage 2 -- mmla_si_loss_grad and mmla_si_finetune -- and training the SI base
// model from scratch -- mmla_si_base_drop_mask, mmla_si_base_loss_grad, mmla_si_base_train (include/mmla.h):
// the same engine with `base` set, which swaps in si_base.hip's training-mode layers.
// Which kernel of si_bwd.hip runs which layer, forward and backward, over a copy of the packed SI blob
// in workspace slot S_FT; the context's loaded model is not touched.  A training step is a fixed
// sequence of launches on the context's stream with no host synchronisation: the loss bookkeeping
// lives in device memory and the history is read once at the end of the fit.  The fit itself -- checks,
// staging, the epoch loop, the callbacks -- is fit_common.h's driver; this file gives it the steps.
#include <algorithm>
#include <cmath>

#include "fit_common.h"
#include "internal.h"
#include "si_base.h"
#include "si_bwd.h"

namespace mmla {
namespace {

constexpr int kMaxPass = 4096;   // windows per forward / backward pass

// offsets (in floats) of the tensors of weights.si_spec(K) in the packed blob
struct UnitOff {
  size_t bn_in, ca_w, ca_b, bn_mid, sc_w, sc_b, cb_w, cb_b;
  int cin, cout;
  bool pool;
};
struct SiOff {
  size_t stem_w, stem_b;
  UnitOff u[9];
  size_t fbn, lk[2], lr[2], lb[2], dw, db, total;
};

SiOff si_offsets(int K) {
  SiOff o{};
  size_t at = 0;
  auto take = [&](size_t n) {
    const size_t r = at;
    at += n;
    return r;
  };
  o.stem_w = take(4 * SI_D * 32);
  o.stem_b = take(32);
  int cin = 32;
  for (int i = 0; i < 9; ++i) {
    UnitOff& u = o.u[i];
    u.cin = cin;
    u.cout = CH[i];
    u.pool = POOL[i];
    u.bn_in = take(4 * (size_t)cin);
    u.ca_w = take(3 * (size_t)cin * u.cout);
    u.ca_b = take(u.cout);
    u.bn_mid = take(4 * (size_t)u.cout);
    if (u.pool) {
      u.sc_w = take((size_t)cin * u.cout);
      u.sc_b = take(u.cout);
    }
    u.cb_w = take(3 * (size_t)u.cout * u.cout);
    u.cb_b = take(u.cout);
    cin = u.cout;
  }
  o.fbn = take(4 * 128);
  for (int d = 0; d < 2; ++d) {
    o.lk[d] = take((size_t)SIB_LSTM_D * SIB_LSTM_G);
    o.lr[d] = take((size_t)SIB_LSTM_U * SIB_LSTM_G);
    o.lb[d] = take(SIB_LSTM_G);
  }
  o.dw = take((size_t)MMLA_SI_EMBED * K);
  o.db = take(K);
  o.total = at;
  return o;
}

// kernel_regularizer=l2(.) of res_model's units 5, 6 (0.1) and 8, 9 (0.2), speaker_identification.py:175-206
float unit_l2(int i) { return i == 4 || i == 5 ? 0.1f : i == 7 || i == 8 ? 0.2f : 0.0f; }

struct UnitAct {
  float *inp, *a1, *o1, *a2, *out;
  uint8_t* idx;
};

// one training engine over a carved workspace: capacity `cap` windows per pass
struct Engine {
  mmla_ctx* c = nullptr;
  SiOff off;
  int K = 0, cap = 0;
  float *W = nullptr, *G = nullptr, *rms = nullptr, *wt = nullptr;
  uint8_t* mask = nullptr;
  double* st = nullptr;
  float *xb = nullptr, *net0 = nullptr, *fin = nullptr, *seq = nullptr, *emb = nullptr, *dzh = nullptr,
        *demb = nullptr;
  int32_t* lb = nullptr;
  UnitAct ua[9];
  float* gbuf[3] = {nullptr, nullptr, nullptr};
  SibLstm lstm{};
  // training a base model from scratch (mmla_si_base_*, si_base.hip): BatchNorm on batch statistics,
  // dropout and the wide softmax head in training passes; the wide head alone in validation passes
  bool base = false;
  SbbDrop drop{};
  float *dbnoise = nullptr, *bstat = nullptr, *part = nullptr, *embd = nullptr, *dmul = nullptr, *hloss = nullptr;
  int32_t *sid = nullptr, *hhit = nullptr;
};
constexpr int kBnSites = 19;   // bn_in, bn_mid of the nine units, then the final one

// the engine's buffers; the pass on a null base only measures (fit_common.h)
void carve(Engine& e, Carver& cv, bool train) {
  const size_t B = e.cap, n = e.off.total;
  e.W = cv.take<float>(n);
  e.G = cv.take<float>(n);
  e.rms = train ? cv.take<float>(n) : nullptr;
  e.mask = train ? cv.take<uint8_t>(n) : nullptr;
  e.wt = cv.take<float>(3 * 128 * 128);
  e.st = cv.take<double>(SIB_ST);
  e.xb = cv.take<float>(B * SI_T * SI_D);
  e.lb = cv.take<int32_t>(B);
  e.net0 = cv.take<float>(B * SI_T * 32);
  int T = SI_T;
  for (int i = 0; i < 9; ++i) {
    const UnitOff& u = e.off.u[i];
    UnitAct& a = e.ua[i];
    if (u.pool) T /= 2;
    a.inp = u.pool ? cv.take<float>(B * T * u.cin) : nullptr;
    a.idx = u.pool ? cv.take<uint8_t>(B * T * u.cin) : nullptr;
    a.a1 = cv.take<float>(B * T * u.cin);
    a.o1 = cv.take<float>(B * T * u.cout);
    a.a2 = cv.take<float>(B * T * u.cout);
    a.out = cv.take<float>(B * T * u.cout);
  }
  e.fin = cv.take<float>(B * 32 * 128);
  e.seq = cv.take<float>(B * SIB_LSTM_T * SIB_LSTM_D);
  e.emb = cv.take<float>(B * MMLA_SI_EMBED);
  e.dzh = cv.take<float>(B * (size_t)std::max(e.K, MMLA_SI_TRAIN_MAX_CLASSES));
  e.demb = cv.take<float>(B * MMLA_SI_EMBED);
  for (int q = 0; q < 3; ++q) e.gbuf[q] = cv.take<float>(B * SI_T * 32);
  SibLstm& l = e.lstm;
  l.gates = cv.take<float>(2 * SIB_LSTM_T * B * SIB_LSTM_G);
  l.cs = cv.take<float>(2 * SIB_LSTM_T * B * SIB_LSTM_U);
  l.hs = cv.take<float>(2 * SIB_LSTM_T * B * SIB_LSTM_U);
  l.dz = cv.take<float>(2 * SIB_LSTM_T * B * SIB_LSTM_G);
  l.dh = cv.take<float>(2 * B * SIB_LSTM_U);
  l.dc = cv.take<float>(2 * B * SIB_LSTM_U);
  l.dxs = cv.take<float>(2 * B * SIB_LSTM_T * SIB_LSTM_D);
  if (e.base) {
    e.bstat = cv.take<float>((size_t)kBnSites * SBB_STAT);
    e.part = cv.take<float>(SBB_PART);
    e.embd = cv.take<float>(B * MMLA_SI_EMBED);
    e.dmul = cv.take<float>(B * MMLA_SI_EMBED);
    e.hloss = cv.take<float>(B);
    e.hhit = cv.take<int32_t>(B);
    e.sid = cv.take<int32_t>(B);
    e.dbnoise = cv.take<float>(SBB_MAX_C);
  }
  if (cv.base) {
    wire_lstm(l, e.off, e.W, e.G);
    l.seq = e.seq;
    l.T = SIB_LSTM_T;
    l.emb = e.emb;
    l.demb = e.demb;
  }
}

SibConv geom(int B, int tin, int cin, int cout, int k, int stride) {
  const int tout = (tin + stride - 1) / stride;
  const int tot = std::max((tout - 1) * stride + k - tin, 0);   // Keras 'same': the smaller half first
  return SibConv{B, tin, tout, cin, cout, k, stride, tot / 2};
}

#define RUN(expr) HIPCHK(e.c, (expr))

// BN + ReLU of site `site`: on the moving statistics, or (a training pass of a base fit) on the batch's
int bn_fwd(Engine& e, int site, const float* x, size_t bn, float* y, int n_pos, int ch, bool train) {
  hipStream_t s = e.c->stream;
  if (e.base && train)
    RUN(sbb_bn_relu_fwd(x, e.W + bn, y, n_pos, ch, e.bstat + (size_t)site * SBB_STAT, e.part, s));
  else
    RUN(sib_bn_relu_fwd(x, e.W + bn, y, n_pos, ch, s));
  return MMLA_OK;
}

int bn_bwd(Engine& e, int site, const float* x, const float* y, const float* dy, size_t bn, const float* add,
           float* dx, int n_pos, int ch) {
  hipStream_t s = e.c->stream;
  if (e.base)
    RUN(sbb_bn_relu_bwd(x, y, dy, e.W + bn, e.bstat + (size_t)site * SBB_STAT, e.part, add, dx, e.G + bn, n_pos,
                        ch, s));
  else
    RUN(sib_bn_relu_bwd(x, y, dy, e.W + bn, add, dx, e.G + bn, n_pos, ch, s));
  return MMLA_OK;
}

SbbHead base_head(Engine& e, int B, double* acc, bool train, float bsz) {
  return SbbHead{e.emb,   e.W + e.off.dw, e.W + e.off.db, e.lb, e.embd, e.dmul, train ? e.dzh : nullptr,
                 e.hloss, e.hhit,         acc,            B,    e.K,    bsz,    train ? 1 : 0};
}

// forward of the B windows in xb / lb; acc: where the loss sum and the hits are added; train: keep dz
int forward(Engine& e, int B, double* acc, bool train, float bsz) {
  hipStream_t s = e.c->stream;
  const float* W = e.W;
  RUN(sib_conv_fwd(geom(B, SI_T, SI_D, 32, 4, 1), e.xb, W + e.off.stem_w, W + e.off.stem_b, nullptr, e.net0, s));
  const float* net = e.net0;
  int T = SI_T;
  for (int i = 0; i < 9; ++i) {
    const UnitOff& u = e.off.u[i];
    const UnitAct& a = e.ua[i];
    const int Tin = T;
    const float* inp = net;
    if (u.pool) {
      T /= 2;
      RUN(sib_maxpool_fwd(net, a.inp, a.idx, B, T, u.cin, s));
      inp = a.inp;
    }
    CHK(bn_fwd(e, 2 * i, inp, u.bn_in, a.a1, B * T, u.cin, train));
    RUN(sib_conv_fwd(geom(B, T, u.cin, u.cout, 3, 1), a.a1, W + u.ca_w, W + u.ca_b, nullptr, a.o1, s));
    CHK(bn_fwd(e, 2 * i + 1, a.o1, u.bn_mid, a.a2, B * T, u.cout, train));
    const float* res = net;
    if (u.pool) {
      RUN(sib_conv_fwd(geom(B, Tin, u.cin, u.cout, 1, 2), net, W + u.sc_w, W + u.sc_b, nullptr, a.out, s));
      res = a.out;
    }
    RUN(sib_conv_fwd(geom(B, T, u.cout, u.cout, 3, 1), a.a2, W + u.cb_w, W + u.cb_b, res, a.out, s));
    net = a.out;
  }
  CHK(bn_fwd(e, 18, net, e.off.fbn, e.fin, B * T, 128, train));
  if (e.base && train)
    RUN(sbb_drop_avgpool4_fwd(e.fin, e.seq, B, e.drop, s));
  else
    RUN(sib_avgpool4_fwd(e.fin, e.seq, B, SIB_LSTM_T, 128, s));
  e.lstm.B = B;
  RUN(sib_lstm_fwd(e.lstm, s));
  if (e.base) {
    RUN(sbb_head_loss(base_head(e, B, acc, train, bsz), e.drop, s));
    return MMLA_OK;
  }
  SibHead h{e.emb, W + e.off.dw, W + e.off.db, e.lb, train ? e.dzh : nullptr, acc, B, e.K, bsz};
  RUN(sib_head_loss(h, s));
  return MMLA_OK;
}

int l2_term(Engine& e) {
  SibL2 a{};
  for (int i = 0; i < 9; ++i) {
    const float lam = unit_l2(i);
    if (lam == 0.0f) continue;
    const UnitOff& u = e.off.u[i];
    a.w[a.n_t] = e.W + u.ca_w;
    a.n[a.n_t] = 3 * u.cin * u.cout;
    a.lambda[a.n_t++] = lam;
    a.w[a.n_t] = e.W + u.cb_w;
    a.n[a.n_t] = 3 * u.cout * u.cout;
    a.lambda[a.n_t++] = lam;
  }
  RUN(sib_l2(a, e.st + 2, e.c->stream));
  return MMLA_OK;
}

// the gradient of (batch-mean data term + R) at every trainable tensor -> G, after forward(train)
int backward(Engine& e, int B) {
  hipStream_t s = e.c->stream;
  const float* W = e.W;
  float* G = e.G;
  // A base fit: every Conv1D output reaches the loss only through batch-statistics BNs (directly, or along
  // the residual stream through max-pools and the unpadded 1 x 1 shortcuts, which all carry a per-channel
  // constant unchanged), so the gradient of a Conv1D bias is identically zero.  What the kernels sum there
  // is rounding noise, which RMSprop would turn into steps of +-3.16 lr: it goes to a scratch row and the
  // slot of G keeps its exact 0.
  auto db = [&](size_t bias) { return e.base ? e.dbnoise : G + bias; };
  if (e.base) {
    RUN(sbb_head_bwd(base_head(e, B, nullptr, true, 1.0f), G + e.off.dw, G + e.off.db, e.demb, s));
  } else {
    SibHead h{e.emb, W + e.off.dw, W + e.off.db, e.lb, e.dzh, nullptr, B, e.K, 1.0f};
    RUN(sib_head_bwd(h, G + e.off.dw, G + e.off.db, e.demb, s));
  }
  RUN(sib_lstm_bwd(e.lstm, s));
  float *cur = e.gbuf[0], *f1 = e.gbuf[1], *f2 = e.gbuf[2];
  if (e.base)
    RUN(sbb_drop_avgpool4_bwd(e.lstm.dxs, f1, B, e.drop, s));
  else
    RUN(sib_avgpool4_bwd(e.lstm.dxs, f1, B, s));
  CHK(bn_bwd(e, 18, e.ua[8].out, e.fin, f1, e.off.fbn, nullptr, cur, B * 32, 128));
  int T = 32;
  for (int i = 8; i >= 0; --i) {
    const UnitOff& u = e.off.u[i];
    const UnitAct& a = e.ua[i];
    const float* net_in = i ? e.ua[i - 1].out : e.net0;
    const float l2x2 = 2.0f * unit_l2(i);
    const SibConv gb = geom(B, T, u.cout, u.cout, 3, 1), ga = geom(B, T, u.cin, u.cout, 3, 1);
    RUN(sib_conv_bwd_weight(gb, a.a2, cur, W + u.cb_w, l2x2, G + u.cb_w, db(u.cb_b), s));
    RUN(sib_conv_transpose(gb, W + u.cb_w, e.wt, s));
    RUN(sib_conv_bwd_data(gb, cur, e.wt, nullptr, f1, s));
    CHK(bn_bwd(e, 2 * i + 1, a.o1, a.a2, f1, u.bn_mid, nullptr, f2, B * T, u.cout));
    RUN(sib_conv_bwd_weight(ga, a.a1, f2, W + u.ca_w, l2x2, G + u.ca_w, db(u.ca_b), s));
    RUN(sib_conv_transpose(ga, W + u.ca_w, e.wt, s));
    RUN(sib_conv_bwd_data(ga, f2, e.wt, nullptr, f1, s));
    if (!u.pool) {   // d net = d out (the identity shortcut) + the main path's, in place
      CHK(bn_bwd(e, 2 * i, net_in, a.a1, f1, u.bn_in, cur, cur, B * T, u.cin));
      continue;
    }
    CHK(bn_bwd(e, 2 * i, a.inp, a.a1, f1, u.bn_in, nullptr, f2, B * T, u.cin));
    RUN(sib_maxpool_bwd(f2, a.idx, f1, B, T, u.cin, s));
    const SibConv gs = geom(B, 2 * T, u.cin, u.cout, 1, 2);
    RUN(sib_conv_bwd_weight(gs, net_in, cur, W + u.sc_w, 0.0f, G + u.sc_w, db(u.sc_b), s));
    RUN(sib_conv_transpose(gs, W + u.sc_w, e.wt, s));
    RUN(sib_conv_bwd_data(gs, cur, e.wt, f1, f1, s));
    std::swap(cur, f1);
    T *= 2;
  }
  RUN(sib_conv_bwd_weight(geom(B, SI_T, SI_D, 32, 4, 1), e.xb, cur, W + e.off.stem_w, 0.0f, G + e.off.stem_w,
                          db(e.off.stem_b), s));
  return MMLA_OK;
}

int check_common(mmla_ctx* c, const char* who, int64_t n_floats, int32_t K,
                 int k_max = MMLA_SI_TRAIN_MAX_CLASSES) {
  if (K < 1 || K > k_max) return fail(c, MMLA_E_INVALID, "%s: n_classes %d outside [1, %d]", who, K, k_max);
  const int64_t want = (int64_t)si_offsets(K).total;
  if (n_floats != want)
    return fail(c, MMLA_E_INVALID, "%s: n_floats %lld, the SI blob with a %d-way head has %lld", who,
                (long long)n_floats, K, (long long)want);
  return MMLA_OK;
}

// sample ids are rows of the training set: none negative (host pointers)
int check_ids(mmla_ctx* c, const char* who, const int32_t* ids, int64_t n) {
  for (int64_t i = 0; ids && i < n; ++i)
    if (ids[i] < 0) return fail(c, MMLA_E_INVALID, "%s: sample_ids[%lld] = %d < 0", who, (long long)i, ids[i]);
  return MMLA_OK;
}

// loss and gradient of the B windows in xb / lb: the data term's sums -> st, R -> st + 2, the gradient -> G
int train_pass(Engine& e, int B) {
  CHK(forward(e, B, e.st, true, (float)B));
  CHK(l2_term(e));
  return backward(e, B);
}

// mmla_si_loss_grad and, with `base`, mmla_si_base_loss_grad
int loss_grad(mmla_ctx* c, const char* who, bool base, int k_max, const float* packed, int64_t n_floats, int32_t K,
              const float* x, const int32_t* labels, int64_t n, int64_t drop_seed, int32_t epoch,
              const int32_t* sample_ids, float* loss, float* grad, float* moving_out, uint32_t flags) {
  if (!c) return MMLA_E_INVALID;
  CHK(check_common(c, who, n_floats, K, k_max));
  if (n < 1 || n > kMaxPass) return fail(c, MMLA_E_INVALID, "%s: n %lld outside [1, %d]", who, (long long)n, kMaxPass);
  if (epoch < 0) return fail(c, MMLA_E_INVALID, "%s: epoch %d < 0", who, epoch);
  if (!packed || !x || !labels || !loss || !grad) return fail(c, MMLA_E_INVALID, "%s: null pointer", who);
  Stager st{c, (flags & MMLA_DEVICE_PTR) != 0};
  if (!st.dev) {
    CHK(check_labels(c, "labels", labels, n, K));
    CHK(check_ids(c, who, sample_ids, n));
  }
  HIPCHK(c, hipSetDevice(c->device));
  Engine e;
  e.c = c;
  e.K = K;
  e.cap = (int)n;
  e.base = base;
  e.off = si_offsets(K);
  float* lp = nullptr;
  int32_t* ids = nullptr;
  CHK(carve_slot(c, S_FT, [&](Carver& cv) -> int {
    carve(e, cv, false);
    lp = cv.take<float>(2);
    if (base) ids = cv.take<int32_t>(n);
    return MMLA_OK;
  }));
  hipStream_t s = c->stream;
  const size_t wbytes = e.off.total * sizeof(float), xbytes = (size_t)n * SI_T * SI_D * sizeof(float);
  HIPCHK(c, hipMemcpyAsync(e.W, packed, wbytes, st.kind_in(), s));
  HIPCHK(c, hipMemcpyAsync(e.xb, x, xbytes, st.kind_in(), s));
  HIPCHK(c, hipMemcpyAsync(e.lb, labels, (size_t)n * sizeof(int32_t), st.kind_in(), s));
  if (base) {
    if (sample_ids) HIPCHK(c, hipMemcpyAsync(ids, sample_ids, (size_t)n * sizeof(int32_t), st.kind_in(), s));
    HIPCHK(c, sbb_ids(sample_ids ? ids : nullptr, nullptr, 0, (int)n, (int)n, e.sid, s));
    e.drop = SbbDrop{(uint64_t)drop_seed, (uint32_t)epoch, e.sid};
  }
  HIPCHK(c, hipMemsetAsync(e.G, 0, wbytes, s));   // the moving-statistics slots stay 0
  HIPCHK(c, hipMemsetAsync(e.st, 0, SIB_ST * sizeof(double), s));
  CHK(train_pass(e, (int)n));
  HIPCHK(c, sib_loss_pair(e.st, (int)n, lp, s));
  HIPCHK(c, hipMemcpyAsync(grad, e.G, wbytes, st.kind_out(), s));
  HIPCHK(c, hipMemcpyAsync(loss, lp, 2 * sizeof(float), st.kind_out(), s));
  // a base model's forward advanced the copy's moving statistics and nothing else of it
  if (moving_out) HIPCHK(c, hipMemcpyAsync(moving_out, e.W, wbytes, st.kind_out(), s));
  return finish(c, st.dev);
}

// mmla_si_finetune and, with `base`, mmla_si_base_train: what fit_common.h's driver runs per step
int si_fit(mmla_ctx* c, FitCall a, bool base, int k_max, float lr, int64_t drop_seed) {
  if (!c) return MMLA_E_INVALID;
  CHK(check_common(c, a.who, (int64_t)a.n_floats, a.n_classes, k_max));
  a.unit = "windows";
  a.slot = S_FT;
  a.max_batch = kMaxPass;
  a.val_chunk = 64;
  a.hist_w = 4;
  a.row_bytes = (size_t)SI_T * SI_D * sizeof(float);
  CHK(fit_check(c, a));
  if (base && (!(lr >= 0.0f) || !std::isfinite(lr)))
    return fail(c, MMLA_E_INVALID, "%s: lr %g is negative or not finite", a.who, lr);
  Engine e;
  e.c = c;
  e.K = a.n_classes;
  e.base = base;
  e.off = si_offsets(e.K);
  e.cap = a.cap();
  hipStream_t s = c->stream;
  const size_t wbytes = e.off.total * sizeof(float);
  const int row = SI_T * SI_D, n = (int)a.n_train, nv = (int)a.n_val;
  return fit(
      c, a,
      [&](Carver& cv, Stager& st, FitBufs& d) -> int {
        carve(e, cv, true);
        d.blob = e.W;
        CHK(d.stage_in(a, cv, st));
        d.stage_out(a, cv, st);
        return MMLA_OK;
      },
      [&]() -> int {
        HIPCHK(c, hipMemsetAsync(e.G, 0, wbytes, s));     // the moving-statistics slots stay 0
        HIPCHK(c, hipMemsetAsync(e.rms, 0, wbytes, s));   // a new optimiser: every accumulator from 0
        HIPCHK(c, hipMemsetAsync(e.st, 0, SIB_ST * sizeof(double), s));
        CHK(mark_trainable(c, e.mask, e.off));
        return freeze_bn(c, e.mask, e.off.fbn, 128);
      },
      [&](const FitBufs& d, int ep, const int32_t* order, int b0, int nb) -> int {
        HIPCHK(c, sib_gather(static_cast<const float*>(d.x), d.labels, order, b0, nb, n, row, e.xb, e.lb, s));
        if (base) {
          HIPCHK(c, sbb_ids(nullptr, order, b0, nb, n, e.sid, s));
          e.drop = SbbDrop{(uint64_t)drop_seed, (uint32_t)ep, e.sid};
        }
        CHK(train_pass(e, nb));
        HIPCHK(c, sib_fold_batch(e.st, nb, s));
        HIPCHK(c, sib_rmsprop(e.W, e.rms, e.G, e.mask, (int64_t)e.off.total, lr, s));
        return b0 + nb == n ? l2_term(e) : MMLA_OK;   // R of the epoch's last weights, for its history row
      },
      [&](const FitBufs& d, int v0, int nb) -> int {
        HIPCHK(c, sib_gather(static_cast<const float*>(d.val_x), d.val_labels, nullptr, v0, nb, nv, row, e.xb, e.lb, s));
        return forward(e, nb, e.st + 5, false, 1.0f);
      },
      [&](int, float* hrow) -> int {
        HIPCHK(c, sib_end_epoch(e.st, n, nv, hrow, s));
        return MMLA_OK;
      });
}
}  // namespace
}  // namespace mmla

using namespace mmla;

#undef RUN
#define RUN(expr) HIPCHK(c, (expr))

extern "C" {

int mmla_si_loss_grad(mmla_ctx* c, const float* packed, int64_t n_floats, int32_t n_classes, const float* x,
                      const int32_t* labels, int64_t n, float* loss, float* grad, uint32_t flags) {
  return loss_grad(c, "si_loss_grad", false, MMLA_SI_TRAIN_MAX_CLASSES, packed, n_floats, n_classes, x, labels, n, 0,
                   0, nullptr, loss, grad, nullptr, flags);
}

int mmla_si_finetune(mmla_ctx* c, const float* packed, int64_t n_floats, int32_t n_classes, const float* x,
                     const int32_t* labels, int64_t n_train, const float* val_x, const int32_t* val_labels,
                     int64_t n_val, int32_t epochs, int32_t batch, float lr, const int32_t* perm,
                     float* packed_out, float* history, uint32_t flags) {
  FitCall a = fit_call("si_finetune", packed, n_floats, x, labels, n_train, val_x, val_labels, n_val, epochs, batch,
                       perm, packed_out, history, flags);
  a.n_classes = n_classes;
  return si_fit(c, a, false, MMLA_SI_TRAIN_MAX_CLASSES, lr, 0);
}

int mmla_si_base_drop_mask(mmla_ctx* c, int64_t drop_seed, int32_t epoch, const int32_t* sample_ids, int64_t n,
                           uint8_t* mask_a, uint8_t* mask_b, uint32_t flags) {
  if (!c) return MMLA_E_INVALID;
  if (n < 1 || n > (1 << 20)) return fail(c, MMLA_E_INVALID, "si_base_drop_mask: n %lld outside [1, 2^20]", (long long)n);
  if (epoch < 0) return fail(c, MMLA_E_INVALID, "si_base_drop_mask: epoch %d < 0", epoch);
  if (!mask_a || !mask_b) return fail(c, MMLA_E_INVALID, "si_base_drop_mask: null pointer");
  Stager st{c, (flags & MMLA_DEVICE_PTR) != 0};
  if (!st.dev) CHK(check_ids(c, "si_base_drop_mask", sample_ids, n));
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  int32_t* sid = nullptr;
  const int32_t* dids = nullptr;
  uint8_t *da = nullptr, *db = nullptr;
  CHK(carve_slot(c, S_FT, [&](Carver& cv) -> int {
    sid = cv.take<int32_t>(n);
    CHK(st.in(cv, sample_ids, (size_t)n, &dids));
    if (!st.dev && !sample_ids) cv.take<int32_t>(n);   // the ids' place, used or not
    da = st.out(cv, mask_a, (size_t)n * SBB_MAP);
    db = st.out(cv, mask_b, (size_t)n * SBB_EMB);
    return MMLA_OK;
  }));
  RUN(sbb_ids(dids, nullptr, 0, (int)n, (int)n, sid, s));
  RUN(sbb_drop_mask(SbbDrop{(uint64_t)drop_seed, (uint32_t)epoch, sid}, (int)n, da, db, s));
  CHK(st.back(mask_a, da, (size_t)n * SBB_MAP));
  CHK(st.back(mask_b, db, (size_t)n * SBB_EMB));
  return finish(c, st.dev);
}

int mmla_si_base_loss_grad(mmla_ctx* c, const float* packed, int64_t n_floats, int32_t n_classes, const float* x,
                           const int32_t* labels, int64_t n, int64_t drop_seed, int32_t epoch,
                           const int32_t* sample_ids, float* loss, float* grad, float* moving_out,
                           uint32_t flags) {
  return loss_grad(c, "si_base_loss_grad", true, MMLA_SI_BASE_MAX_CLASSES, packed, n_floats, n_classes, x, labels, n,
                   drop_seed, epoch, sample_ids, loss, grad, moving_out, flags);
}

int mmla_si_base_train(mmla_ctx* c, const float* packed, int64_t n_floats, int32_t n_classes, const float* x,
                       const int32_t* labels, int64_t n_train, const float* val_x, const int32_t* val_labels,
                       int64_t n_val, int32_t epochs, int32_t batch, float lr, const int32_t* perm,
                       int64_t drop_seed, int32_t patience, int32_t ckpt_period, float* packed_out,
                       float* best_out, float* history, int32_t* epochs_run, int32_t* best_epoch,
                       uint32_t flags) {
  FitCall a = fit_call("si_base_train", packed, n_floats, x, labels, n_train, val_x, val_labels, n_val, epochs, batch,
                       perm, packed_out, history, flags);
  a.n_classes = n_classes;
  a.callbacks = FIT_STOP | FIT_CKPT;
  a.patience = patience;
  a.ckpt_period = ckpt_period;
  a.best_out = best_out;
  a.epochs_run = epochs_run;
  a.best_epoch = best_epoch;
  // NaN: rows after an early stop
  a.nan_fill = [](float* h, size_t n, hipStream_t s) { return hipMemsetAsync(h, 0xff, n * sizeof(float), s); };
  return si_fit(c, a, true, MMLA_SI_BASE_MAX_CLASSES, lr, drop_seed);
}

}  // extern "C"
