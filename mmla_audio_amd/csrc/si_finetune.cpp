// libmmla: speaker registration stage 2 -- mmla_si_loss_grad and mmla_si_finetune -- and training the SI base
// model from scratch -- mmla_si_base_drop_mask, mmla_si_base_loss_grad, mmla_si_base_train (include/mmla.h):
// the same engine with `base` set, which swaps in si_base.hip's training-mode layers.
// Which kernel of si_bwd.hip runs which layer, forward and backward, over a copy of the packed SI blob
// in workspace slot S_FT; the context's loaded model is not touched.  A training step is a fixed
// sequence of launches on the context's stream with no host synchronisation: the loss bookkeeping
// lives in device memory and the history is read once at the end of the fit.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

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

// carve: first pass (base == nullptr) only measures
struct Carver {
  char* base;
  size_t total = 0;
  template <typename T>
  T* take(size_t count) {
    const size_t at = total;
    total += (count * sizeof(T) + 255) & ~(size_t)255;
    return base ? reinterpret_cast<T*>(base + at) : nullptr;
  }
};

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
    for (int d = 0; d < 2; ++d) {
      l.wk[d] = e.W + e.off.lk[d];
      l.wr[d] = e.W + e.off.lr[d];
      l.bias[d] = e.W + e.off.lb[d];
      l.dwk[d] = e.G + e.off.lk[d];
      l.dwr[d] = e.G + e.off.lr[d];
      l.dbias[d] = e.G + e.off.lb[d];
    }
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

// e.mask: trainable = everything but moving_mean / moving_variance
int mark_trainable(Engine& e) {
  hipStream_t s = e.c->stream;
  HIPCHK(e.c, hipMemsetAsync(e.mask, 1, e.off.total, s));
  auto frozen = [&](size_t bn, int ch) { return hipMemsetAsync(e.mask + bn + 2 * ch, 0, 2 * (size_t)ch, s); };
  for (int i = 0; i < 9; ++i) {
    HIPCHK(e.c, frozen(e.off.u[i].bn_in, e.off.u[i].cin));
    HIPCHK(e.c, frozen(e.off.u[i].bn_mid, e.off.u[i].cout));
  }
  HIPCHK(e.c, frozen(e.off.fbn, 128));
  return MMLA_OK;
}

// perm [epochs, n]: every row a permutation of 0..n-1
int check_perm(mmla_ctx* c, const char* who, const int32_t* perm, int epochs, int64_t n) {
  std::vector<uint8_t> seen(n);
  for (int ep = 0; ep < epochs; ++ep) {
    std::fill(seen.begin(), seen.end(), 0);
    const int32_t* p = perm + (size_t)ep * n;
    for (int64_t i = 0; i < n; ++i) {
      if (p[i] < 0 || p[i] >= n || seen[p[i]])
        return fail(c, MMLA_E_INVALID, "%s: perm row %d is not a permutation of 0..%lld", who, ep,
                    (long long)(n - 1));
      seen[p[i]] = 1;
    }
  }
  return MMLA_OK;
}

int check_labels(mmla_ctx* c, const char* what, const int32_t* l, int64_t n, int K) {
  for (int64_t i = 0; i < n; ++i)
    if (l[i] < 0 || l[i] >= K)
      return fail(c, MMLA_E_INVALID, "%s[%lld] = %d outside [0, %d)", what, (long long)i, l[i], K);
  return MMLA_OK;
}

}  // namespace
}  // namespace mmla

using namespace mmla;

#undef RUN
#define RUN(expr) HIPCHK(c, (expr))

extern "C" {

int mmla_si_loss_grad(mmla_ctx* c, const float* packed, int64_t n_floats, int32_t n_classes, const float* x,
                      const int32_t* labels, int64_t n, float* loss, float* grad, uint32_t flags) {
  if (!c) return MMLA_E_INVALID;
  CHK(check_common(c, "si_loss_grad", n_floats, n_classes));
  if (n < 1 || n > kMaxPass)
    return fail(c, MMLA_E_INVALID, "si_loss_grad: n %lld outside [1, %d]", (long long)n, kMaxPass);
  if (!packed || !x || !labels || !loss || !grad) return fail(c, MMLA_E_INVALID, "si_loss_grad: null pointer");
  const bool dev = flags & MMLA_DEVICE_PTR;
  if (!dev) CHK(check_labels(c, "labels", labels, n, n_classes));
  HIPCHK(c, hipSetDevice(c->device));
  Engine e;
  e.c = c;
  e.K = n_classes;
  e.cap = (int)n;
  e.off = si_offsets(n_classes);
  Carver cv{nullptr};
  carve(e, cv, false);
  float* lp = cv.take<float>(2);
  void* p = nullptr;
  CHK(ws_get(c, S_FT, cv.total, &p));
  cv = Carver{static_cast<char*>(p)};
  carve(e, cv, false);
  lp = cv.take<float>(2);
  hipStream_t s = c->stream;
  const size_t wbytes = e.off.total * sizeof(float), xbytes = (size_t)n * SI_T * SI_D * sizeof(float);
  const hipMemcpyKind in = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  HIPCHK(c, hipMemcpyAsync(e.W, packed, wbytes, in, s));
  HIPCHK(c, hipMemcpyAsync(e.xb, x, xbytes, in, s));
  HIPCHK(c, hipMemcpyAsync(e.lb, labels, (size_t)n * sizeof(int32_t), in, s));
  HIPCHK(c, hipMemsetAsync(e.G, 0, wbytes, s));   // the moving-statistics slots stay 0
  HIPCHK(c, hipMemsetAsync(e.st, 0, SIB_ST * sizeof(double), s));
  CHK(forward(e, (int)n, e.st, true, (float)n));
  CHK(l2_term(e));
  CHK(backward(e, (int)n));
  RUN(sib_loss_pair(e.st, (int)n, lp, s));
  const hipMemcpyKind out = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  HIPCHK(c, hipMemcpyAsync(grad, e.G, wbytes, out, s));
  HIPCHK(c, hipMemcpyAsync(loss, lp, 2 * sizeof(float), out, s));
  return finish(c, dev);
}

int mmla_si_finetune(mmla_ctx* c, const float* packed, int64_t n_floats, int32_t n_classes, const float* x,
                     const int32_t* labels, int64_t n_train, const float* val_x, const int32_t* val_labels,
                     int64_t n_val, int32_t epochs, int32_t batch, float lr, const int32_t* perm,
                     float* packed_out, float* history, uint32_t flags) {
  if (!c) return MMLA_E_INVALID;
  CHK(check_common(c, "si_finetune", n_floats, n_classes));
  if (batch < 1) return fail(c, MMLA_E_INVALID, "si_finetune: batch %d < 1", batch);
  if (n_train < 1) return fail(c, MMLA_E_INVALID, "si_finetune: n_train %lld < 1", (long long)n_train);
  if (n_val < 0 || epochs < 0 || n_train > (1 << 24) || n_val > (1 << 24))
    return fail(c, MMLA_E_INVALID, "si_finetune: bad sizes (n_val %lld, epochs %d)", (long long)n_val, epochs);
  if (std::min<int64_t>(batch, n_train) > kMaxPass)
    return fail(c, MMLA_E_INVALID, "si_finetune: a batch of more than %d windows", kMaxPass);
  if (!packed || !x || !labels || !packed_out || (epochs > 0 && (!perm || !history)) ||
      (n_val > 0 && (!val_x || !val_labels)))
    return fail(c, MMLA_E_INVALID, "si_finetune: null pointer");
  const bool dev = flags & MMLA_DEVICE_PTR;
  const int K = n_classes;
  if (!dev) {
    CHK(check_labels(c, "labels", labels, n_train, K));
    CHK(check_labels(c, "val_labels", val_labels, n_val, K));
    CHK(check_perm(c, "si_finetune", perm, epochs, n_train));
  }
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  Engine e;
  e.c = c;
  e.K = K;
  e.off = si_offsets(K);
  const size_t wbytes = e.off.total * sizeof(float);
  const hipMemcpyKind in = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  const hipMemcpyKind out = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (epochs == 0) {   // the input blob, unchanged
    if (packed_out == packed) return MMLA_OK;
    if (!dev) {
      std::memcpy(packed_out, packed, wbytes);
      return MMLA_OK;
    }
    HIPCHK(c, hipMemcpyAsync(packed_out, packed, wbytes, in, s));
    return finish(c, dev);
  }
  e.cap = (int)std::max<int64_t>(std::min<int64_t>(batch, n_train), std::min<int64_t>(n_val, 64));
  const size_t row = (size_t)SI_T * SI_D;
  const float *dx = x, *dvx = val_x;
  const int32_t *dl = labels, *dvl = val_labels, *dperm = perm;
  float* dhist = history;
  // measure, allocate, carve
  size_t total = 0;
  float *sx = nullptr, *svx = nullptr, *shist = nullptr;
  int32_t *sl = nullptr, *svl = nullptr, *sperm = nullptr;
  for (int pass = 0; pass < 2; ++pass) {
    void* p = nullptr;
    if (pass) CHK(ws_get(c, S_FT, total, &p));
    Carver cv{static_cast<char*>(p)};
    carve(e, cv, true);
    if (!dev) {
      sx = cv.take<float>((size_t)n_train * row);
      sl = cv.take<int32_t>(n_train);
      svx = cv.take<float>((size_t)n_val * row);
      svl = cv.take<int32_t>(n_val);
      sperm = cv.take<int32_t>((size_t)epochs * n_train);
      shist = cv.take<float>((size_t)epochs * 4);
    }
    total = cv.total;
  }
  if (!dev) {
    HIPCHK(c, hipMemcpyAsync(sx, x, (size_t)n_train * row * sizeof(float), in, s));
    HIPCHK(c, hipMemcpyAsync(sl, labels, (size_t)n_train * sizeof(int32_t), in, s));
    if (n_val > 0) {
      HIPCHK(c, hipMemcpyAsync(svx, val_x, (size_t)n_val * row * sizeof(float), in, s));
      HIPCHK(c, hipMemcpyAsync(svl, val_labels, (size_t)n_val * sizeof(int32_t), in, s));
    }
    HIPCHK(c, hipMemcpyAsync(sperm, perm, (size_t)epochs * n_train * sizeof(int32_t), in, s));
    dx = sx;
    dl = sl;
    dvx = svx;
    dvl = svl;
    dperm = sperm;
    dhist = shist;
  }
  HIPCHK(c, hipMemcpyAsync(e.W, packed, wbytes, in, s));
  HIPCHK(c, hipMemsetAsync(e.G, 0, wbytes, s));     // the moving-statistics slots stay 0
  HIPCHK(c, hipMemsetAsync(e.rms, 0, wbytes, s));   // a new optimiser: every accumulator from 0
  HIPCHK(c, hipMemsetAsync(e.st, 0, SIB_ST * sizeof(double), s));
  CHK(mark_trainable(e));
  for (int ep = 0; ep < epochs; ++ep) {
    const int32_t* order = dperm + (size_t)ep * n_train;
    for (int64_t b0 = 0; b0 < n_train; b0 += batch) {
      const int nb = (int)std::min<int64_t>(batch, n_train - b0);
      RUN(sib_gather(dx, dl, order, (int)b0, nb, (int)n_train, (int)row, e.xb, e.lb, s));
      CHK(forward(e, nb, e.st, true, (float)nb));
      CHK(l2_term(e));
      CHK(backward(e, nb));
      RUN(sib_fold_batch(e.st, nb, s));
      RUN(sib_rmsprop(e.W, e.rms, e.G, e.mask, (int64_t)e.off.total, lr, s));
    }
    CHK(l2_term(e));
    for (int64_t v0 = 0; v0 < n_val; v0 += e.cap) {
      const int nb = (int)std::min<int64_t>(e.cap, n_val - v0);
      RUN(sib_gather(dvx, dvl, nullptr, (int)v0, nb, (int)n_val, (int)row, e.xb, e.lb, s));
      CHK(forward(e, nb, e.st + 5, false, 1.0f));
    }
    RUN(sib_end_epoch(e.st, (int)n_train, (int)n_val, dhist + (size_t)ep * 4, s));
  }
  HIPCHK(c, hipMemcpyAsync(packed_out, e.W, wbytes, out, s));
  if (!dev) HIPCHK(c, hipMemcpyAsync(history, dhist, (size_t)epochs * 4 * sizeof(float), out, s));
  return finish(c, dev);
}

int mmla_si_base_drop_mask(mmla_ctx* c, int64_t drop_seed, int32_t epoch, const int32_t* sample_ids, int64_t n,
                           uint8_t* mask_a, uint8_t* mask_b, uint32_t flags) {
  if (!c) return MMLA_E_INVALID;
  if (n < 1 || n > (1 << 20)) return fail(c, MMLA_E_INVALID, "si_base_drop_mask: n %lld outside [1, 2^20]", (long long)n);
  if (epoch < 0) return fail(c, MMLA_E_INVALID, "si_base_drop_mask: epoch %d < 0", epoch);
  if (!mask_a || !mask_b) return fail(c, MMLA_E_INVALID, "si_base_drop_mask: null pointer");
  const bool dev = flags & MMLA_DEVICE_PTR;
  if (!dev && sample_ids)
    for (int64_t i = 0; i < n; ++i)
      if (sample_ids[i] < 0)
        return fail(c, MMLA_E_INVALID, "si_base_drop_mask: sample_ids[%lld] = %d < 0", (long long)i, sample_ids[i]);
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  int32_t *sid = nullptr, *ids = nullptr;
  uint8_t *da = mask_a, *db = mask_b;
  size_t total = 0;
  for (int pass = 0; pass < 2; ++pass) {
    void* p = nullptr;
    if (pass) CHK(ws_get(c, S_FT, total, &p));
    Carver cv{static_cast<char*>(p)};
    sid = cv.take<int32_t>(n);
    if (!dev) {
      ids = cv.take<int32_t>(n);
      da = cv.take<uint8_t>((size_t)n * SBB_MAP);
      db = cv.take<uint8_t>((size_t)n * SBB_EMB);
    }
    total = cv.total;
  }
  const int32_t* dids = sample_ids;
  if (!dev && sample_ids) {
    HIPCHK(c, hipMemcpyAsync(ids, sample_ids, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    dids = ids;
  }
  RUN(sbb_ids(dids, nullptr, 0, (int)n, (int)n, sid, s));
  RUN(sbb_drop_mask(SbbDrop{(uint64_t)drop_seed, (uint32_t)epoch, sid}, (int)n, da, db, s));
  if (!dev) {
    HIPCHK(c, hipMemcpyAsync(mask_a, da, (size_t)n * SBB_MAP, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(mask_b, db, (size_t)n * SBB_EMB, hipMemcpyDeviceToHost, s));
  }
  return finish(c, dev);
}

int mmla_si_base_loss_grad(mmla_ctx* c, const float* packed, int64_t n_floats, int32_t n_classes, const float* x,
                           const int32_t* labels, int64_t n, int64_t drop_seed, int32_t epoch,
                           const int32_t* sample_ids, float* loss, float* grad, float* moving_out,
                           uint32_t flags) {
  if (!c) return MMLA_E_INVALID;
  CHK(check_common(c, "si_base_loss_grad", n_floats, n_classes, MMLA_SI_BASE_MAX_CLASSES));
  if (n < 1 || n > kMaxPass)
    return fail(c, MMLA_E_INVALID, "si_base_loss_grad: n %lld outside [1, %d]", (long long)n, kMaxPass);
  if (epoch < 0) return fail(c, MMLA_E_INVALID, "si_base_loss_grad: epoch %d < 0", epoch);
  if (!packed || !x || !labels || !loss || !grad)
    return fail(c, MMLA_E_INVALID, "si_base_loss_grad: null pointer");
  const bool dev = flags & MMLA_DEVICE_PTR;
  if (!dev) {
    CHK(check_labels(c, "labels", labels, n, n_classes));
    if (sample_ids)
      for (int64_t i = 0; i < n; ++i)
        if (sample_ids[i] < 0)
          return fail(c, MMLA_E_INVALID, "si_base_loss_grad: sample_ids[%lld] = %d < 0", (long long)i,
                      sample_ids[i]);
  }
  HIPCHK(c, hipSetDevice(c->device));
  Engine e;
  e.c = c;
  e.K = n_classes;
  e.cap = (int)n;
  e.base = true;
  e.off = si_offsets(n_classes);
  float* lp = nullptr;
  int32_t* ids = nullptr;
  size_t total = 0;
  for (int pass = 0; pass < 2; ++pass) {
    void* p = nullptr;
    if (pass) CHK(ws_get(c, S_FT, total, &p));
    Carver cv{static_cast<char*>(p)};
    carve(e, cv, false);
    lp = cv.take<float>(2);
    ids = cv.take<int32_t>(n);
    total = cv.total;
  }
  hipStream_t s = c->stream;
  const size_t wbytes = e.off.total * sizeof(float), xbytes = (size_t)n * SI_T * SI_D * sizeof(float);
  const hipMemcpyKind in = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  const hipMemcpyKind out = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  HIPCHK(c, hipMemcpyAsync(e.W, packed, wbytes, in, s));
  HIPCHK(c, hipMemcpyAsync(e.xb, x, xbytes, in, s));
  HIPCHK(c, hipMemcpyAsync(e.lb, labels, (size_t)n * sizeof(int32_t), in, s));
  if (sample_ids) HIPCHK(c, hipMemcpyAsync(ids, sample_ids, (size_t)n * sizeof(int32_t), in, s));
  RUN(sbb_ids(sample_ids ? ids : nullptr, nullptr, 0, (int)n, (int)n, e.sid, s));
  e.drop = SbbDrop{(uint64_t)drop_seed, (uint32_t)epoch, e.sid};
  HIPCHK(c, hipMemsetAsync(e.G, 0, wbytes, s));   // the moving-statistics slots stay 0
  HIPCHK(c, hipMemsetAsync(e.st, 0, SIB_ST * sizeof(double), s));
  CHK(forward(e, (int)n, e.st, true, (float)n));
  CHK(l2_term(e));
  CHK(backward(e, (int)n));
  RUN(sib_loss_pair(e.st, (int)n, lp, s));
  HIPCHK(c, hipMemcpyAsync(grad, e.G, wbytes, out, s));
  HIPCHK(c, hipMemcpyAsync(loss, lp, 2 * sizeof(float), out, s));
  if (moving_out) HIPCHK(c, hipMemcpyAsync(moving_out, e.W, wbytes, out, s));   // only the forward wrote W
  return finish(c, dev);
}

int mmla_si_base_train(mmla_ctx* c, const float* packed, int64_t n_floats, int32_t n_classes, const float* x,
                       const int32_t* labels, int64_t n_train, const float* val_x, const int32_t* val_labels,
                       int64_t n_val, int32_t epochs, int32_t batch, float lr, const int32_t* perm,
                       int64_t drop_seed, int32_t patience, int32_t ckpt_period, float* packed_out,
                       float* best_out, float* history, int32_t* epochs_run, int32_t* best_epoch,
                       uint32_t flags) {
  if (!c) return MMLA_E_INVALID;
  CHK(check_common(c, "si_base_train", n_floats, n_classes, MMLA_SI_BASE_MAX_CLASSES));
  if (batch < 1) return fail(c, MMLA_E_INVALID, "si_base_train: batch %d < 1", batch);
  if (n_train < 1) return fail(c, MMLA_E_INVALID, "si_base_train: n_train %lld < 1", (long long)n_train);
  if (n_val < 0 || epochs < 0 || patience < 0 || ckpt_period < 0 || n_train > (1 << 24) || n_val > (1 << 24))
    return fail(c, MMLA_E_INVALID, "si_base_train: bad sizes (n_val %lld, epochs %d, patience %d, ckpt_period %d)",
                (long long)n_val, epochs, patience, ckpt_period);
  if (std::min<int64_t>(batch, n_train) > kMaxPass)
    return fail(c, MMLA_E_INVALID, "si_base_train: a batch of more than %d windows", kMaxPass);
  if (!(lr >= 0.0f) || !std::isfinite(lr))
    return fail(c, MMLA_E_INVALID, "si_base_train: lr %g is negative or not finite", lr);
  const bool ckpt = ckpt_period > 0 && n_val > 0;
  if (!packed || !x || !labels || !packed_out || !epochs_run || !best_epoch ||
      (epochs > 0 && (!perm || !history)) || (n_val > 0 && (!val_x || !val_labels)) ||
      (epochs > 0 && ckpt && !best_out))
    return fail(c, MMLA_E_INVALID, "si_base_train: null pointer");
  const bool dev = flags & MMLA_DEVICE_PTR;
  const int K = n_classes;
  if (!dev) {
    CHK(check_labels(c, "labels", labels, n_train, K));
    CHK(check_labels(c, "val_labels", val_labels, n_val, K));
    CHK(check_perm(c, "si_base_train", perm, epochs, n_train));
  }
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  Engine e;
  e.c = c;
  e.K = K;
  e.base = true;
  e.off = si_offsets(K);
  const size_t wbytes = e.off.total * sizeof(float);
  const hipMemcpyKind in = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  const hipMemcpyKind out = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  int ran = 0, best_ep = -1;
  auto report = [&]() -> int {   // epochs_run, best_epoch: host or device words like every other output
    if (!dev) {
      *epochs_run = ran;
      *best_epoch = best_ep;
      return MMLA_OK;
    }
    HIPCHK(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(epochs_run), ran, 1, s));
    HIPCHK(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(best_epoch), best_ep, 1, s));
    return MMLA_OK;
  };
  if (epochs == 0) {   // the input blob, unchanged
    if (!dev) {
      if (packed_out != packed) std::memcpy(packed_out, packed, wbytes);
      return report();
    }
    if (packed_out != packed) HIPCHK(c, hipMemcpyAsync(packed_out, packed, wbytes, in, s));
    CHK(report());
    return finish(c, dev);
  }
  e.cap = (int)std::max<int64_t>(std::min<int64_t>(batch, n_train), std::min<int64_t>(n_val, 64));
  const size_t row = (size_t)SI_T * SI_D;
  const float *dx = x, *dvx = val_x;
  const int32_t *dl = labels, *dvl = val_labels, *dperm = perm;
  float *dhist = history, *dbest = best_out;
  size_t total = 0;
  float *sx = nullptr, *svx = nullptr, *shist = nullptr, *sbest = nullptr;
  int32_t *sl = nullptr, *svl = nullptr, *sperm = nullptr;
  for (int pass = 0; pass < 2; ++pass) {
    void* p = nullptr;
    if (pass) CHK(ws_get(c, S_FT, total, &p));
    Carver cv{static_cast<char*>(p)};
    carve(e, cv, true);
    if (!dev) {
      sx = cv.take<float>((size_t)n_train * row);
      sl = cv.take<int32_t>(n_train);
      svx = cv.take<float>((size_t)n_val * row);
      svl = cv.take<int32_t>(n_val);
      sperm = cv.take<int32_t>((size_t)epochs * n_train);
      shist = cv.take<float>((size_t)epochs * 4);
      sbest = ckpt ? cv.take<float>(e.off.total) : nullptr;
    }
    total = cv.total;
  }
  if (!dev) {
    HIPCHK(c, hipMemcpyAsync(sx, x, (size_t)n_train * row * sizeof(float), in, s));
    HIPCHK(c, hipMemcpyAsync(sl, labels, (size_t)n_train * sizeof(int32_t), in, s));
    if (n_val > 0) {
      HIPCHK(c, hipMemcpyAsync(svx, val_x, (size_t)n_val * row * sizeof(float), in, s));
      HIPCHK(c, hipMemcpyAsync(svl, val_labels, (size_t)n_val * sizeof(int32_t), in, s));
    }
    HIPCHK(c, hipMemcpyAsync(sperm, perm, (size_t)epochs * n_train * sizeof(int32_t), in, s));
    dx = sx;
    dl = sl;
    dvx = svx;
    dvl = svl;
    dperm = sperm;
    dhist = shist;
    dbest = sbest;
  }
  HIPCHK(c, hipMemcpyAsync(e.W, packed, wbytes, in, s));
  HIPCHK(c, hipMemsetAsync(e.G, 0, wbytes, s));     // the moving-statistics slots stay 0
  HIPCHK(c, hipMemsetAsync(e.rms, 0, wbytes, s));   // a new optimiser: every accumulator from 0
  HIPCHK(c, hipMemsetAsync(e.st, 0, SIB_ST * sizeof(double), s));
  CHK(mark_trainable(e));
  HIPCHK(c, hipMemsetAsync(dhist, 0xff, (size_t)epochs * 4 * sizeof(float), s));   // NaN: rows after an early stop
  const bool stopping = patience > 0 && n_val > 0;
  float best_loss = INFINITY, best_acc = -INFINITY;
  int wait = 0;
  for (int ep = 0; ep < epochs; ++ep) {
    const int32_t* order = dperm + (size_t)ep * n_train;
    for (int64_t b0 = 0; b0 < n_train; b0 += batch) {
      const int nb = (int)std::min<int64_t>(batch, n_train - b0);
      RUN(sib_gather(dx, dl, order, (int)b0, nb, (int)n_train, (int)row, e.xb, e.lb, s));
      RUN(sbb_ids(nullptr, order, (int)b0, nb, (int)n_train, e.sid, s));
      e.drop = SbbDrop{(uint64_t)drop_seed, (uint32_t)ep, e.sid};
      CHK(forward(e, nb, e.st, true, (float)nb));
      CHK(l2_term(e));
      CHK(backward(e, nb));
      RUN(sib_fold_batch(e.st, nb, s));
      RUN(sib_rmsprop(e.W, e.rms, e.G, e.mask, (int64_t)e.off.total, lr, s));
    }
    CHK(l2_term(e));
    for (int64_t v0 = 0; v0 < n_val; v0 += e.cap) {
      const int nb = (int)std::min<int64_t>(e.cap, n_val - v0);
      RUN(sib_gather(dvx, dvl, nullptr, (int)v0, nb, (int)n_val, (int)row, e.xb, e.lb, s));
      CHK(forward(e, nb, e.st + 5, false, 1.0f));
    }
    RUN(sib_end_epoch(e.st, (int)n_train, (int)n_val, dhist + (size_t)ep * 4, s));
    ran = ep + 1;
    if (!stopping && !ckpt) continue;
    // the two Keras callbacks: one history row read back per epoch
    float hrow[4];
    HIPCHK(c, hipMemcpyAsync(hrow, dhist + (size_t)ep * 4, sizeof(hrow), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    // ModelCheckpoint(val_categorical_accuracy, save_best_only, mode 'max', period)
    if (ckpt && (ep + 1) % ckpt_period == 0 && hrow[3] > best_acc) {
      best_acc = hrow[3];
      best_ep = ep;
      HIPCHK(c, hipMemcpyAsync(dbest, e.W, wbytes, hipMemcpyDeviceToDevice, s));
    }
    // EarlyStopping(val_loss, patience)
    if (!stopping) continue;
    if (hrow[2] < best_loss) {
      best_loss = hrow[2];
      wait = 0;
    } else if (++wait >= patience) {
      break;
    }
  }
  HIPCHK(c, hipMemcpyAsync(packed_out, e.W, wbytes, out, s));
  if (!dev) {
    HIPCHK(c, hipMemcpyAsync(history, dhist, (size_t)epochs * 4 * sizeof(float), out, s));
    if (best_ep >= 0) HIPCHK(c, hipMemcpyAsync(best_out, dbest, wbytes, out, s));
  }
  CHK(report());
  return finish(c, dev);
}

}  // extern "C"
