// libmmla weights: the packed float blob of mmla_load_weights -> device tensors in the layouts the
// kernels read (exact f32, the 3xFP16 hi/lo splits, the fused res_block fragments).
#include <algorithm>
#include <cmath>

#include "conv_h3.h"
#include "internal.h"
#include "nets.h"
#include "resblk.h"

using namespace mmla;

namespace mmla __attribute__((visibility("hidden"))) {
void free_allocs(std::vector<void*>& al) {
  for (void* p : al) (void)hipFree(p);
  al.clear();
}
}  // namespace mmla

namespace {

struct Cursor {
  const float* p;
  int64_t left;
  bool ok = true;
  bool f16_bad = false;   // a tensor taken so far holds inf / NaN: that model runs exact f32 only
  const float* take(int64_t n) {
    if (n > left) {
      ok = false;
      return nullptr;
    }
    const float* r = p;
    p += n;
    left -= n;
    return r;
  }
};

int upload(mmla_ctx* c, std::vector<void*>& allocs, const void* host, size_t bytes, float** out) {
  void* d = nullptr;
  if (hipMalloc(&d, bytes) != hipSuccess) return fail(c, MMLA_E_OOM, "weight hipMalloc failed");
  allocs.push_back(d);
  HIPCHK(c, hipMemcpy(d, host, bytes, hipMemcpyHostToDevice));
  *out = static_cast<float*>(d);
  return MMLA_OK;
}

int upload_u16(mmla_ctx* c, std::vector<void*>& allocs, const std::vector<uint16_t>& h, uint16_t** out) {
  float* p = nullptr;
  CHK(upload(c, allocs, h.data(), h.size() * sizeof(uint16_t), &p));
  *out = reinterpret_cast<uint16_t*>(p);
  return MMLA_OK;
}

// The power-of-two scale at which a weight tensor is split into fp16 hi + lo for the 3xFP16 MFMA
// paths (one fixed 2^8 sent a whole model to exact f32 as soon as one weight
// reached 255.9).  2^8 for the usual max |w| in [1/16, 255.9) -- the arithmetic of earlier rounds,
// bit for bit -- else the scale that puts max |w| in [2^13, 2^14): far from the fp16 overflow and
// with the lo halves of the large weights normal.  The kernels multiply by its inverse (exact).
// false in *finite for a tensor holding inf / NaN (that model runs exact f32).
float pick_wscale(const float* w, size_t n, bool* finite) {
  float m = 0.0f;
  *finite = true;
  for (size_t i = 0; i < n; ++i) {
    const float a = std::fabs(w[i]);
    if (!(a <= 3.4e38f)) *finite = false;
    else m = std::max(m, a);
  }
  if (m == 0.0f || (m < 255.9f && m >= 0.0625f)) return 256.0f;
  // e >= -126: the largest finite max |w| (< 2^128) needs e = -114, so after the clamp
  // m * 2^e < 2^14 for every finite tensor and its fp16 hi half never overflows
  const int e = std::max(-126, std::min(100, (int)std::floor(std::log2(16384.0 / m))));
  return std::ldexp(1.0f, e);
}

int take_conv(mmla_ctx* c, Cursor& cur, std::vector<void*>& al, int kh, int kw, int cin, int cout,
              ConvW* w) {
  const float* k = cur.take((int64_t)kh * kw * cin * cout);
  const float* b = cur.take(cout);
  if (!cur.ok) return fail(c, MMLA_E_SHAPE, "weight blob too short");
  // 3xFP16: any finite tensor fits the fp16 split at its own power-of-two scale
  bool finite = true;
  w->wscale = pick_wscale(k, (size_t)kh * kw * cin * cout, &finite);
  if (!finite) cur.f16_bad = true;
  w->kh = kh;
  w->kw = kw;
  w->cin = cin;
  w->cout = cout;
  w->cout_pad = (cout + 31) / 32 * 32;
  if (w->cout_pad > 128) w->cout_pad = (cout + 127) / 128 * 128;
  std::vector<float> kp((size_t)kh * kw * cin * w->cout_pad, 0.0f), bp(w->cout_pad, 0.0f);
  for (int64_t r = 0; r < (int64_t)kh * kw * cin; ++r)
    memcpy(&kp[r * w->cout_pad], k + r * cout, sizeof(float) * cout);
  memcpy(bp.data(), b, sizeof(float) * cout);
  CHK(upload(c, al, kp.data(), kp.size() * sizeof(float), &w->wt));
  CHK(upload(c, al, bp.data(), bp.size() * sizeof(float), &w->bias));
  // spatial conv: also the 3xFP16 operand layout (cin % 4 != 0: only the SI stem's 4-tap Conv1D,
  // conv_h3.hip stages it element-wise)
  // (1x1 convs with 16-channel steps too: the OD pool blocks' shortcut, fused into the pooled conv(4,1))
  if ((kh * kw > 1 && (cin % 4 == 0 || (kh == 4 && kw == 1 && cout <= 32))) || (kh * kw == 1 && cin % 16 == 0)) {
    w->cin_pad = (cin + 15) / 16 * 16;
    const size_t n = (size_t)kh * kw * w->cout_pad * w->cin_pad;
    std::vector<uint16_t> hi(n), lo(n);
    conv_h3_split_weights(k, kh, kw, cin, cout, w->cin_pad, w->cout_pad, hi.data(), lo.data(),
                          w->wscale);
    CHK(upload_u16(c, al, hi, &w->wh));
    CHK(upload_u16(c, al, lo, &w->wl));
  }
  if (cin % 16 == 0 && cout % 16 == 0) {   // fused res_block layout (resblk.hip)
    w->kpad = (kh * kw * cin + 31) / 32 * 32;
    const size_t n = (size_t)cout * w->kpad;
    std::vector<uint16_t> hi(n), lo(n);
    // the 3x3 (GEMM 1) and conv(4,1) (GEMM 2) weights in MFMA fragment order; the 1x1 shortcut
    // keeps [co][k] rows
    resblk_split_weights(k, kh * kw, cin, cout, w->kpad, hi.data(), lo.data(), kh > 1, w->wscale);
    CHK(upload_u16(c, al, hi, &w->fh));
    CHK(upload_u16(c, al, lo, &w->fl));
  }
  return MMLA_OK;
}

int take_bn(mmla_ctx* c, Cursor& cur, std::vector<void*>& al, int ch, BnW* bn) {
  const float* g = cur.take(ch);
  const float* be = cur.take(ch);
  const float* m = cur.take(ch);
  const float* v = cur.take(ch);
  if (!cur.ok) return fail(c, MMLA_E_SHAPE, "weight blob too short");
  std::vector<float> sc(ch), sh(ch);
  for (int i = 0; i < ch; ++i) {   // Keras BN(eps=1e-3) inference: x * s + (beta - mean * s)
    const double s = (double)g[i] / std::sqrt((double)v[i] + 1e-3);
    sc[i] = (float)s;
    sh[i] = (float)((double)be[i] - (double)m[i] * s);
  }
  bn->c = ch;
  CHK(upload(c, al, sc.data(), ch * sizeof(float), &bn->scale));
  CHK(upload(c, al, sh.data(), ch * sizeof(float), &bn->shift));
  return MMLA_OK;
}

int take_lstm(mmla_ctx* c, Cursor& cur, std::vector<void*>& al, int d, LstmW* l) {
  for (int dir = 0; dir < 2; ++dir) {
    const float* k = cur.take((int64_t)d * 1024);
    const float* r = cur.take(256 * 1024);
    const float* b = cur.take(1024);
    if (!cur.ok) return fail(c, MMLA_E_SHAPE, "weight blob too short");
    std::vector<float> wc((size_t)(256 + d) * 1024);
    memcpy(wc.data(), r, sizeof(float) * 256 * 1024);
    memcpy(wc.data() + 256 * 1024, k, sizeof(float) * d * 1024);
    CHK(upload(c, al, wc.data(), wc.size() * sizeof(float), &l->wcat[dir]));
    CHK(upload(c, al, b, 1024 * sizeof(float), &l->bias[dir]));
    bool finite = true;
    l->ws[dir] = pick_wscale(wc.data(), wc.size(), &finite);
    if (!finite) cur.f16_bad = true;
    std::vector<uint16_t> hi(wc.size()), lo(wc.size());
    bilstm_h3_split_weights(wc.data(), d, hi.data(), lo.data(), l->ws[dir]);
    CHK(upload_u16(c, al, hi, &l->wth[dir]));
    CHK(upload_u16(c, al, lo, &l->wtl[dir]));
  }
  return MMLA_OK;
}

// the nine res units of either network; the two blobs differ in where the shortcut sits: OD
// bn_in, ca, bn_mid, cb, sc; SI bn_in, ca, bn_mid, sc, cb
int take_units(mmla_ctx* c, Cursor& cur, std::vector<void*>& al, ResUnitW* unit, int cin, int kh_a,
               int kw_a, int kh_b, int kw_b, bool sc_last) {
  for (int u = 0; u < 9; ++u) {
    const int ch = CH[u];
    ResUnitW& U = unit[u];
    CHK(take_bn(c, cur, al, cin, &U.bn_in));
    CHK(take_conv(c, cur, al, kh_a, kw_a, cin, ch, &U.ca));
    CHK(take_bn(c, cur, al, ch, &U.bn_mid));
    if (POOL[u] && !sc_last) CHK(take_conv(c, cur, al, 1, 1, cin, ch, &U.sc));
    CHK(take_conv(c, cur, al, kh_b, kw_b, ch, ch, &U.cb));
    if (POOL[u] && sc_last) CHK(take_conv(c, cur, al, 1, 1, cin, ch, &U.sc));
    cin = ch;
  }
  return MMLA_OK;
}

}  // namespace

extern "C" int mmla_load_weights(mmla_ctx* c, int kind, const float* packed, int64_t n_floats,
                                 int32_t n_classes, int32_t head) {
  if (!c) return MMLA_E_INVALID;
  if (!packed || n_floats <= 0) return fail(c, MMLA_E_INVALID, "null weight blob");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  Cursor cur{packed, n_floats};
  if (kind == MMLA_MODEL_OD) {
    if (n_classes < 2 || n_classes > MMLA_OD_MAX_CLASSES)
      return fail(c, MMLA_E_INVALID, "OD n_classes %d outside [2, %d]", n_classes, MMLA_OD_MAX_CLASSES);
    // more than two classes: the size is checked before the loaded model is let go (a two-class blob of the
    // wrong size keeps its MMLA_E_SHAPE below)
    // a one-channel model's blob (stem [1,1,1,16]) is 32 floats shorter; 513 K - 32 is no multiple of 513,
    // so no three-channel blob has that size
    const int channels = n_floats == od_blob_floats(n_classes, 1) ? 1 : 3;
    const int64_t want = od_blob_floats(n_classes);
    if (n_classes != 2 && channels == 3 && n_floats != want)
      return fail(c, MMLA_E_INVALID, "OD blob of %lld floats, %d classes need %lld", (long long)n_floats, n_classes,
                  (long long)want);
    free_allocs(c->od_allocs);
    c->od_loaded = false;
    OdNet& W = c->od;
    auto& al = c->od_allocs;
    if (channels == 1) {
      // the stem as three rows {w, 0, 0} (and its bias): the network reads the pixel (g, g, g), and
      // fma(g, 0, acc) leaves the one-channel sum as it is
      const float* k1 = cur.take(16);
      const float* b1 = cur.take(16);
      if (!cur.ok) return fail(c, MMLA_E_SHAPE, "weight blob too short");
      float wide[4 * 16] = {0.0f};
      memcpy(wide, k1, 16 * sizeof(float));
      memcpy(wide + 3 * 16, b1, 16 * sizeof(float));
      Cursor cs{wide, 4 * 16};
      CHK(take_conv(c, cs, al, 1, 1, 3, 16, &W.stem));
      if (cs.f16_bad) cur.f16_bad = true;
    } else {
      CHK(take_conv(c, cur, al, 1, 1, 3, 16, &W.stem));
    }
    CHK(take_units(c, cur, al, W.blk, 16, 3, 3, 4, 1, true));
    CHK(take_lstm(c, cur, al, 128, &W.lstm));
    const float* hw = cur.take(512 * (int64_t)n_classes);
    const float* hb = cur.take(n_classes);
    if (!cur.ok) return fail(c, MMLA_E_SHAPE, "OD weight blob too short");
    CHK(upload(c, al, hw, 512 * (size_t)n_classes * sizeof(float), &W.head_w));
    CHK(upload(c, al, hb, (size_t)n_classes * sizeof(float), &W.head_b));
    W.k = n_classes;
    if (cur.left != 0)
      return fail(c, MMLA_E_SHAPE, "OD weight blob has %lld extra floats", (long long)cur.left);
    W.channels = channels;
    c->od_img_type = channels == 1 ? MMLA_OD_IMG_GRAY : MMLA_OD_IMG_ZCR;   // the type is the model's: reset
    c->od_f32_only = cur.f16_bad;   // some weight outside the fp16 range: exact f32 only
    c->od_loaded = true;
    return MMLA_OK;
  }
  if (kind == MMLA_MODEL_SI) {
    if (n_classes < 1) return fail(c, MMLA_E_INVALID, "SI n_classes must be >= 1");
    if (head != MMLA_HEAD_SOFTMAX && head != MMLA_HEAD_SIGMOID)
      return fail(c, MMLA_E_INVALID, "unknown head %d", head);
    free_allocs(c->si_allocs);
    free_allocs(c->si_head_allocs);
    c->si_loaded = false;
    SiNet& W = c->si;
    auto& al = c->si_allocs;
    CHK(take_conv(c, cur, al, 4, 1, 39, 32, &W.stem));
    CHK(take_units(c, cur, al, W.unit, 32, 3, 1, 3, 1, false));
    CHK(take_bn(c, cur, al, 128, &W.final_bn));
    CHK(take_lstm(c, cur, al, 128, &W.lstm));
    c->si_base_f16_bad = cur.f16_bad;
    W.dense = ConvW();
    CHK(take_conv(c, cur, c->si_head_allocs, 1, 1, 512, n_classes, &W.dense));
    if (cur.left != 0)
      return fail(c, MMLA_E_SHAPE, "SI weight blob has %lld extra floats", (long long)cur.left);
    W.k = n_classes;
    W.head = head;
    c->si_f32_only = cur.f16_bad;
    c->si_loaded = true;
    return MMLA_OK;
  }
  return fail(c, MMLA_E_INVALID, "unknown model kind %d", kind);
}

extern "C" int mmla_od_classes(mmla_ctx* c, int32_t* k) {
  if (!c) return MMLA_E_INVALID;
  if (!k) return fail(c, MMLA_E_INVALID, "od_classes: null pointer");
  if (!c->od_loaded) return fail(c, MMLA_E_NOWEIGHTS, "OD weights not loaded");
  *k = c->od.k;
  return MMLA_OK;
}

extern "C" int mmla_od_set_image_type(mmla_ctx* c, int32_t type) {
  if (!c) return MMLA_E_INVALID;
  if (!c->od_loaded) return fail(c, MMLA_E_NOWEIGHTS, "OD weights not loaded");
  if (type < MMLA_OD_IMG_ZCR || type > MMLA_OD_IMG_VIRIDIS) return fail(c, MMLA_E_INVALID, "unknown image type %d", type);
  if (c->od.channels == 1 && type != MMLA_OD_IMG_GRAY)
    return fail(c, MMLA_E_INVALID, "a one-channel OD model reads gray images only (type %d)", type);
  c->od_img_type = type;
  return MMLA_OK;
}

extern "C" int mmla_od_image(mmla_ctx* c, int32_t* type, int32_t* channels) {
  if (!c) return MMLA_E_INVALID;
  if (!c->od_loaded) return fail(c, MMLA_E_NOWEIGHTS, "OD weights not loaded");
  if (type) *type = c->od_img_type;
  if (channels) *channels = c->od.channels;
  return MMLA_OK;
}

// The Dense head of the loaded SI model replaced in place: the tensors go through take_conv as the
// blob's last two do in mmla_load_weights (the 3xFP16 split at the tensor's own scale, a non-finite
// tensor sending the whole model to exact f32), so every later call gives the bits of a full load with
// that head.  The old head is freed only once the new one is on the device.
extern "C" int mmla_si_set_head(mmla_ctx* c, const float* w, const float* b, int32_t n_classes, int32_t head) {
  if (!c) return MMLA_E_INVALID;
  if (!w || !b) return fail(c, MMLA_E_INVALID, "null head tensors");
  if (n_classes < 1) return fail(c, MMLA_E_INVALID, "SI n_classes must be >= 1");
  if (head != MMLA_HEAD_SOFTMAX && head != MMLA_HEAD_SIGMOID)
    return fail(c, MMLA_E_INVALID, "unknown head %d", head);
  if (!c->si_loaded) return fail(c, MMLA_E_NOWEIGHTS, "SI weights not loaded");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // kernel [512, K] then bias [K], contiguous as in the blob
  std::vector<float> blob((size_t)512 * n_classes + n_classes);
  memcpy(blob.data(), w, sizeof(float) * 512 * n_classes);
  memcpy(blob.data() + (size_t)512 * n_classes, b, sizeof(float) * n_classes);
  Cursor cur{blob.data(), (int64_t)blob.size()};
  std::vector<void*> al;
  ConvW dense;
  const int rc = take_conv(c, cur, al, 1, 1, 512, n_classes, &dense);
  if (rc != MMLA_OK) {   // the model keeps the head it had
    free_allocs(al);
    return rc;
  }
  free_allocs(c->si_head_allocs);
  c->si_head_allocs.swap(al);
  c->si.dense = dense;
  c->si.k = n_classes;
  c->si.head = head;
  c->si_f32_only = c->si_base_f16_bad || cur.f16_bad;
  return MMLA_OK;
}
