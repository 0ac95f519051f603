// libmmla network runners: OD-NET and SI-NET on one device micro-batch.  Which kernel runs each OD
// res block is decided in od_choose(), which launch covers each SI res unit in si_choose() (pool-chain,
// pair, single unit, conv pair in that order).  One filler per kernel argument struct, one FLOP
// formula per block kind, one tail that advances the state.  Precision, the split BiLSTM and the range
// words of a run are its Arith argument (internal.h), never the context's.  DESIGN.md ("Where the
// dispatch lives") says how to add a path.
#include <algorithm>

#include "conv.h"
#include "conv_h3.h"
#include "internal.h"
#include "nets.h"
#include "odu.h"
#include "resblk.h"
#include "siu.h"

using namespace mmla;

namespace {

ConvArgs conv_args(const ConvW& w, const float* x, float* y, int n, int h, int wd, int stride,
                   const BnW* bn, int pro, int epi, const float* res) {
  ConvArgs a{};
  a.x = x;
  a.wt = w.wt;
  a.bias = w.bias;
  a.scale = bn ? bn->scale : nullptr;
  a.shift = bn ? bn->shift : nullptr;
  a.res = res;
  a.y = y;
  a.n = n;
  a.h = h;
  a.w = wd;
  a.cin = w.cin;
  a.ho = (h + stride - 1) / stride;
  a.wo = (wd + stride - 1) / stride;
  a.cout = w.cout;
  a.cout_pad = w.cout_pad;
  a.ldy = w.cout;
  a.kh = w.kh;
  a.kw = w.kw;
  a.stride = stride;
  const int th = std::max((a.ho - 1) * stride + w.kh - h, 0);
  const int tw = std::max((a.wo - 1) * stride + w.kw - wd, 0);
  a.pad_h = th / 2;   // Keras 'same': extra padding goes after
  a.pad_w = tw / 2;
  a.pro = pro;
  a.epi = epi;
  return a;
}

double conv_flops(const ConvArgs& a) {
  return 2.0 * (double)a.n * a.ho * a.wo * a.kh * a.kw * a.cin * a.cout;
}

int conv_run(mmla_ctx* c, const ConvArgs& a, int stage = MMLA_STAGE_CONV) {
  LAUNCH(c, stage, conv_flops(a), conv_launch(a, c->stream));
  return MMLA_OK;
}

ConvH3Args conv_h3_args(const ConvW& w, const float* x, float* y, int n, int h, int wd, const BnW* bn,
                        int pro, int epi, const float* res, int* range_flag) {
  ConvH3Args a{};
  a.x = x;
  a.wh = w.wh;
  a.wl = w.wl;
  a.unscale = w.unscale();
  a.bias = w.bias;
  a.scale = bn ? bn->scale : nullptr;
  a.shift = bn ? bn->shift : nullptr;
  a.res = res;
  a.y = y;
  a.n = n;
  a.h = h;
  a.w = wd;
  a.cin = w.cin;
  a.cin_pad = w.cin_pad;
  a.cout = w.cout;
  a.cout_pad = w.cout_pad;
  a.kh = w.kh;
  a.kw = w.kw;
  a.pad_h = (w.kh - 1) / 2;   // Keras 'same', stride 1: extra padding after
  a.pad_w = (w.kw - 1) / 2;
  a.pro = pro;
  a.epi = epi;
  a.range_flag = range_flag;
  return a;
}

// spatial conv on the 3xFP16 path when enabled (falls back to the exact-f32 kernel otherwise);
// pool_out: write MaxPool2D(2,'same') of the output instead of the output (OD pool blocks).
// sc / sc_x (pool_out only): the block's shortcut Conv2D(1x1, stride 2) of sc_x, added to the pooled
// output inside the same launch
int conv_spatial(mmla_ctx* c, const Arith& ar, const ConvW& w, const float* x, float* y, int n, int h, int wd,
                 const BnW* bn, int pro, int epi, const float* res, bool pool_out = false,
                 int pool_in_h = 0, const ConvW* sc = nullptr, const float* sc_x = nullptr,
                 int sc_h = 0) {
  if (ar.h3() && w.wh) {
    ConvH3Args a = conv_h3_args(w, x, y, n, h, wd, bn, pro, epi, res, ar.range);
    double sc_flops = 0.0;
    if (sc && sc_x) {
      a.sc_x = sc_x;
      a.sc_wh = sc->wh;
      a.sc_wl = sc->wl;
      a.sc_bias = sc->bias;
      a.sc_cin = sc->cin;
      a.sc_h = sc_h;
      a.sc_unscale = sc->unscale();
      // pooled 2-D blocks: one output per pooled pixel; Conv1D: one per output row (h = rows)
      sc_flops = sc_h > 0 ? 2.0 * n * h * sc->cin * sc->cout
                          : 2.0 * n * ((h + 1) / 2) * ((wd + 1) / 2) * sc->cin * sc->cout;
    }
    a.pool_in = pool_in_h > 0;   // x = the unpooled [n, pool_in_h, 1, cin] (MaxPool1D fused)
    a.h_in = pool_in_h;
    a.pool_out = pool_out ? 1 : 0;
    LAUNCH(c, MMLA_STAGE_CONV, 2.0 * n * h * wd * w.kh * w.kw * w.cin * w.cout + sc_flops,
           conv_h3_launch(a, c->stream));
    return MMLA_OK;
  }
  ConvArgs a = conv_args(w, x, y, n, h, wd, 1, bn, pro, epi, res);
  if (!pool_out) return conv_run(c, a);
  return fail(c, MMLA_E_INVALID, "pooled epilogue needs the 3xFP16 conv path");
}

int ws_floats(mmla_ctx* c, int slot, size_t count, float** out) {
  void* p = nullptr;
  CHK(ws_get(c, slot, count * sizeof(float), &p));
  *out = static_cast<float*>(p);
  return MMLA_OK;
}

double lstm_flops(int64_t n, int T, int D) { return 2.0 * n * T * 2 * (256.0 + D) * 1024.0; }

// BiLSTM on the 3xFP16 path when enabled (exact-f32 MFMA kernel otherwise)
hipError_t lstm_run(mmla_ctx* c, const Arith& ar, const LstmW& L, const float* seq, int64_t n, int T, float* out) {
  if (ar.h3() && L.wth[0] && ar.split &&
      n <= std::min(c->lstm_split_max, bilstm_h3_split_max_clips())) {
    void* ws = nullptr;   // small batches (the real-time calls): each direction over eight CUs
    if (ws_get(c, S_LSTM, bilstm_h3_split_ws_bytes(), &ws) != MMLA_OK) return hipErrorOutOfMemory;
    return bilstm_h3_split_launch(seq, (int)n, T, 128, L.wth[0], L.wtl[0], L.wth[1], L.wtl[1],
                                  L.bias[0], L.bias[1], out, ar.range, L.ws[0], L.ws[1], ws,
                                  ar.timeout, c->lstm_spin, c->stream);
  }
  if (ar.h3() && L.wth[0])
    return bilstm_h3_launch(seq, (int)n, T, 128, L.wth[0], L.wtl[0], L.wth[1], L.wtl[1], L.bias[0],
                            L.bias[1], out, ar.range, L.ws[0], L.ws[1], c->stream);
  return bilstm_launch(seq, (int)n, T, 128, L.wcat[0], L.wcat[1], L.bias[0], L.bias[1], out,
                       c->stream);
}

// ---- OD-NET: which kernel runs res block b ---------------------------------------------------------

enum OdPath {
  OD_STRIPS,   // rbs.hip: the whole block, rolling down 16-column strips (conv_h3 weight layout)
  OD_TILES,    // resblk.hip: the whole block on 16 x 16 tiles (fused fragment layout)
  OD_ODU,      // odu.hip: the whole block, blocks 4-9
  OD_PAIR      // conv_h3 / exact-f32 launches, one per conv
};
struct OdChoice {
  OdPath path;
  // block 1 only: Conv2D(16, 1x1) on the PNG image (overlap_detector_temp.py:282) computed inside
  // the block's staging (rbs.hip / resblk.hip STEM) instead of as its own launch
  bool stem;
  // OD_ODU only: strips per workgroup, two for the blocks that are faster so (odu_two_strips)
  int strips;
  // OD_STRIPS only: blocks 2-3 with the 3x3 conv's weights in LDS (rbs_w1l.hip)
  bool w1_lds;
  // OD_STRIPS only: block 1 with the clips' ragged last strips paired (rbs_tp.hip)
  bool tail_pair;
};

bool strips_ok(const ResUnitW& B, bool pool, int h, int w) {
  return B.ca.wh && B.cb.wh && (!pool || B.sc.wh) && B.ca.cin_pad == B.ca.cin && B.ca.cout_pad == 32 &&
         B.cb.cin_pad == 32 && B.cb.cout_pad == 32 && B.cb.kh == 4 && B.cb.kw == 1 &&
         (!pool || (B.sc.cin_pad == B.ca.cin && B.sc.cout_pad == 32)) &&
         rbs_supported(h, w, B.ca.cin, B.ca.cout, pool);
}

bool tiles_ok(const ResUnitW& B, bool pool) {
  return B.ca.fh && B.cb.fh && B.cb.kpad == 4 * B.cb.cin && (!pool || B.sc.fh) &&
         resblk_supported(B.ca.cin, B.ca.cout, pool);
}

bool odu_ok(const ResUnitW& B, bool pool, int h, int w) {
  return B.ca.wh && B.cb.wh && (!pool || B.sc.wh) && odu_supported(h, w, B.ca.cin, B.ca.cout, pool) &&
         B.ca.cin_pad == B.ca.cin && B.ca.cout_pad == B.ca.cout && B.cb.cin == B.ca.cout &&
         B.cb.cout == B.ca.cout && B.cb.cin_pad == B.cb.cin && B.cb.cout_pad == B.cb.cout &&
         B.cb.kh == 4 && B.cb.kw == 1 &&
         (!pool || (B.sc.cin == B.ca.cin && B.sc.cout == B.ca.cout && B.sc.cout_pad == B.sc.cout));
}

// stop: the debug trace's last stage (-1: none); a trace of the stem alone (0) needs it in HBM
OdChoice od_choose(const mmla_ctx* c, const Arith& ar, const ResUnitW& B, int b, int h, int w, int stop) {
  OdChoice k{OD_PAIR, false, 1, false, false};
  if (!ar.h3()) return k;
  if (c->rbs && strips_ok(B, POOL[b], h, w)) {
    k.path = OD_STRIPS;
    k.w1_lds = c->rbs_w1l && !POOL[b];
    k.tail_pair = c->rbs_tailpair && POOL[b];
  } else if (tiles_ok(B, POOL[b])) {
    k.path = OD_TILES;
  } else if (c->odu && odu_ok(B, POOL[b], h, w)) {
    k.path = OD_ODU;
    k.strips = c->odw && odu_two_strips(h, w, B.ca.cin, B.ca.cout, POOL[b]) ? 2 : 1;
  }
  k.stem = b == 0 && stop != 0 && (k.path == OD_STRIPS || k.path == OD_TILES);
  return k;
}

// fused: read the fused fragment layout fh/fl (tiles) instead of the conv_h3 layout wh/wl (strips);
// stem != null: block 1 reads the image (u8, else f32) through the stem instead of x
ResBlkArgs resblk_args(const ResUnitW& B, bool pool, bool fused, const float* x, float* y, int64_t n,
                       int h, int w, int* range_flag, const ConvW* stem, const uint8_t* img_u8,
                       const float* img_f32) {
  ResBlkArgs r{};
  r.x = x;
  r.y = y;
  r.w1h = fused ? B.ca.fh : B.ca.wh;
  r.w1l = fused ? B.ca.fl : B.ca.wl;
  r.b1 = B.ca.bias;
  r.u1 = B.ca.unscale();
  r.s1 = B.bn_in.scale;
  r.t1 = B.bn_in.shift;
  r.w2h = fused ? B.cb.fh : B.cb.wh;
  r.w2l = fused ? B.cb.fl : B.cb.wl;
  r.b2 = B.cb.bias;
  r.u2 = B.cb.unscale();
  r.s2 = B.bn_mid.scale;
  r.t2 = B.bn_mid.shift;
  if (pool) {
    r.wsh = fused ? B.sc.fh : B.sc.wh;
    r.wsl = fused ? B.sc.fl : B.sc.wl;
    r.bs = B.sc.bias;
    r.us = B.sc.unscale();
  }
  if (stem) {
    r.x = nullptr;
    r.img8 = img_u8;
    r.imgf = img_u8 ? nullptr : img_f32;
    r.wst = stem->wt;
    r.bst = stem->bias;
    r.ldst = stem->cout_pad;
  }
  r.n = (int)n;
  r.h = h;
  r.w = w;
  r.range_flag = range_flag;
  return r;
}

OduArgs odu_args(const ResUnitW& B, bool pool, const float* x, float* y, int64_t n, int* range_flag) {
  OduArgs o{};
  o.x = x;
  o.y = y;
  o.wah = B.ca.wh;
  o.wal = B.ca.wl;
  o.wbh = B.cb.wh;
  o.wbl = B.cb.wl;
  o.ba = B.ca.bias;
  o.bb = B.cb.bias;
  o.s_in = B.bn_in.scale;
  o.t_in = B.bn_in.shift;
  o.s_mid = B.bn_mid.scale;
  o.t_mid = B.bn_mid.shift;
  o.ua = B.ca.unscale();
  o.ub = B.cb.unscale();
  o.n = (int)n;
  o.range_flag = range_flag;
  if (pool) {
    o.wsh = B.sc.wh;
    o.wsl = B.sc.wl;
    o.bs = B.sc.bias;
    o.us = B.sc.unscale();
  }
  return o;
}

// a whole res block in one launch: both convs at (h, w), the pool blocks' shortcut at the pooled size
double od_block_flops(const ResUnitW& B, bool pool, int64_t n, int h, int w) {
  return 2.0 * n * h * w * (9.0 * B.ca.cin * B.ca.cout + 4.0 * B.cb.cin * B.cb.cout) +
         (pool ? 2.0 * n * ((h + 1) / 2) * ((w + 1) / 2) * B.sc.cin * B.sc.cout : 0.0);
}

// the block as one launch per conv: X -> T1 -> the result, which is X itself for an identity block
// (the residual is added in place) and T1 for a pool block (T2 holds the unpooled or pooled conv(4,1))
int od_block_pair(mmla_ctx* c, const Arith& ar, const ResUnitW& B, bool pool, int n, int h, int w, float* X,
                  float*& T1, float*& T2, float** out) {
  CHK(conv_spatial(c, ar, B.ca, X, T1, n, h, w, &B.bn_in, PRO_BN_ELU, EPI_BIAS, nullptr));
  if (!pool) {
    *out = X;
    return conv_spatial(c, ar, B.cb, T1, X, n, h, w, &B.bn_mid, PRO_BN_ELU, EPI_ADD, X);
  }
  if (!ar.h3()) {
    CHK(conv_spatial(c, ar, B.cb, T1, T2, n, h, w, &B.bn_mid, PRO_BN_ELU, EPI_BIAS, nullptr));
    // shortcut Conv2D(1x1, stride 2) + MaxPool2D(2, 'same')(t2), fused
    ConvArgs s = conv_args(B.sc, X, T1, n, h, w, 2, nullptr, PRO_NONE, EPI_ADD_POOL, T2);
    s.hp = h;
    s.wp = w;
    CHK(conv_run(c, s));
  } else if (B.sc.wh && B.sc.cout == B.cb.cout && B.cb.cout_pad == B.sc.cout_pad) {
    // conv(4,1) + MaxPool2D(2,'same') + the shortcut Conv2D(1x1, stride 2) of X + Add, one launch
    CHK(conv_spatial(c, ar, B.cb, T1, T2, n, h, w, &B.bn_mid, PRO_BN_ELU, EPI_BIAS, nullptr, true, 0, &B.sc,
                     X));
    std::swap(T1, T2);
  } else {
    // conv(4,1) with MaxPool2D(2,'same') fused into its epilogue -> T2 at half resolution;
    // then shortcut Conv2D(1x1, stride 2) + pooled T2
    CHK(conv_spatial(c, ar, B.cb, T1, T2, n, h, w, &B.bn_mid, PRO_BN_ELU, EPI_BIAS, nullptr, true));
    CHK(conv_run(c, conv_args(B.sc, X, T1, n, h, w, 2, nullptr, PRO_NONE, EPI_ADD, T2)));
  }
  *out = T1;
  return MMLA_OK;
}

}  // namespace

namespace mmla __attribute__((visibility("hidden"))) {

// OD-NET on a device batch; input = uint8 image (img_u8) or float NHWC (img_f32).
// `stop` >= 0 (debug trace): return after stage `stop` (0 stem, 1..9 res blocks, 10 mean, 11
// BiLSTM) with *tap / *tap_n set to that stage's output tensor.
int run_od_net(mmla_ctx* c, const Arith& ar, const uint8_t* img_u8, const float* img_f32, int64_t n,
               float* probs, int32_t* argmax, OdGate gate, int stop, const float** tap, int64_t* tap_n) {
  const OdNet& W = c->od;
  const size_t big = (size_t)n * OD_PIX * 32;
  float *X, *T1, *T2, *SEQ, *H;
  CHK(ws_floats(c, S_X, big, &X));
  CHK(ws_floats(c, S_T1, big, &T1));
  CHK(ws_floats(c, S_T2, big, &T2));
  CHK(ws_floats(c, S_SEQ, (size_t)n * 19 * 128, &SEQ));
  CHK(ws_floats(c, S_HOUT, (size_t)n * 512, &H));
  const double stem_flops = 2.0 * n * OD_PIX * 3 * 16;
  const OdChoice first = od_choose(c, ar, W.blk[0], 0, OD_H, OD_W, stop);
  if (!first.stem)
    LAUNCH(c, MMLA_STAGE_GLUE, stem_flops,
           od_stem_launch(img_u8, img_f32, n * OD_PIX, W.stem.cout_pad, W.stem.wt, W.stem.bias, X,
                          c->stream));
  int h = OD_H, w = OD_W;
  if (stop == 0) {
    *tap = X;
    *tap_n = n * OD_PIX * 16;
    return MMLA_OK;
  }
  for (int b = 0; b < 9; ++b) {   // res_block, overlap_detector_temp.py:253-277
    const ResUnitW& B = W.blk[b];
    const bool pool = POOL[b];
    const OdChoice k = b == 0 ? first : od_choose(c, ar, B, b, h, w, stop);
    // a fused stem's FLOPs are booked with the block that computes it
    const double flops = od_block_flops(B, pool, n, h, w) + (k.stem ? stem_flops : 0.0);
    float* out = T1;   // where the block's output lands
    switch (k.path) {
      case OD_STRIPS:
      case OD_TILES: {
        const bool tiles = k.path == OD_TILES;
        const ResBlkArgs r = resblk_args(B, pool, tiles, X, T1, n, h, w, ar.range,
                                         k.stem ? &W.stem : nullptr, img_u8, img_f32);
        LAUNCH(c, MMLA_STAGE_CONV, flops,
               tiles ? resblk_launch(r, B.ca.cin, B.ca.cout, pool, c->stream)
                     : rbs_launch(r, B.ca.cin, B.ca.cout, pool, k.w1_lds, k.tail_pair, c->stream));
        break;
      }
      case OD_ODU: {   // t1 stays in LDS, bit-identical to the pair
        const OduArgs o = odu_args(B, pool, X, T1, n, ar.range);
        LAUNCH(c, MMLA_STAGE_CONV, flops,
               odu_launch(o, h, w, B.ca.cin, B.ca.cout, pool, k.strips, c->stream));
        break;
      }
      case OD_PAIR:
        CHK(od_block_pair(c, ar, B, pool, (int)n, h, w, X, T1, T2, &out));
        break;
    }
    // the tail every block runs through: pooled size, the output becomes X, trace tap
    if (pool) {
      h = (h + 1) / 2;
      w = (w + 1) / 2;
    }
    if (out != X) std::swap(X, T1);
    if (stop == b + 1) {
      *tap = X;
      *tap_n = n * h * w * CH[b];
      return MMLA_OK;
    }
  }
  // h = 16, w = 19, c = 128: Lambda(K.mean(x, axis=1)) -> [n, 19, 128]
  LAUNCH(c, MMLA_STAGE_GLUE, (double)n * h * w * 128,
         mean_h_launch(X, (int)n, h, w, 128, SEQ, c->stream));
  if (stop == 10) {
    *tap = SEQ;
    *tap_n = n * w * 128;
    return MMLA_OK;
  }
  LAUNCH(c, MMLA_STAGE_LSTM, lstm_flops(n, w, 128),
         lstm_run(c, ar, W.lstm, SEQ, n, w, H));
  if (stop == 11) {
    *tap = H;
    *tap_n = n * 512;
    return MMLA_OK;
  }
  LAUNCH(c, MMLA_STAGE_HEAD, 2.0 * n * 512 * W.k,
         od_head_launch(H, (int)n, W.k, W.head_w, W.head_b, probs, argmax,
                        gate.lens, gate.clip_len, gate.silent, gate.ssim, gate.ssim_threshold,
                        c->stream));
  return MMLA_OK;
}

}  // namespace mmla

// ---- SI-NET ----------------------------------------------------------------------------------------

namespace {

// a res unit without pooling that siu.hip runs (3xFP16 weights of the exact widths)
bool siu_ok(const ResUnitW& U, int cin) {
  return U.ca.wh && U.cb.wh && siu_chain_supported(cin, cin, false, 1, false) && U.ca.cin == cin &&
         U.ca.cout == cin && U.cb.cin == cin && U.cb.cout == cin && U.ca.cin_pad == cin && U.ca.cout_pad == cin &&
         U.cb.cout_pad == cin;
}

// ... and a pool unit (siu.hip POOL)
bool sipu_ok(const ResUnitW& U, int cin) {
  return U.ca.wh && U.cb.wh && U.sc.wh && siu_chain_supported(cin, U.ca.cout, true, 1, false) &&
         U.ca.cin_pad == cin && U.ca.cout_pad == U.ca.cout && U.cb.cin == U.ca.cout && U.cb.cout == U.ca.cout &&
         U.cb.cout_pad == U.ca.cout && U.sc.cin == cin && U.sc.cout == U.ca.cout &&
         U.sc.cout_pad == U.ca.cout;
}

// how many units the siu.hip launch that starts at unit u covers: a pool unit with the two units
// after it or alone, two units without pooling or one; 0: the unit runs as conv_h3 / exact-f32 launches
int si_choose(const mmla_ctx* c, const Arith& ar, const SiNet& W, int u) {
  if (!c->siu || !ar.h3()) return 0;
  const int cin = W.unit[u].ca.cin, C = W.unit[u].ca.cout;
  auto plain = [&](int v) { return v < 9 && !POOL[v] && siu_ok(W.unit[v], C); };
  if (POOL[u]) {
    if (!c->sipu || !sipu_ok(W.unit[u], cin)) return 0;
    return c->sichain && siu_chain_supported(cin, C, true, 3, false) && plain(u + 1) && plain(u + 2) ? 3 : 1;
  }
  if (!siu_ok(W.unit[u], cin)) return 0;
  return c->sipair && siu_chain_supported(cin, cin, false, 2, false) && plain(u + 1) ? 2 : 1;
}

// a whole res unit at t (pooled) rows per clip: both convs, and the pool units' shortcut
double si_unit_flops(const ResUnitW& U, bool pool, int64_t n, int t) {
  return 2.0 * n * t *
         (3.0 * U.ca.cin * U.ca.cout + 3.0 * U.cb.cin * U.cb.cout + (pool ? 1.0 * U.sc.cin * U.sc.cout : 0.0));
}

// t: the unit's rows.  t_src > 0: a pool unit reading t_src rows through MaxPool1D, with its shortcut
SiuArgs siu_args(const ResUnitW& U, const float* x, float* y, int64_t n, int t, int* range_flag,
                 int t_src = 0) {
  SiuArgs s{};
  s.n = (int)n;
  s.t = t;
  s.range_flag = range_flag;
  s.x = x;
  s.y = y;
  s.wah = U.ca.wh;
  s.wal = U.ca.wl;
  s.wbh = U.cb.wh;
  s.wbl = U.cb.wl;
  s.ba = U.ca.bias;
  s.bb = U.cb.bias;
  s.s_in = U.bn_in.scale;
  s.t_in = U.bn_in.shift;
  s.s_mid = U.bn_mid.scale;
  s.t_mid = U.bn_mid.shift;
  s.ua = U.ca.unscale();
  s.ub = U.cb.unscale();
  if (t_src > 0) {
    s.t_src = t_src;
    s.wsh = U.sc.wh;
    s.wsl = U.sc.wl;
    s.bs = U.sc.bias;
    s.us = U.sc.unscale();
  }
  return s;
}

}  // namespace

namespace mmla __attribute__((visibility("hidden"))) {

// ldx: the features' row stride (39, or 40 from si_fe with a zero 40th column: the stem then stages
// 16-B aligned rows, conv_h3's float4 path, bit-identical -- its weights' padded channels are zero)
// `stop` >= 0: return after stage `stop` (0 stem, 1..9 res units, 10 final BN + ReLU + AvgPool4, 11
// BiLSTM = base_model.layers[-2].output, mmla_si_embed's; 12 the logits, rows of cout_pad floats) with
// *tap / *tap_n (nullable) set to that stage's output tensor.  The launches are the ones the context's
// switches select whatever `stop` is: a stage that such a launch keeps on chip is MMLA_E_INVALID
int run_si_net(mmla_ctx* c, const Arith& ar, const float* x, int64_t n, float* probs, int32_t* argmax,
               const uint8_t* silent, int ldx, int stop, const float** tap, int64_t* tap_n) {
  const SiNet& W = c->si;
  auto stopped = [&](const float* p, int64_t floats) {
    *tap = p;
    if (tap_n) *tap_n = floats;
    return MMLA_OK;
  };
  if (stop >= 0 && !tap) return fail(c, MMLA_E_INVALID, "SI stop stage without a tap");
  const size_t big = (size_t)n * SI_T * 32;
  float *X, *T1, *XP, *R, *SEQ, *H, *L;
  CHK(ws_floats(c, S_X, big, &X));
  CHK(ws_floats(c, S_T1, big, &T1));
  CHK(ws_floats(c, S_T2, big, &XP));
  CHK(ws_floats(c, S_T3, big, &R));
  CHK(ws_floats(c, S_SEQ, (size_t)n * 8 * 128, &SEQ));
  CHK(ws_floats(c, S_HOUT, (size_t)n * 512, &H));
  CHK(ws_floats(c, S_LOGIT, (size_t)n * W.dense.cout_pad, &L));
  int t = SI_T;
  const bool h3 = ar.h3();
  bool fused_final = false;   // the last unit wrote BN + ReLU + AvgPool4 itself (siu FIN)
  // Conv1D(32, 4, same): [n, 256, 1, 39] -> [n, 256, 1, 32] (speaker_identification.py:195)
  ConvW stem = W.stem;
  if (ldx == SI_D + 1 && h3 && stem.wh && stem.cin_pad > SI_D) stem.cin = ldx;
  else if (ldx != SI_D) return fail(c, MMLA_E_INVALID, "padded SI features need the 3xFP16 stem");
  CHK(conv_spatial(c, ar, stem, x, X, (int)n, t, 1, nullptr, PRO_NONE, EPI_BIAS, nullptr));
  if (stop == 0) return stopped(X, n * t * W.stem.cout);
  for (int u = 0; u < 9; ++u) {   // res_unit, speaker_identification.py:168-190
    const ResUnitW& U = W.unit[u];
    const int cin = U.ca.cin;
    const bool pool = POOL[u];
    const int tp = pool ? (t + 1) / 2 : t;
    const int units = si_choose(c, ar, W, u);
    float* out = R;   // where the unit's (or the chain's) output lands
    if (units > 0) {
      // the units in one launch (siu.hip): MaxPool1D in the staging, every t1 and the outputs between
      // units on chip, the shortcut in the epilogue, bit-identical to the conv_h3 launches below
      const int C = U.ca.cout;
      SiuArgs s[3];
      double flops = 0.0;
      for (int k = 0; k < units; ++k) {
        const bool first = k == 0;
        s[k] = siu_args(W.unit[u + k], first ? X : nullptr, k == units - 1 ? R : nullptr, n, tp, ar.range,
                        first && pool ? t : 0);
        flops += si_unit_flops(W.unit[u + k], first && pool, n, tp);
      }
      // a launch that ends with unit 9: + the final BN + ReLU + AveragePooling1D(4) in its epilogue,
      // so the unit's output never reaches HBM (bit-identical to bn_relu_avgpool4_launch below)
      if (u + units == 9 && c->sifin && tp % 4 == 0 && siu_chain_supported(cin, C, pool, units, true)) {
        SiuArgs& last = s[units - 1];
        last.y = nullptr;
        last.seq = SEQ;
        last.fs = W.final_bn.scale;
        last.ft = W.final_bn.shift;
        fused_final = true;
      }
      // the trace's stage inside this launch: the outputs between its units, and unit 9's under a fused
      // final epilogue, never reach memory
      if (stop > u && stop < u + units)
        return fail(c, MMLA_E_INVALID, "SI stage %d stays on chip: one siu chain launch runs units %d-%d",
                    stop, u + 1, u + units);
      if (stop == 9 && fused_final)
        return fail(c, MMLA_E_INVALID, "SI stage 9 stays on chip: the siu chain launch of units %d-9 writes "
                    "the final BN + ReLU + AvgPool4 instead (MMLA_NO_SIFIN unset)", u + 1);
      LAUNCH(c, MMLA_STAGE_CONV, flops, siu_chain_launch(s, units, pool, cin, C, c->stream));
      u += units - 1;
    } else if (pool) {
      if (h3 && U.ca.wh) {
        // MaxPool1D(2, same) taken inside the conv's staging (conv_h3.hip PIN)
        CHK(conv_spatial(c, ar, U.ca, X, T1, (int)n, tp, 1, &U.bn_in, PRO_BN_RELU, EPI_BIAS, nullptr,
                         false, t));
      } else {
        LAUNCH(c, MMLA_STAGE_GLUE, (double)n * t * cin,
               maxpool_t2_launch(X, (int)n, t, cin, XP, c->stream));
        CHK(conv_spatial(c, ar, U.ca, XP, T1, (int)n, tp, 1, &U.bn_in, PRO_BN_RELU, EPI_BIAS, nullptr));
      }
      if (h3 && U.cb.wh && U.sc.wh && U.sc.cout == U.cb.cout && U.sc.cout_pad == U.cb.cout_pad) {
        // Conv1D(3) + the shortcut Conv1D(1, stride 2) of X as its residual + Add, one launch
        CHK(conv_spatial(c, ar, U.cb, T1, R, (int)n, tp, 1, &U.bn_mid, PRO_BN_RELU, EPI_ADD, nullptr, false,
                         0, &U.sc, X, t));
      } else {
        CHK(conv_run(c, conv_args(U.sc, X, R, (int)n, t, 1, 2, nullptr, PRO_NONE, EPI_BIAS, nullptr)));
        CHK(conv_spatial(c, ar, U.cb, T1, R, (int)n, tp, 1, &U.bn_mid, PRO_BN_RELU, EPI_ADD, R));
      }
    } else {
      CHK(conv_spatial(c, ar, U.ca, X, T1, (int)n, t, 1, &U.bn_in, PRO_BN_RELU, EPI_BIAS, nullptr));
      CHK(conv_spatial(c, ar, U.cb, T1, X, (int)n, t, 1, &U.bn_mid, PRO_BN_RELU, EPI_ADD, X));
      out = X;
    }
    // the tail every unit runs through: the output becomes X, pooled rows
    if (out != X) std::swap(X, R);
    t = tp;
    if (stop == u + 1) return stopped(X, n * t * W.unit[u].cb.cout);
  }
  // t = 32, c = 128 -> BN -> ReLU -> AvgPool1D(4) -> [n, 8, 128] (speaker_identification.py:208-212)
  if (!fused_final)
    LAUNCH(c, MMLA_STAGE_GLUE, 3.0 * n * t * 128,
           bn_relu_avgpool4_launch(X, (int)n, t, 128, W.final_bn.scale, W.final_bn.shift,
                                   SEQ, c->stream));
  if (stop == 10) return stopped(SEQ, n * (t / 4) * 128);
  LAUNCH(c, MMLA_STAGE_LSTM, lstm_flops(n, t / 4, 128),
         lstm_run(c, ar, W.lstm, SEQ, n, t / 4, H));
  if (stop == 11) return stopped(H, n * 512);   // mmla_si_embed: the BiLSTM output itself, no Dense, no head
  if (h3 && W.dense.wh && W.dense.cin % 32 == 0) {
    // Dense(K) as a 1x1 conv over the clips on the 3xFP16 path (conv_h3 Conv1D tiles of 128 clips):
    // all cout_pad columns are written (the padding columns: zero weights and bias), so the logits
    // keep the cout_pad row stride the head reads
    ConvH3Args a = conv_h3_args(W.dense, H, L, (int)n, 1, 1, nullptr, PRO_NONE, EPI_BIAS, nullptr,
                                ar.range);
    a.cout = W.dense.cout_pad;
    LAUNCH(c, MMLA_STAGE_HEAD, 2.0 * n * W.dense.cin * W.dense.cout, conv_h3_launch(a, c->stream));
  } else {
    ConvArgs d = conv_args(W.dense, H, L, (int)n, 1, 1, 1,
                           nullptr, PRO_NONE, EPI_BIAS, nullptr);
    d.ldy = W.dense.cout_pad;
    CHK(conv_run(c, d, MMLA_STAGE_HEAD));
  }
  if (stop == 12) return stopped(L, n * W.dense.cout_pad);
  LAUNCH(c, MMLA_STAGE_HEAD, 4.0 * n * W.k,
         si_head_launch(L, (int)n, W.k, W.dense.cout_pad, W.head, probs,
                        argmax, silent, c->stream));
  return MMLA_OK;
}

}  // namespace mmla
