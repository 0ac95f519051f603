// libmmla internals shared by the C ABI's translation units: the context, the weight structs, the
// workspace slots and the error / launch macros.
//   context.cpp      context, profiler, workspace; create / destroy / setters / profile entry points
//   weights.cpp      take_*, mmla_load_weights
//   net_runners.cpp  conv_spatial, lstm_run, run_od_net, run_si_net (which kernel runs which block), each in
//                    the arithmetic of its Arith argument
//   pipeline.cpp     staging, micro-batching, the range guard (it builds each pass's Arith); feature /
//                    forward / pipeline entry points
//   capi.cpp         the auxiliary entry points and the head trainer (mmla_si_head_fit)
//   fit_common.h     what the trainers share, host code only: Carver / carve_slot, staged operands (Stager),
//                    check_perm / check_labels, wire_lstm / mark_trainable and the fit driver (fit_check, fit)
//   si_finetune.cpp  SI-NET's engine over si_bwd.hip and, with `base`, si_base.hip; one loss-grad body
//                    (mmla_si_loss_grad, mmla_si_base_loss_grad) and one set of fit callables (mmla_si_finetune,
//                    mmla_si_base_train) for the driver; mmla_si_base_drop_mask
//   od_finetune.cpp  OD-NET's engine over conv.hip, od_bwd.hip, si_bwd.hip; mmla_od_loss_grad, and one set of
//                    fit callables (mmla_od_finetune, mmla_od_train) for the driver; mmla_od_drop_mask,
//                    mmla_od_auc, mmla_od_augment (od_aug.hip)
// All but mmla_ctx (the type include/mmla.h names) lives in namespace mmla, which is not exported.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mmla.h"
#include "nr.h"
#include "od_fe.h"
#include "mix.h"
#include "si_fe.h"
#include "ssim.h"
#include "vad.h"

namespace mmla __attribute__((visibility("hidden"))) {

constexpr int OD_H = 128, OD_W = 151, OD_PIX = OD_H * OD_W;
constexpr int OD_IMG = OD_PIX * 3;
constexpr int SI_T = 256, SI_D = 39;
constexpr int SI_NEED_SAMPLES = 160 * 259 + 400;   // frames 0..259 (delta-delta reach)
constexpr int CH[9] = {32, 32, 32, 64, 64, 64, 128, 128, 128};
constexpr bool POOL[9] = {true, false, false, true, false, false, true, false, false};

// floats of the packed OD blob (weights.od_spec(K)): everything below the Dense head, then kernel [512, K], bias [K]
constexpr int64_t od_body_floats() {
  int64_t n = 3 * 16 + 16;
  int cin = 16;
  for (int u = 0; u < 9; ++u) {
    const int ch = CH[u];
    n += 4 * cin + (9 * cin * ch + ch) + 4 * ch + (4 * ch * ch + ch) + (POOL[u] ? cin * ch + ch : 0);
    cin = ch;
  }
  return n + 2 * ((128 + 256) * 1024 + 1024);
}
constexpr int64_t od_blob_floats(int k, int channels = 3) {
  return od_body_floats() + 513 * (int64_t)k - (channels == 1 ? 32 : 0);   // stem kernel [1,1,C,16]
}
static_assert(od_blob_floats(2) == 1548706, "the two-class OD blob");

struct ConvW {
  float* wt = nullptr;
  float* bias = nullptr;
  uint16_t* wh = nullptr;   // 3xFP16 split weights [tap][cout_pad][cin_pad] (spatial convs only)
  uint16_t* wl = nullptr;
  uint16_t* fh = nullptr;   // fused res_block layout [cout][kpad], k = tap * cin + ci (resblk.hip)
  uint16_t* fl = nullptr;
  int kh = 0, kw = 0, cin = 0, cout = 0, cout_pad = 0, cin_pad = 0, kpad = 0;
  float wscale = 256.0f;    // power-of-two scale of the fp16 hi/lo split (pick_wscale)
  float unscale() const { return 1.0f / (16.0f * wscale); }   // x the 2^4 activation scale
};
struct BnW {
  float* scale = nullptr;
  float* shift = nullptr;
  int c = 0;
};
struct LstmW {
  float* wcat[2] = {nullptr, nullptr};
  float* bias[2] = {nullptr, nullptr};
  uint16_t* wth[2] = {nullptr, nullptr};   // 3xFP16 split, transposed [1024][256 + D] (nets.hip)
  uint16_t* wtl[2] = {nullptr, nullptr};
  float ws[2] = {256.0f, 256.0f};          // per-direction split scale (pick_wscale)
};
// one res unit of either network: BN -> act -> ca -> BN -> act -> cb (+ sc, the 1x1 stride-2 shortcut
// of the pool units).  OD: ca = Conv2D(3x3), cb = Conv2D((4,1)); SI: both Conv1D(3)
struct ResUnitW {
  BnW bn_in, bn_mid;
  ConvW ca, cb, sc;
};
struct OdNet {
  ConvW stem;
  ResUnitW blk[9];
  LstmW lstm;
  float* head_w = nullptr;   // Dense [512, k]
  float* head_b = nullptr;
  int k = 2;                 // classes of the loaded head, 2 .. MMLA_OD_MAX_CLASSES
  // channels of the blob's stem kernel [1,1,C,16], 3 or 1.  The device-side image has 3 bytes per pixel
  // either way: a one-channel stem is stored as rows {w, 0, 0} and reads the pixel (g, g, g)
  int channels = 3;
};
struct SiNet {
  ConvW stem;
  ResUnitW unit[9];
  BnW final_bn;
  LstmW lstm;
  ConvW dense;
  int k = 0, head = 0;
};

struct ProfRec {
  int stage;
  hipEvent_t a, b;
  double work;
};

// Micro-batch caps (clips per internal pass).  The default (mmla_set_microbatch 0) is sized from
// the device's free memory at call time, capped here: 16384 OD clips = 124 GB of activations
// (4096: -2.4 % clips/s), 65536 SI clips = 9 GB (16384: -4 %).  A micro-batch whose workspace
// allocation fails is halved and retried (down to kMinMicrobatch) instead of failing the call.
constexpr int64_t kOdMicrobatch = 16384;
constexpr int64_t kSiMicrobatch = 65536;
constexpr int64_t kMinMicrobatch = 64;

// host-pinned staging of small host-pointer calls (mmla_ctx::pin_small)
constexpr size_t kPinSlotBytes = 64u << 10;
constexpr size_t kPinInBytes = 1u << 20;
constexpr int kPinSlots = 4;   // S_OUT0 .. S_OUT3

// the words of mmla_ctx::range_dev: an operand outside the fp16 range, or a split-BiLSTM workgroup that
// gave up waiting, in a device-pointer call (sticky until mmla_range_check) or in the current pass of a
// host-pointer micro-batch (pipeline.cpp guarded(): re-run); the two host words are neighbours
enum RangeWord { RW_DEV_RANGE = 0, RW_HOST_RANGE, RW_HOST_TIMEOUT, RW_DEV_TIMEOUT, RW_COUNT };

}  // namespace mmla

struct mmla_ctx {
  bool prof_on = false;
  std::vector<mmla::ProfRec> prof_pending;
  std::vector<hipEvent_t> prof_pool;
  double prof_ms[MMLA_NSTAGES] = {0};
  double prof_work[MMLA_NSTAGES] = {0};
  int64_t prof_n[MMLA_NSTAGES] = {0};
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t own_stream = nullptr;
  std::string err;
  OdFeTables* od_tables = nullptr;
  SiFeTables* si_tables = nullptr;
  bool od_loaded = false, si_loaded = false;
  // the image the front-end makes in front of OD-NET (MMLA_OD_IMG_*): a property of the loaded OD model,
  // reset by mmla_load_weights, changed by mmla_od_set_image_type
  int od_img_type = MMLA_OD_IMG_ZCR;
  mmla::OdNet od;
  mmla::SiNet si;
  std::vector<void*> od_allocs, si_allocs;
  // the SI Dense head's tensors, apart from the frozen base's in si_allocs: mmla_si_set_head frees and
  // replaces them alone
  std::vector<void*> si_head_allocs;
  std::vector<void*> ws;
  std::vector<size_t> ws_size;
  std::vector<size_t> ws_guard;   // MMLA_WS_GUARD: guard bytes before and after each slot (0 = none)
  int64_t od_mb = 0, si_mb = 0;            // user caps (0 = sized from free memory)
  int64_t od_mb_cap = mmla::kOdMicrobatch, si_mb_cap = mmla::kSiMicrobatch;   // default caps of the automatic size
  int debug_fail_allocs = 0;   // test hook (env MMLA_DEBUG_FAIL_ALLOC at create): fail this many workspace allocations
  int debug_trace_guard = 0;   // test hook (env MMLA_DEBUG_TRACE_GUARD at create): mmla_debug_od_trace / _si_trace under the range guard
  int precision = MMLA_PREC_F16X3;   // mmla_set_precision: the user's setting (a pass runs its Arith)
  // SI res units as fused launches of siu.hip's one template, siu_chain_kernel<..., POOL, NU, FIN, ...>
  // (net_runners.cpp si_choose); env MMLA_NO_SIU=1 at create: two conv_h3 launches per unit (A/B)
  bool siu = true;
  // ... and the pool units too (POOL); env MMLA_NO_SIPU=1 at create: the conv_h3 pair
  bool sipu = true;
  // ... and the last one with the final BN + ReLU + AvgPool4 (FIN); env MMLA_NO_SIFIN=1: the unit
  // writes its output and bn_relu_avgpool4 runs as its own launch
  bool sifin = true;
  // ... and two consecutive units without pooling (2-3, 5-6, 8-9) in one launch (NU = 2: the first
  // unit's output stays on chip); env MMLA_NO_SIPAIR=1: one launch each (NU = 1)
  bool sipair = true;
  // ... and a pool unit with the two units after it (1-3, 4-6, 7-9) in one launch (POOL, NU = 2); env
  // MMLA_NO_SICHAIN=1: the pool unit alone (POOL, NU = 0), then the pair
  bool sichain = true;
  // fused SI pipeline: si_fe writes 40-float feature rows for the stem (env MMLA_NO_SIPAD=1: 39)
  bool si_pad_feat = true;
  // OD blocks 4-9 as one fused kernel each (odu.hip: t1 on chip); env MMLA_NO_ODU=1 at create: the
  // conv_h3 pairs (A/B, bit-identical)
  bool odu = true;
  // ... with two strips per workgroup on one weight stream where that measured faster (odu.hip
  // odu_two_strips); env MMLA_NO_ODW=1 at create: one strip for every block (A/B, bit-identical)
  bool odw = true;
  // the speech detector with one stream per wave where that measured faster (vad.hip
  // vad_speech_wave_kernel, vad_wave_streams); env MMLA_NO_VADW=1 at create: one thread per stream
  // everywhere (A/B, bit-identical); env MMLA_VADW=1: one stream per wave everywhere
  bool vadw = true;
  int vadw_all = 0;
  // OD blocks 1-3 as rolling column strips (rbs.hip); env MMLA_RB_TILE=1 at create: the 16 x 16 tile
  // kernels of resblk.hip instead
  bool rbs = true;
  // ... blocks 2-3 with the 3x3 conv's weights copied to LDS once per strip (rbs_w1l.hip); env
  // MMLA_NO_RBS_W1L=1 at create: rbs.hip's kernel, which streams them from global memory every chunk
  // (A/B, bit-identical)
  bool rbs_w1l = true;
  // ... block 1 with the 7-column last strips of two consecutive clips in one workgroup (rbs_tp.hip); env
  // MMLA_NO_RBS_TAILPAIR=1 at create: rbs.hip's kernel, one workgroup per clip for them (A/B, bit-identical)
  bool rbs_tailpair = true;
  // batches of <= lstm_split_max clips: the 3xFP16 BiLSTM with each direction's hidden units on eight workgroups
  // (nets.hip bilstm_h3_split_kernel); env MMLA_NO_LSTM_SPLIT=1 at create: one workgroup per direction
  bool lstm_split = true;
  // measured (tools/lat_split_sweep.py): OD 1.62 -> 1.53 ms at 128 clips, even at 192, +1 % at 256
  int lstm_split_max = 128;   // env MMLA_LSTM_SPLIT_MAX (A/B; the kernel takes up to 256)
  // test hook (env MMLA_DEBUG_LSTM_SPIN at create): the split BiLSTM's wait bound in polls (0 = default,
  // < 0 = give up at the first wait)
  int lstm_spin = 0;
  // 3xFP16 range guard: kernels set a word of range_dev [RW_COUNT] (enum RangeWord) when an operand they
  // split into fp16 is >= 65504 in magnitude or not finite (host-pointer micro-batches: re-run in exact
  // f32), the split BiLSTM (bilstm_h3_split_kernel) when a wait timed out (host-pointer micro-batches:
  // re-run on the one-workgroup-per-direction kernel)
  int* range_dev = nullptr;
  int* range_host = nullptr;                // pinned copy of range_dev[RW_HOST_RANGE .. RW_HOST_TIMEOUT]
  // small host-pointer calls (the real-time loops' batch-1 case): the range flag and the outputs live
  // in host-mapped coherent memory that the kernels write over the bus, so a micro-batch ends with one
  // stream synchronisation and host memcpys instead of three or four device-to-host copies, a flag
  // memset and a second synchronisation (each copy ≈ 20 µs of a 0.55 ms call).  env MMLA_NO_PIN_OUT=1
  // at create: staging slots in HBM + hipMemcpyAsync (A/B)
  bool pin_small = true;
  int* range_map = nullptr;       // host view: [0] range flag, [1] split-BiLSTM timeout
  int* range_map_dev = nullptr;   // device view of the same words
  char* pin_out = nullptr;        // kPinSlots x kPinSlotBytes, host view
  char* pin_out_dev = nullptr;
  char* pin_in = nullptr;         // kPinInBytes of pinned input staging: one DMA for PCM + lens
  int64_t lstm_split_reruns = 0;
  int64_t range_reruns = 0;
  bool od_f32_only = false, si_f32_only = false;   // weights outside the fp16 range
  bool si_base_f16_bad = false;   // a non-finite tensor below the SI head (si_f32_only = this or the head's)
  // mmla_vad_reset: webrtcvad.Vad(mode) per stream (device), [2 * vad_streams]: the second half
  // holds the states a conditioned micro-batch started from, for its re-runs (pipeline.cpp)
  VadState* vad_state = nullptr;
  int64_t vad_streams = 0;
  // mmla_capture_reset: the capture format (cap_ir / cap_or: the rate and 16000 over their gcd) and
  // audioop's ratecv state (d, prev) per stream (device, [2][cap_streams][2] int32).  A call reads half
  // cap_cur and writes the other one, which becomes current once every launch of the call is enqueued:
  // a call that fails on the way leaves the states it found
  int32_t* cap_state = nullptr;
  int cap_cur = 0;
  int64_t cap_streams = 0;
  int32_t cap_rate = 0, cap_channels = 0, cap_channel = 0, cap_ir = 0, cap_or = 0;
  // noise gate (nr.hip): tables + the bank of noise profiles' thresholds [nr_profiles][513]
  NrTables* nr_tables = nullptr;
  float* nr_thresh = nullptr;
  int64_t nr_profiles = 0;
  bool nr_ready = false;
  int32_t nr_bank_sr = 0;      // the sample rate the bank was built for (0: no bank)
  // the non-stationary gate's parameters (mmla_nr_set_nonstationary; noisereduce's defaults)
  double ns_time_constant_s = 2.0, ns_thresh_n_mult = 2.0, ns_sigmoid_slope = 10.0;
  int32_t ns_sr = 16000;
};

namespace mmla __attribute__((visibility("hidden"))) {

int fail(mmla_ctx* c, int code, const char* fmt, ...);

#define HIPCHK(ctx, expr)                                                                        \
  do {                                                                                           \
    hipError_t e_ = (expr);                                                                      \
    if (e_ != hipSuccess)                                                                        \
      return mmla::fail(ctx, MMLA_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                     \
  } while (0)

#define CHK(expr)              \
  do {                         \
    int r_ = (expr);           \
    if (r_ != MMLA_OK) return r_; \
  } while (0)

// ---- tracing: hipEvents around each launch when enabled (context.cpp) --------------------------
int prof_begin(mmla_ctx* c, int stage);
void prof_end(mmla_ctx* c, int idx, double work);
int prof_collect(mmla_ctx* c);

// launch `expr` (a hipError_t-returning launcher) as stage `st` with algorithmic work `wk`
#define LAUNCH(c, st, wk, expr)                  \
  do {                                           \
    const int pi_ = mmla::prof_begin((c), (st)); \
    HIPCHK((c), (expr));                         \
    mmla::prof_end((c), pi_, (wk));              \
  } while (0)

// ---- growable device workspace slots (context.cpp) ---------------------------------------------
enum Slot {
  S_PCM = 0, S_LENS, S_IMG, S_X, S_T1, S_T2, S_T3, S_SEQ, S_HOUT, S_LOGIT, S_FEAT, S_SILENT,
  S_OUT0, S_OUT1, S_OUT2, S_OUT3, S_IN,
  S_NR_S, S_NR_BITS, S_NR_FMAX, S_NR_FRAMES, S_NR_ITEMS, S_NR_Y, S_NR_ROWS,
  S_VAD_SPEECH, S_VAD_OUT, S_VAD_LENS, S_RS_TR, S_RS_WIN, S_LSTM,
  S_TRAIN,  // mmla_si_head_fit: every host-pointer operand, carved from one slot (carve_slot, fit_common.h)
  S_IMG2, S_GATE_Y0, S_GATE_Y1, S_SSIM,   // mmla_od_pipeline_gated / mmla_ssim_u8
  S_NR_PROF, S_COND_Q, S_COND_KEPT,       // profile indices of the gate; mmla_condition's outputs
  S_ROOM_P, S_ROOM_A,                     // mmla_room_pipeline_conditioned: the SI outputs' staging
  S_ENROL_VAD, S_ENROL_NW,                // mmla_si_enrol_embed: the temporary detectors, the window counts
  // mmla_si_loss_grad / mmla_si_finetune / mmla_si_base_*: the blob's copy, its gradient and every activation,
  // then the call's staged host-pointer operands; carved anew by every call (carve_slot)
  S_FT,
  S_MIX, S_MIX_LEN,  // mmla_od_mix / mmla_od_pipeline_mixed: a micro-batch's mixed clips and their lengths
  S_WIDE,  // a one-channel OD model's staged [.,1] images, before od_widen_launch widens them
  S_ODFT,  // mmla_od_loss_grad / mmla_od_finetune / mmla_od_train: likewise for the OD blob; the staged
           // operands of mmla_od_drop_mask, mmla_od_auc and mmla_od_augment
  // kept slots: a call fills them once, in front of its micro-batches, so they outlive the ws_release
  // before a repeated micro-batch, are not what microbatch() can reclaim, and are at least 256 bytes.
  // A capture conversion's staged raw clips, host frame counts, per-clip entry (d0, prev), converted
  // clips and their lengths; a host-pointer mix's pool and plan
  S_KEPT_BEGIN,
  S_CAP_RAW = S_KEPT_BEGIN, S_CAP_FRAMES, S_CAP_ITEM, S_CAP_CLIPS, S_CAP_LENS, S_MIX_POOL, S_MIX_PLAN,
  S_KEPT_END
};
inline bool slot_kept(int slot) { return slot >= S_KEPT_BEGIN && slot < S_KEPT_END; }

int ws_get(mmla_ctx* c, int slot, size_t bytes, void** out);
// free every workspace slot once the stream has drained; the kept ones only with kept_too
int ws_release(mmla_ctx* c, bool kept_too = false);
int64_t microbatch(mmla_ctx* c, bool od);
// the end of every entry point that launched: the last error, host-mode synchronisation, guard bands
int finish(mmla_ctx* c, bool dev);
void free_allocs(std::vector<void*>& al);   // weights.cpp
// which detector kernel a call with n_streams streams runs (mmla_debug_vad_path reports it)
inline bool vad_use_wave(const mmla_ctx* c, int64_t n_streams) {
  return c->vadw && (c->vadw_all > 0 || vad_wave_streams(n_streams));
}
// the body of mmla_nr_reduce on device pointers (capi.cpp): y [n_signals, stride] -> out [n_signals,
// len].  At most 512 items per launch with a stream synchronisation between launches.  profile
// (device, nullable = all 0): signal i is gated with noise profile profile[i] of the bank.
// nonstationary: the gate of mmla_nr_reduce_ns with the context's parameters instead; no bank is
// needed and profile is not read.
int nr_reduce_dev(mmla_ctx* c, const float* y, int64_t n_signals, int64_t stride, int64_t len, float* out,
                  const int32_t* profile = nullptr, bool nonstationary = false);

// device view of `count` input elements: the caller's pointer (device mode) or a copy in `slot`
template <typename T>
int in_ptr(mmla_ctx* c, const T* user, size_t count, bool dev, int slot, const T** d) {
  *d = user;
  if (dev || !user) return MMLA_OK;
  void* p = nullptr;
  CHK(ws_get(c, slot, count * sizeof(T), &p));
  HIPCHK(c, hipMemcpyAsync(p, user, count * sizeof(T), hipMemcpyHostToDevice, c->stream));
  *d = static_cast<const T*>(p);
  return MMLA_OK;
}

// device destination for an output chunk: the caller's pointer (device mode), a host-mapped slot
// (small host-mode outputs, mmla_ctx::pin_small) or a staging slot in HBM
template <typename T>
int out_ptr(mmla_ctx* c, T* user, int64_t off, size_t count, bool dev, int slot, T** d) {
  if (!user) {
    *d = nullptr;
    return MMLA_OK;
  }
  if (dev) {
    *d = user + off;
    return MMLA_OK;
  }
  if (c->pin_small && c->pin_out_dev && slot >= S_OUT0 && slot < S_OUT0 + kPinSlots &&
      count * sizeof(T) <= kPinSlotBytes) {
    *d = reinterpret_cast<T*>(c->pin_out_dev + (size_t)(slot - S_OUT0) * kPinSlotBytes);
    return MMLA_OK;
  }
  void* p = nullptr;
  CHK(ws_get(c, slot, count * sizeof(T), &p));
  *d = static_cast<T*>(p);
  return MMLA_OK;
}

template <typename T>
int copy_back(mmla_ctx* c, T* user, int64_t off, const T* d, size_t count, bool dev) {
  if (!user || dev) return MMLA_OK;
  const char* dc = reinterpret_cast<const char*>(d);
  if (c->pin_out_dev && dc >= c->pin_out_dev && dc < c->pin_out_dev + kPinSlots * kPinSlotBytes) {
    HIPCHK(c, hipStreamSynchronize(c->stream));   // the kernels wrote host memory: wait, then copy
    std::memcpy(user + off, c->pin_out + (dc - c->pin_out_dev), count * sizeof(T));
    return MMLA_OK;
  }
  HIPCHK(c, hipMemcpyAsync(user + off, d, count * sizeof(T), hipMemcpyDeviceToHost, c->stream));
  return MMLA_OK;
}

// ---- network runners (net_runners.cpp): device pointers, one micro-batch -----------------------

// The arithmetic of one pass over a micro-batch: the runners, their kernel choices and their
// kernel-argument fillers read it from this argument and nothing of it from the context
struct Arith {
  int prec;                  // MMLA_PREC_*
  bool split;                // the split BiLSTM may run
  int* range = nullptr;      // the word the kernels flag an out-of-range operand in (null: unguarded)
  int* timeout = nullptr;    // ... and the split BiLSTM a timeout (null: nowhere)
  bool h3() const { return prec == MMLA_PREC_F16X3; }
};
// the user's settings, unguarded: front-end and conditioning bodies, the debug trace
inline Arith unguarded(const mmla_ctx* c) { return Arith{c->precision, c->lstm_split}; }

// the OD 'silent' gate of one micro-batch: fewer than 4000 samples (record_on_pc.py:141-154; device
// lens (nullable) or clip_len), or the similarity of the clip's image to its denoised image below a
// threshold (record_on_pi.py:103-124; device ssim, nullable); silent output (nullable)
struct OdGate {
  const int32_t* lens = nullptr;
  int clip_len = -1;   // < 0: no gate (network-only calls)
  uint8_t* silent = nullptr;
  const float* ssim = nullptr;
  float ssim_threshold = 0.0f;
};

int run_od_net(mmla_ctx* c, const Arith& ar, const uint8_t* img_u8, const float* img_f32, int64_t n,
               float* probs, int32_t* argmax, OdGate gate = OdGate(), int stop = -1,
               const float** tap = nullptr, int64_t* tap_n = nullptr);
int run_si_net(mmla_ctx* c, const Arith& ar, const float* x, int64_t n, float* probs, int32_t* argmax,
               const uint8_t* silent, int ldx = SI_D, int stop = -1, const float** tap = nullptr,
               int64_t* tap_n = nullptr);

}  // namespace mmla
