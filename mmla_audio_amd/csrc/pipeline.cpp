// libmmla feature, forward and pipeline entry points: PCM staging, micro-batching and the 3xFP16
// range guard around the front-end kernels and the network runners (net_runners.cpp).
#include <algorithm>
#include <cmath>
#include <numeric>
#include <type_traits>

#include "internal.h"
#include "nets.h"
#include "resample.h"

using namespace mmla;

namespace {

// ---- PCM staging -------------------------------------------------------------------------------

template <typename T>
struct PcmT {
  const T* p;
  int64_t stride;
  const int32_t* lens;
  int32_t clip_len;   // samples of a row the kernels may read: the staged width at most
  int32_t true_len;   // without lens the clips' true length (it decides 'silent' and SI's T, not the
                      // staged width); 0 with lens
};
using Pcm = PcmT<int16_t>;

// Device view of clips [c0, c0 + cnt): offsets in device mode, a dense copy of the first
// `need` samples per clip in host mode.
template <typename T>
int stage_pcm(mmla_ctx* c, const T* pcm, int64_t c0, int64_t cnt, int64_t stride,
              const int32_t* lens, int32_t clip_len, int need, bool dev, PcmT<T>* out) {
  const int32_t tl = lens ? 0 : clip_len;
  if (dev) {
    *out = {pcm + c0 * stride, stride, lens ? lens + c0 : nullptr, clip_len, tl};
    return MMLA_OK;
  }
  int64_t width = lens ? std::min<int64_t>(need, stride) : std::min<int64_t>(need, clip_len);
  if (width < 1) width = 1;
  void* dp = nullptr;
  const bool overlap = !lens && stride < width;
  const size_t pbytes = (size_t)(overlap ? (cnt - 1) * stride + width : cnt * width) * sizeof(T);
  const size_t loff = (pbytes + 255) & ~(size_t)255;
  const size_t tot = loff + (lens ? cnt * sizeof(int32_t) : 0);
  if (c->pin_small && c->pin_in && tot <= kPinInBytes) {
    // small calls: gather into pinned memory on the host, one asynchronous DMA (host-mode bodies
    // end with a stream synchronisation, so the staging is free again when the next one starts)
    if (overlap) {
      std::memcpy(c->pin_in, pcm + c0 * stride, pbytes);
    } else {
      for (int64_t i = 0; i < cnt; ++i)
        std::memcpy(c->pin_in + (size_t)i * width * sizeof(T), pcm + (c0 + i) * stride, width * sizeof(T));
    }
    if (lens) std::memcpy(c->pin_in + loff, lens + c0, cnt * sizeof(int32_t));
    CHK(ws_get(c, S_PCM, tot, &dp));
    HIPCHK(c, hipMemcpyAsync(dp, c->pin_in, tot, hipMemcpyHostToDevice, c->stream));
    const int32_t* dl = lens ? reinterpret_cast<const int32_t*>(static_cast<char*>(dp) + loff) : nullptr;
    *out = {static_cast<T*>(dp), overlap ? stride : width, dl, (int32_t)std::min<int64_t>(clip_len, width), tl};
    return MMLA_OK;
  }
  if (overlap) {
    // overlapping windows of one signal (segmentation with step < window): copy the covered span
    // once and let the kernels read window c at c * stride
    const int64_t span = (cnt - 1) * stride + width;
    CHK(ws_get(c, S_PCM, (size_t)span * sizeof(T), &dp));
    HIPCHK(c, hipMemcpyAsync(dp, pcm + c0 * stride, span * sizeof(T), hipMemcpyHostToDevice,
                             c->stream));
    *out = {static_cast<T*>(dp), stride, nullptr, (int32_t)std::min<int64_t>(clip_len, width), tl};
    return MMLA_OK;
  }
  CHK(ws_get(c, S_PCM, (size_t)cnt * width * sizeof(T), &dp));
  HIPCHK(c, hipMemcpy2DAsync(dp, width * sizeof(T), pcm + c0 * stride, stride * sizeof(T),
                             width * sizeof(T), cnt, hipMemcpyHostToDevice, c->stream));
  int32_t* dl = nullptr;
  if (lens) {
    void* lp = nullptr;
    CHK(ws_get(c, S_LENS, (size_t)cnt * sizeof(int32_t), &lp));
    HIPCHK(c, hipMemcpyAsync(lp, lens + c0, cnt * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    dl = static_cast<int32_t*>(lp);
  }
  *out = {static_cast<T*>(dp), width, dl, (int32_t)std::min<int64_t>(clip_len, width), tl};
  return MMLA_OK;
}

// ---- micro-batching and the 3xFP16 range guard -------------------------------------------------

// body(c0, cnt) over clips [0, n) in micro-batches.  A workspace allocation failure (MMLA_E_OOM)
// frees the context's workspaces, halves the micro-batch (unless the caller fixed it with
// mmla_set_microbatch) and retries the same clips; the halving holds for the rest of this call only
// (a transient OOM, e.g. while another context held memory, must not cap every later call).
// granule: micro-batches are multiples of it (the conditioned calls' items_per_stream: a VAD
// stream's clips stay in one micro-batch), at least one granule even where the cap is smaller.
template <class F>
int for_microbatches(mmla_ctx* c, bool od, int64_t n, F&& body, int64_t granule = 1) {
  int64_t c0 = 0;
  auto whole = [&](int64_t m) { return std::max(granule, m / granule * granule); };
  int64_t mb = whole(microbatch(c, od));   // fixed for the call (unless an allocation fails)
  while (c0 < n) {
    const int64_t cnt = std::min(mb, n - c0);
    const int rc = body(c0, cnt);
    if (rc == MMLA_E_OOM && (od ? c->od_mb : c->si_mb) == 0 && cnt > kMinMicrobatch &&
        whole(std::max(kMinMicrobatch, cnt / 2)) < cnt) {
      CHK(ws_release(c));
      mb = whole(std::max(kMinMicrobatch, cnt / 2));   // this call only: the next call re-reads free memory
      continue;
    }
    CHK(rc);
    c0 += cnt;
  }
  return MMLA_OK;
}

// one micro-batch of a network call under the 3xFP16 range guard: body(ar) runs it in the arithmetic
// ar, built here per pass from the context's settings, which no pass changes.  Device-pointer calls let
// the kernels flag into range_dev's sticky words (reported by mmla_range_check / mmla_synchronize);
// host-pointer calls check their own words after the micro-batch and re-run it in exact f32 when an
// operand left the fp16 range.  f32_only: the model's weights are outside the fp16 range.
template <class F>
int guarded(mmla_ctx* c, bool dev, bool f32_only, F&& body) {
  Arith ar = unguarded(c);
  if (f32_only) ar.prec = MMLA_PREC_F32;
  if (!ar.h3()) return body(ar);
  if (dev) {
    ar.range = c->range_dev + RW_DEV_RANGE;
    ar.timeout = c->range_dev + RW_DEV_TIMEOUT;
    return body(ar);
  }
  // one pass of the micro-batch; -> its range flag and split-BiLSTM timeout flag
  auto pass = [&](bool* flagged, bool* timed_out) -> int {
    if (c->pin_small && c->range_map) {   // the flags in host-mapped memory: no memset, no copy
      ar.range = c->range_map_dev;
      ar.timeout = c->range_map_dev + 1;
      reinterpret_cast<volatile int*>(c->range_map)[0] = 0;   // host calls leave the stream idle
      reinterpret_cast<volatile int*>(c->range_map)[1] = 0;
      CHK(body(ar));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      *flagged = reinterpret_cast<volatile int*>(c->range_map)[0] != 0;
      *timed_out = reinterpret_cast<volatile int*>(c->range_map)[1] != 0;
    } else {
      static_assert(RW_HOST_TIMEOUT == RW_HOST_RANGE + 1, "one memset, one copy for both host words");
      ar.range = c->range_dev + RW_HOST_RANGE;
      ar.timeout = c->range_dev + RW_HOST_TIMEOUT;
      HIPCHK(c, hipMemsetAsync(ar.range, 0, 2 * sizeof(int), c->stream));
      CHK(body(ar));
      HIPCHK(c, hipMemcpyAsync(c->range_host, ar.range, 2 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      *flagged = c->range_host[0] != 0;
      *timed_out = c->range_host[1] != 0;
    }
    return MMLA_OK;
  };
  bool flagged = false, timed_out = false;
  CHK(pass(&flagged, &timed_out));
  if (timed_out) {   // a split-BiLSTM workgroup gave up waiting (NaN outputs): the unsplit kernel,
    ar.split = false;   // the same arithmetic bit for bit
    c->lstm_split_reruns += 1;
    CHK(pass(&flagged, &timed_out));
    if (timed_out) return fail(c, MMLA_E_HIP, "BiLSTM timed out without the split kernel");
  }
  if (flagged) {
    c->range_reruns += 1;
    CHK(body(Arith{MMLA_PREC_F32, ar.split}));
  }
  return MMLA_OK;
}

// The skeleton of the entry points over clips [0, n): null check, argument check (bad_args: the
// message, or null), hipSetDevice, then body(c0, cnt, dev, ar) per micro-batch with the host-mode
// synchronisation behind it, then finish.  ar: the guard's arithmetic of this pass for a network call, the
// unguarded one (for what the body runs outside its own guards) for every other.
//   FEATURES_*  a front-end call: in device mode one launch over the caller's buffers
//   NET_*       a network call: needs that model's weights; every micro-batch under the range guard
//   COND_*      a conditioned call (OD, SI, or both for a room): needs the weights of every network it
//               runs; micro-batched under both pointer modes (SI's cap for COND_SI, else OD's); the body
//               puts each network under a guard of its own, behind the conditioning
enum CallKind { FEATURES_OD, FEATURES_SI, NET_OD, NET_SI, COND_OD, COND_SI, COND_ROOM };

// the model a call of this kind needs and the context has not loaded (OD named first), or null
const char* missing_weights(const mmla_ctx* c, CallKind kind) {
  if ((kind == NET_OD || kind == COND_OD || kind == COND_ROOM) && !c->od_loaded) return "OD";
  if ((kind == NET_SI || kind == COND_SI || kind == COND_ROOM) && !c->si_loaded) return "SI";
  return nullptr;
}

template <class F>
int clip_call(mmla_ctx* c, CallKind kind, int64_t n, uint32_t flags, const char* bad_args, F&& body,
              int64_t granule = 1) {
  if (!c) return MMLA_E_INVALID;
  if (bad_args) return fail(c, MMLA_E_INVALID, "%s", bad_args);
  if (const char* m = missing_weights(c, kind)) return fail(c, MMLA_E_NOWEIGHTS, "%s weights not loaded", m);
  const bool od = kind != FEATURES_SI && kind != NET_SI && kind != COND_SI;   // whose micro-batch cap
  const bool net = kind == NET_OD || kind == NET_SI, cond = kind >= COND_OD;
  HIPCHK(c, hipSetDevice(c->device));
  const bool dev = flags & MMLA_DEVICE_PTR;
  auto once = [&](int64_t c0, int64_t cnt, const Arith& ar) -> int {
    CHK(body(c0, cnt, dev, ar));
    if (!dev) HIPCHK(c, hipStreamSynchronize(c->stream));
    return MMLA_OK;
  };
  if (net) {
    CHK(for_microbatches(c, od, n, [&](int64_t c0, int64_t cnt) -> int {
      return guarded(c, dev, od ? c->od_f32_only : c->si_f32_only,
                     [&](const Arith& ar) -> int { return once(c0, cnt, ar); });
    }, granule));
  } else if (dev && !cond) {
    if (n > 0) CHK(once(0, n, unguarded(c)));
  } else {
    CHK(for_microbatches(c, od, n, [&](int64_t c0, int64_t cnt) -> int { return once(c0, cnt, unguarded(c)); },
                         granule));
  }
  return finish(c, dev);
}

// The front-ends' arguments on a device view of clips; the outputs are the caller's to set.  img_type: the
// image a feature call asks for; the pipelines (-1) make the loaded OD model's (mmla_od_set_image_type)
template <typename T>
OdFeArgs od_fe_args(const mmla_ctx* c, const PcmT<T>& p, int img_type = -1) {
  OdFeArgs a{};
  a.img_type = img_type < 0 ? c->od_img_type : img_type;
  if constexpr (std::is_same<T, float>::value) a.pcm_f32 = p.p;
  else a.pcm = p.p;
  a.clip_stride = p.stride;
  a.lens = p.lens;
  a.clip_len = p.clip_len;
  a.tables = c->od_tables;
  return a;
}

SiFeArgs si_fe_args(const mmla_ctx* c, const Pcm& p) {
  SiFeArgs a{};
  a.pcm = p.p;
  a.clip_stride = p.stride;
  a.lens = p.lens;
  a.clip_len = p.true_len;
  a.tables = c->si_tables;
  return a;
}

// algorithmic HBM bytes of one front-end launch: PCM actually consumed + outputs
double od_fe_bytes(int64_t n, const OdFeArgs& a) {
  const double in = a.lens ? (double)MMLA_OD_CLIP * 2 : (double)std::min(a.clip_len, MMLA_OD_CLIP) * 2;
  const double out = (a.db ? OD_PIX * 4.0 : 0) + (a.norm ? OD_PIX * 4.0 : 0) +
                     (a.zcr ? OD_W * 4.0 : 0) + (a.img ? (double)OD_IMG : 0);
  return (double)n * (in + out);
}

double si_fe_bytes(int64_t n, const SiFeArgs& a) {
  const double in = a.lens ? (double)SI_NEED_SAMPLES * 2 : (double)std::min(a.clip_len, SI_NEED_SAMPLES) * 2;
  return (double)n * (in + SI_T * SI_D * 4.0 + (a.silent ? 1.0 : 0.0));
}

// 256-frame windows of a signal of n >= 1 samples: ceil(T / 256), T = psf's frame count
int64_t si_seq_windows(int64_t n) {
  const int64_t T = n <= 400 ? 1 : 1 + (n - 400 + 159) / 160;
  return (T + SI_T - 1) / SI_T;
}

bool bad_pcm_args(const void* pcm, int64_t n, int64_t stride, const int32_t* lens, int32_t clip_len) {
  if (n < 0 || (n > 0 && !pcm)) return true;
  if (!lens && clip_len < 0) return true;
  if (!lens && n > 1 && stride < 1) return true;   // stride < clip_len: overlapping windows
  return false;
}

template <typename T>
int od_features_common(mmla_ctx* c, const T* pcm, int64_t n, int64_t stride, const int32_t* lens,
                       int32_t clip_len, float* db, float* norm, float* zcr, uint8_t* img,
                       uint32_t flags) {
  // float PCM: the front-end splits y 2^3 into fp16 hi + lo, so the kernel checks every sample it
  // reads (the first min(len, 24000) of each clip) into a range word: device-pointer calls into the
  // sticky word (mmla_range_check / mmla_synchronize report it), host-pointer calls into their own
  // word, read after the micro-batch's synchronisation; only then is the micro-batch re-scanned on
  // the host, to name the first offending sample
  auto host_range_error = [&](int64_t c0, int64_t cnt) -> int {
    if constexpr (std::is_same<T, float>::value) {
      for (int64_t i = c0; i < c0 + cnt; ++i) {
        const int64_t len = std::min<int64_t>(lens ? lens[i] : clip_len, MMLA_OD_CLIP);
        for (int64_t j = 0; j < len; ++j)
          if (!(std::fabs(pcm[i * stride + j]) < 8188.0f))
            return fail(c, MMLA_E_RANGE,
                        "float PCM clip %lld sample %lld = %g: the front-end needs |y| < 8188 (y * 8 is "
                        "split into fp16)", (long long)i, (long long)j, (double)pcm[i * stride + j]);
      }
    }
    return fail(c, MMLA_E_RANGE, "float PCM outside |y| < 8188 in clips %lld..%lld", (long long)c0,
                (long long)(c0 + cnt - 1));
  };
  // the image type in the flags' two bits: none = ZCR, both = no type
  const int img_type = (int)((flags & MMLA_OD_IMG_MASK) >> MMLA_OD_IMG_SHIFT);
  const char* bad = bad_pcm_args(pcm, n, stride, lens, clip_len) ? "bad pcm args"
                    : img_type > MMLA_OD_IMG_VIRIDIS             ? "both image-type flags set"
                                                                 : nullptr;
  return clip_call(c, FEATURES_OD, n, flags, bad, [&](int64_t c0, int64_t cnt, bool dev, const Arith&) -> int {
    PcmT<T> p;
    CHK(stage_pcm(c, pcm, c0, cnt, stride, lens, clip_len, MMLA_OD_CLIP, dev, &p));
    OdFeArgs a = od_fe_args(c, p, img_type);
    if constexpr (std::is_same<T, float>::value) {
      a.range_flag = c->range_dev + (dev ? RW_DEV_RANGE : RW_HOST_RANGE);
      if (!dev) HIPCHK(c, hipMemsetAsync(a.range_flag, 0, sizeof(int), c->stream));
    }
    CHK(out_ptr(c, db, c0 * OD_PIX, cnt * OD_PIX, dev, S_OUT0, &a.db));
    CHK(out_ptr(c, norm, c0 * OD_PIX, cnt * OD_PIX, dev, S_OUT1, &a.norm));
    CHK(out_ptr(c, zcr, c0 * OD_W, cnt * OD_W, dev, S_OUT2, &a.zcr));
    CHK(out_ptr(c, img, c0 * OD_IMG, cnt * OD_IMG, dev, S_OUT3, &a.img));
    LAUNCH(c, MMLA_STAGE_OD_FE, od_fe_bytes(cnt, a), od_fe_launch(a, cnt, c->stream));
    CHK(copy_back(c, db, c0 * OD_PIX, a.db, cnt * OD_PIX, dev));
    CHK(copy_back(c, norm, c0 * OD_PIX, a.norm, cnt * OD_PIX, dev));
    CHK(copy_back(c, zcr, c0 * OD_W, a.zcr, cnt * OD_W, dev));
    CHK(copy_back(c, img, c0 * OD_IMG, a.img, cnt * OD_IMG, dev));
    if (std::is_same<T, float>::value && !dev) {   // the range word, once the launch has drained
      HIPCHK(c, hipStreamSynchronize(c->stream));
      int flag = 0;
      HIPCHK(c, hipMemcpy(&flag, c->range_dev + RW_HOST_RANGE, sizeof(int), hipMemcpyDeviceToHost));
      if (flag) return host_range_error(c0, cnt);
    }
    return MMLA_OK;
  });
}

// A caller's OD images [cnt,128,151,C] (C of the loaded model) on the device as the network reads them,
// 3 per pixel: a three-channel model's as they are (host: copied into `slot`), a one-channel model's
// widened to (g, g, g) into `slot`
template <typename T>
int od_net_input(mmla_ctx* c, const T* user, int64_t cnt, bool dev, int slot, const T** d) {
  if (c->od.channels == 3) return in_ptr(c, user, cnt * OD_IMG, dev, slot, d);
  const T* g = nullptr;
  CHK(in_ptr(c, user, cnt * OD_PIX, dev, S_WIDE, &g));
  void* w = nullptr;
  CHK(ws_get(c, slot, cnt * OD_IMG * sizeof(T), &w));
  if constexpr (std::is_same<T, float>::value)
    LAUNCH(c, MMLA_STAGE_GLUE, (double)cnt * OD_PIX * 16, od_widen_launch(nullptr, g, cnt * OD_PIX, w, c->stream));
  else
    LAUNCH(c, MMLA_STAGE_GLUE, (double)cnt * OD_PIX * 4, od_widen_launch(g, nullptr, cnt * OD_PIX, w, c->stream));
  *d = static_cast<const T*>(w);
  return MMLA_OK;
}

// OD-NET over float NHWC (x_f32) or uint8 (x_u8) images
int od_forward_common(mmla_ctx* c, const float* x_f32, const uint8_t* x_u8, int64_t n, float* probs,
                      uint32_t flags) {
  const bool bad = n < 0 || (n > 0 && ((!x_f32 && !x_u8) || !probs));
  return clip_call(c, NET_OD, n, flags, bad ? "bad od_forward args" : nullptr,
                   [&](int64_t c0, int64_t cnt, bool dev, const Arith& ar) -> int {
    const float* df = nullptr;
    const uint8_t* du = nullptr;
    const int64_t per = (int64_t)OD_PIX * c->od.channels;
    if (x_f32) CHK(od_net_input(c, x_f32 + c0 * per, cnt, dev, S_IN, &df));
    else CHK(od_net_input(c, x_u8 + c0 * per, cnt, dev, S_IMG, &du));
    float* dp;
    const int k = c->od.k;
    CHK(out_ptr(c, probs, c0 * k, cnt * k, dev, S_OUT0, &dp));
    CHK(run_od_net(c, ar, du, df, cnt, dp, nullptr));
    return copy_back(c, probs, c0 * k, dp, cnt * k, dev);
  });
}

// The noise gate's passes over clips p (their first D samples): y = pcm / 32768 into y0, then nr_passes x
// (the gate y0 -> y1, the PCM_16 round trip back into y0); the last pass leaves its int16 samples in q
// instead.  y0, y1 [cnt][D] floats and q are the caller's; profile: device indices, nullable.
int gate_passes(mmla_ctx* c, const Pcm& p, int64_t cnt, int D, int nr_passes, const int32_t* profile, bool ns,
                float* y0, float* y1, int16_t* q) {
  LAUNCH(c, MMLA_STAGE_GLUE, (double)cnt * D * 6, pcm_f32_launch(p.p, p.stride, p.lens, D, cnt, y0, c->stream));
  for (int k = 0; k < nr_passes; ++k) {
    // a pass re-uses the gate's item table and scratch: the one before it has drained
    if (k) HIPCHK(c, hipStreamSynchronize(c->stream));
    CHK(nr_reduce_dev(c, y0, cnt, D, D, y1, profile, ns));
    const bool last = k == nr_passes - 1;
    LAUNCH(c, MMLA_STAGE_GLUE, (double)cnt * D * (last ? 6 : 8),
           requant_launch(y1, p.lens, D, cnt, last ? nullptr : y0, last ? q : nullptr, c->stream));
  }
  return MMLA_OK;
}

// the OD front-end's image of clips p into the workspace slot `slot`
int od_image(mmla_ctx* c, const Pcm& p, int64_t cnt, int slot, const uint8_t** img) {
  void* pimg = nullptr;
  CHK(ws_get(c, slot, cnt * OD_IMG, &pimg));
  OdFeArgs a = od_fe_args(c, p);
  a.img = static_cast<uint8_t*>(pimg);
  LAUNCH(c, MMLA_STAGE_OD_FE, od_fe_bytes(cnt, a), od_fe_launch(a, cnt, c->stream));
  *img = a.img;
  return MMLA_OK;
}

// OD-NET on a micro-batch's images with the 'silent' gate on the lengths of p (and on g's SSIM fields,
// where the caller set them), results into probs / argmax / silent at clip c0
int od_net_out(mmla_ctx* c, const Arith& ar, const uint8_t* img, const Pcm& p, OdGate g, int64_t c0, int64_t cnt,
               bool dev, float* probs, int32_t* argmax, uint8_t* silent) {
  float* dp;
  int32_t* da;
  const int k = c->od.k;   // the loaded head's classes
  CHK(out_ptr(c, probs, c0 * k, cnt * k, dev, S_OUT0, &dp));
  CHK(out_ptr(c, argmax, c0, cnt, dev, S_OUT1, &da));
  CHK(out_ptr(c, silent, c0, cnt, dev, S_OUT2, &g.silent));
  g.lens = p.lens;
  g.clip_len = p.true_len;
  CHK(run_od_net(c, ar, img, nullptr, cnt, dp, da, g));
  CHK(copy_back(c, probs, c0 * k, dp, cnt * k, dev));
  CHK(copy_back(c, argmax, c0, da, cnt, dev));
  return copy_back(c, silent, c0, g.silent, cnt, dev);
}

// OD front-end + network of one micro-batch on the device view p of its clips
int od_fe_net(mmla_ctx* c, const Arith& ar, const Pcm& p, int64_t c0, int64_t cnt, bool dev, float* probs,
              int32_t* argmax, uint8_t* silent) {
  const uint8_t* img;
  CHK(od_image(c, p, cnt, S_IMG, &img));
  return od_net_out(c, ar, img, p, OdGate(), c0, cnt, dev, probs, argmax, silent);
}

// the fused OD pipeline; `gated` adds the denoise-and-compare silence gate of record_on_pi.py:103-124
// (nr_passes gate + PCM_16 round trips, the second image, their SSIM) in front of the network
int od_pipeline_common(mmla_ctx* c, const int16_t* pcm, int64_t n, int64_t stride, const int32_t* lens,
                       int32_t clip_len, bool gated, int32_t nr_passes, float ssim_threshold,
                       float* probs, int32_t* argmax, uint8_t* silent, float* ssim, uint32_t flags,
                       bool pcm_dev = false) {
  const char* bad = bad_pcm_args(pcm, n, stride, lens, clip_len) ? "bad pcm args" : nullptr;
  const bool ns = flags & MMLA_NR_NONSTATIONARY;   // the passes run the non-stationary gate: no bank
  if (c && !bad && gated) {
    // the gate's SSIM is defined on the ZCR images (record_on_pi.py:117-120)
    if (c->od_loaded && c->od_img_type != MMLA_OD_IMG_ZCR) bad = "the gated pipeline needs a ZCR model";
    else if (nr_passes < 0) bad = "nr_passes < 0";
    else if (nr_passes > 0 && !ns && !c->nr_ready) bad = "nr_passes > 0: mmla_nr_set_noise must be called first";
  }
  return clip_call(c, NET_OD, n, flags, bad, [&](int64_t c0, int64_t cnt, bool dev, const Arith& ar) -> int {
    Pcm p;
    CHK(stage_pcm(c, pcm, c0, cnt, stride, lens, clip_len, MMLA_OD_CLIP, dev || pcm_dev, &p));
    if (!gated) return od_fe_net(c, ar, p, c0, cnt, dev, probs, argmax, silent);
    const uint8_t *img, *net_img;
    CHK(od_image(c, p, cnt, S_IMG, &img));
    net_img = img;
    float* dss;
    CHK(out_ptr(c, ssim, c0, cnt, dev, S_OUT3, &dss));
    if (!dss) {
      void* q = nullptr;
      CHK(ws_get(c, S_SSIM, cnt * sizeof(float), &q));
      dss = static_cast<float*>(q);
    }
    // the gate sees what the front-end sees: the first 24000 samples at most
    const int D = (int)std::min<int64_t>(clip_len, MMLA_OD_CLIP);
    if (nr_passes > 0 && D > 0) {
      // two float clip buffers; the last pass leaves its int16 samples in the first one.  The slack
      // keeps the front-end's read of a clip whose lens[i] exceeds clip_len inside the buffer
      const size_t ybytes = (size_t)cnt * D * sizeof(float) + MMLA_OD_CLIP * sizeof(int16_t);
      void *py0 = nullptr, *py1 = nullptr;
      CHK(ws_get(c, S_GATE_Y0, ybytes, &py0));
      CHK(ws_get(c, S_GATE_Y1, ybytes, &py1));
      int16_t* yq = static_cast<int16_t*>(py0);
      CHK(gate_passes(c, p, cnt, D, nr_passes, nullptr, ns, static_cast<float*>(py0), static_cast<float*>(py1), yq));
      CHK(od_image(c, Pcm{yq, D, p.lens, D, p.true_len}, cnt, S_IMG2, &net_img));
      LAUNCH(c, MMLA_STAGE_OD_FE, (double)cnt * (2.0 * OD_IMG + 4),
             ssim_u8_launch(img, net_img, cnt, OD_H, OD_W, 3, dss, c->stream));
    } else {   // not denoised: the second image is the first, their similarity 1
      LAUNCH(c, MMLA_STAGE_GLUE, (double)cnt * 4, fill_f32_launch(dss, cnt, 1.0f, c->stream));
    }
    OdGate g;
    g.ssim = dss;
    g.ssim_threshold = ssim_threshold;
    CHK(od_net_out(c, ar, net_img, p, g, c0, cnt, dev, probs, argmax, silent));
    return copy_back(c, ssim, c0, static_cast<const float*>(dss), cnt, dev);
  });
}

// SI front-end + network of one micro-batch on the device view p of its clips, results into probs /
// argmax / silent at clip c0 (host mode: staged in the output slots slot_p / slot_a)
int si_fe_net(mmla_ctx* c, const Arith& ar, const Pcm& p, int64_t c0, int64_t cnt, bool dev, float* probs,
              int32_t* argmax, uint8_t* silent, int slot_p = S_OUT0, int slot_a = S_OUT1) {
  const int k = c->si.k;
  void* pf;
  // the features stay on the device: rows of 40 floats when the 3xFP16 stem reads them
  const int ldf = ar.h3() && c->si.stem.wh && c->si.stem.cin_pad > SI_D && c->si_pad_feat ? SI_D + 1 : SI_D;
  CHK(ws_get(c, S_FEAT, cnt * SI_T * ldf * sizeof(float), &pf));
  uint8_t* pso = nullptr;   // host mode: the caller's 'silent' flags through an output slot
  if (!dev && silent) CHK(out_ptr(c, silent, c0, cnt, dev, S_OUT2, &pso));
  void* ps = pso;
  if (!ps) CHK(ws_get(c, S_SILENT, cnt, &ps));
  SiFeArgs a = si_fe_args(c, p);
  a.feat = static_cast<float*>(pf);
  a.ldf = ldf;
  a.silent = static_cast<uint8_t*>(ps);
  LAUNCH(c, MMLA_STAGE_SI_FE, si_fe_bytes(cnt, a), si_fe_launch(a, cnt, c->stream));
  float* dp;
  int32_t* da;
  CHK(out_ptr(c, probs, c0 * k, cnt * k, dev, slot_p, &dp));
  CHK(out_ptr(c, argmax, c0, cnt, dev, slot_a, &da));
  CHK(run_si_net(c, ar, a.feat, cnt, dp, da, a.silent, ldf));
  CHK(copy_back(c, probs, c0 * k, dp, cnt * k, dev));
  CHK(copy_back(c, argmax, c0, da, cnt, dev));
  if (silent && dev)
    HIPCHK(c, hipMemcpyAsync(silent + c0, a.silent, cnt, hipMemcpyDeviceToDevice, c->stream));
  else if (silent)
    CHK(copy_back(c, silent, c0, pso, cnt, dev));
  return MMLA_OK;
}

// ---- the PC loop's pre-conditioning: save_wave_file(noise_reduce=True, silence_remove=...) --------

// The arguments of mmla_condition and the state its micro-batches share.  run() conditions clips
// [c0, c0 + cnt) into the context's workspace: q [cnt][clip_len] int16 (the rewritten file, zeros
// behind it) and kept [cnt].  The noise gate is stateless, the detectors are not: run() copies the
// micro-batch's streams' VadState aside the first time it sees c0 and puts the copy back when it is
// called for the same c0 again (for_microbatches repeating the micro-batch with fewer clips after an
// allocation failure; a guard re-run repeats a network alone and does not come here), so the decisions
// and the state left behind do not depend on whether a re-run happened.
struct Conditioner {
  const int16_t* pcm;
  int64_t n, stride;
  const int32_t* lens;
  int32_t clip_len;
  const int32_t* profile;
  int32_t nr_passes, silence_remove;
  int64_t ips;
  int16_t* out_pcm;    // nullable
  int32_t* kept_len;   // nullable
  bool ns = false;     // MMLA_NR_NONSTATIONARY: the passes need no bank and read no profile
  // pcm and lens are device pointers whatever the call's flags say (the capture calls: the converted
  // clips never leave the device); profile and the outputs follow the flags
  bool pcm_dev = false;
  // mmla_si_enrol_embed: whole recordings (clip_len up to MMLA_ENROL_MAX_SAMPLES, gated chunk by chunk
  // inside nr_reduce_dev), one per stream, each on a fresh temporary detector of mode vad_mode that
  // run() creates anew every time: the context's vad_state is neither needed nor touched, and a
  // repeated micro-batch simply starts again
  bool enrol = false;
  int32_t vad_mode = 3;
  int64_t snap_c0 = -1, snap_streams = 0;
  const int16_t* q = nullptr;      // device results of the last run()
  const int32_t* kept = nullptr;
  std::vector<VadState> fresh;     // enrol: the host image of the temporary detectors

  const char* bad(const mmla_ctx* c, bool dev) const {
    if (bad_pcm_args(pcm, n, stride, lens, clip_len)) return "bad pcm args";
    if (enrol) {
      if (clip_len < 1 || clip_len > MMLA_ENROL_MAX_SAMPLES)
        return "clip_len must be in [1, MMLA_ENROL_MAX_SAMPLES] (4096 detector frames)";
      if (vad_mode < 0 || vad_mode > 3) return "VAD mode must be 0..3";
    } else if (clip_len < 1 || clip_len > 600000) {
      return "clip_len must be in [1, 600000] (one gate chunk)";
    }
    if (n > 1 && stride < clip_len) return "clip_stride < clip_len";
    if (nr_passes < 0) return "nr_passes < 0";
    if (nr_passes > 0 && !ns && !c->nr_ready) return "nr_passes > 0: mmla_nr_set_noise(_bank) must be called first";
    if (ips < 1 || n % ips) return "n_clips is not a multiple of items_per_stream";
    if (silence_remove && !enrol && (!c->vad_state || c->vad_streams != n / ips))
      return "silence_remove: mmla_vad_reset must have created n_clips / items_per_stream streams";
    // device-pointer profile indices cannot be seen here: the kernels clamp them into the bank
    if (profile && !dev && nr_passes > 0 && !ns)
      for (int64_t i = 0; i < n; ++i)
        if (profile[i] < 0 || profile[i] >= c->nr_profiles) return "profile index outside the bank";
    return nullptr;
  }
  bool off() const { return nr_passes == 0 && !silence_remove; }

  int run(mmla_ctx* c, int64_t c0, int64_t cnt, bool dev) {
    const int D = clip_len;
    Pcm p;
    CHK(stage_pcm(c, pcm, c0, cnt, n > 1 ? stride : (int64_t)D, lens, D, D, dev || pcm_dev, &p));
    void *py0 = nullptr, *py1 = nullptr, *pq = nullptr, *pk = nullptr;
    CHK(ws_get(c, S_COND_Q, (size_t)cnt * D * sizeof(int16_t), &pq));
    CHK(ws_get(c, S_COND_KEPT, (size_t)cnt * sizeof(int32_t), &pk));
    int16_t* dq = static_cast<int16_t*>(pq);
    int32_t* dk = static_cast<int32_t*>(pk);
    // the input of the silence removal (it cannot rewrite in place): the first float buffer, as int16
    int16_t* src = silence_remove ? nullptr : dq;
    if (silence_remove || nr_passes > 0) {
      CHK(ws_get(c, S_GATE_Y0, (size_t)cnt * D * sizeof(float), &py0));
      if (silence_remove) src = static_cast<int16_t*>(py0);
    }
    if (nr_passes > 0) {
      CHK(ws_get(c, S_GATE_Y1, (size_t)cnt * D * sizeof(float), &py1));
      const int32_t* dprof;
      CHK(in_ptr(c, profile && !ns ? profile + c0 : nullptr, (size_t)cnt, dev, S_NR_PROF, &dprof));
      CHK(gate_passes(c, p, cnt, D, nr_passes, dprof, ns, static_cast<float*>(py0), static_cast<float*>(py1), src));
    } else {
      LAUNCH(c, MMLA_STAGE_GLUE, (double)cnt * D * 4,
             pcm_i16_launch(p.p, p.stride, p.lens, D, cnt, src, c->stream));
    }
    const int32_t* vad_lens = nullptr;
    if (silence_remove) {
      const int64_t s0 = c0 / ips, ns = cnt / ips;
      VadState* state = c->vad_state + s0;
      VadState* snap = c->vad_state + c->vad_streams;
      if (enrol) {
        VadState init;
        if (!vad_init_state(&init, vad_mode)) return fail(c, MMLA_E_INVALID, "VAD mode must be 0..3");
        void* pst = nullptr;
        CHK(ws_get(c, S_ENROL_VAD, (size_t)cnt * sizeof(VadState), &pst));
        fresh.assign((size_t)cnt, init);
        HIPCHK(c, hipMemcpyAsync(pst, fresh.data(), (size_t)cnt * sizeof(VadState), hipMemcpyHostToDevice,
                                 c->stream));
        // a device-pointer call returns with its launches only enqueued: the host image must have left
        if (dev) HIPCHK(c, hipStreamSynchronize(c->stream));
        state = static_cast<VadState*>(pst);
      } else if (c0 == snap_c0) {
        HIPCHK(c, hipMemcpyAsync(c->vad_state + s0, snap + s0, snap_streams * sizeof(VadState),
                                 hipMemcpyDeviceToDevice, c->stream));
      } else {
        HIPCHK(c, hipMemcpyAsync(snap + s0, c->vad_state + s0, ns * sizeof(VadState),
                                 hipMemcpyDeviceToDevice, c->stream));
        snap_c0 = c0;
        snap_streams = ns;
      }
      void *psp = nullptr, *pvl = nullptr;
      VadArgs v{};
      v.pcm = src;
      v.stride = D;
      v.lens = p.lens;
      v.clip_len = D;
      v.n_items = cnt;
      v.items_per_stream = ips;
      v.state = state;
      v.max_frames = std::max(1, vad_frames(D));
      CHK(ws_get(c, S_VAD_SPEECH, (size_t)cnt * v.max_frames, &psp));
      CHK(ws_get(c, S_VAD_LENS, (size_t)cnt * sizeof(int32_t), &pvl));
      v.speech = static_cast<uint8_t*>(psp);
      v.out = dq;
      v.out_lens = static_cast<int32_t*>(pvl);
      LAUNCH(c, MMLA_STAGE_GLUE, (double)cnt * D, vad_speech_launch(v, vad_use_wave(c, ns), c->stream));
      LAUNCH(c, MMLA_STAGE_GLUE, (double)cnt * D, vad_collect_launch(v, c->stream));
      vad_lens = v.out_lens;
    }
    LAUNCH(c, MMLA_STAGE_GLUE, (double)cnt * D * 2,
           cond_finish_launch(dq, vad_lens, p.lens, D, cnt, dk, c->stream));
    const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (out_pcm)
      HIPCHK(c, hipMemcpyAsync(out_pcm + c0 * D, dq, (size_t)cnt * D * sizeof(int16_t), kind, c->stream));
    if (kept_len)
      HIPCHK(c, hipMemcpyAsync(kept_len + c0, dk, (size_t)cnt * sizeof(int32_t), kind, c->stream));
    q = dq;
    kept = dk;
    return MMLA_OK;
  }
};

// mmla_condition once cd.bad() has passed: FEATURES_* micro-batching (host mode), one pass over the whole
// batch (device mode)
int condition_call(mmla_ctx* c, Conditioner& cd, uint32_t flags) {
  return clip_call(c, FEATURES_OD, cd.n, flags, nullptr, [&](int64_t c0, int64_t cnt, bool dev, const Arith&) -> int {
    return cd.run(c, c0, cnt, dev);
  }, std::max<int64_t>(cd.ips, 1));
}

int si_pipeline_common(mmla_ctx* c, const int16_t* pcm, int64_t n, int64_t stride, const int32_t* lens,
                       int32_t clip_len, float* probs, int32_t* argmax, uint8_t* silent, uint32_t flags,
                       bool pcm_dev = false) {
  return clip_call(c, NET_SI, n, flags, bad_pcm_args(pcm, n, stride, lens, clip_len) ? "bad pcm args" : nullptr,
                   [&](int64_t c0, int64_t cnt, bool dev, const Arith& ar) -> int {
    Pcm p;
    CHK(stage_pcm(c, pcm, c0, cnt, stride, lens, clip_len, SI_NEED_SAMPLES, dev || pcm_dev, &p));
    return si_fe_net(c, ar, p, c0, cnt, dev, probs, argmax, silent);
  });
}

// ---- the conditioned pipelines on a Conditioner (mmla_*_pipeline_conditioned, _capture) ------------

// the networks' outputs of the three calls: COND_OD / COND_SI use their own (probs, argmax), COND_ROOM
// all four
struct NetOut {
  float* od_probs;
  int32_t* od_argmax;
  float* si_probs;
  int32_t* si_argmax;
  uint8_t* silent;
};

// cd.bad() has passed and the weights are loaded
int conditioned_body(mmla_ctx* c, CallKind kind, Conditioner& cd, const NetOut& o, uint32_t flags) {
  if (kind == FEATURES_OD) return condition_call(c, cd, flags);   // mmla_condition: no network
  const bool od = kind != COND_SI, si = kind != COND_OD;
  if (cd.off()) {   // nothing to condition: the plain pipelines, then the copies asked for
    if (od)
      CHK(od_pipeline_common(c, cd.pcm, cd.n, cd.stride, cd.lens, cd.clip_len, false, 0, 0.0f, o.od_probs,
                             o.od_argmax, o.silent, nullptr, flags, cd.pcm_dev));
    if (si)
      CHK(si_pipeline_common(c, cd.pcm, cd.n, cd.stride, cd.lens, cd.clip_len, o.si_probs, o.si_argmax,
                             od ? nullptr : o.silent, flags, cd.pcm_dev));
    return cd.out_pcm || cd.kept_len ? condition_call(c, cd, flags) : MMLA_OK;
  }
  // Per micro-batch (whole streams) Conditioner::run once, then each network's front-end + net under
  // its own range guard, reading the conditioned clips that stay in S_COND_Q / S_COND_KEPT with lens =
  // kept_len (a row holds clip_len samples, zeros behind kept_len).  A guard re-run repeats that network
  // alone; an allocation failure repeats the micro-batch with fewer clips, the detectors restored by
  // Conditioner::run's snapshot.  With OD in the call, 'silent' (kept_len < 4000) is its gate's: SI's own
  // flag, the same rule, stays in the workspace, and SI's outputs are staged in slots of their own.
  return clip_call(c, kind, cd.n, flags, nullptr, [&](int64_t c0, int64_t cnt, bool dev, const Arith&) -> int {
    CHK(cd.run(c, c0, cnt, dev));
    const Pcm p{cd.q, cd.clip_len, cd.kept, cd.clip_len, 0};
    if (od)
      CHK(guarded(c, dev, c->od_f32_only, [&](const Arith& ar) -> int {
        return od_fe_net(c, ar, p, c0, cnt, dev, o.od_probs, o.od_argmax, o.silent);
      }));
    if (si)
      CHK(guarded(c, dev, c->si_f32_only, [&](const Arith& ar) -> int {
        return si_fe_net(c, ar, p, c0, cnt, dev, o.si_probs, o.si_argmax, od ? nullptr : o.silent,
                         od ? S_ROOM_P : S_OUT0, od ? S_ROOM_A : S_OUT1);
      }));
    return MMLA_OK;
  }, std::max<int64_t>(cd.ips, 1));
}

// ---- a room's capture format in front of the conditioned pipelines ----------------------------------

// raw capture staged per piece of a host-pointer conversion (whole streams; one stream where a stream
// is larger)
constexpr size_t kCapStageBytes = 64u << 20;

// One conversion: interleaved capture clips -> 16 kHz mono.  fresh: from fresh states, the context's
// left alone (a whole recording); else on the states mmla_capture_reset created, advanced once.
struct Capture {
  const int16_t* pcm;
  int64_t n, stride;
  const int32_t* frames;
  int32_t clip_frames;
  int64_t ips;
  bool fresh;
  int32_t out_clip_len = 0;

  const char* bad(const mmla_ctx* c, bool dev) {
    if (!c->cap_rate) return "mmla_capture_reset must be called first";
    if (n < 0 || (n > 0 && !pcm)) return "bad capture pcm args";
    if (clip_frames < 1) return "clip_frames < 1";
    if (stride < (int64_t)clip_frames * c->cap_channels) return "clip_stride < clip_frames * channels";
    if (ips < 1 || n % ips) return "n_clips is not a multiple of items_per_stream";
    if (!fresh && (!c->cap_state || n / ips != c->cap_streams))
      return "mmla_capture_reset must have created n_clips / items_per_stream streams";
    const int64_t ocl = ((int64_t)clip_frames * c->cap_or - 1) / c->cap_ir + 1;
    if (ocl > 600000) return "out_clip_len > 600000 (one gate chunk)";
    out_clip_len = (int32_t)ocl;
    if (frames && !dev)   // device-pointer frames cannot be seen here: the kernels clamp them
      for (int64_t i = 0; i < n; ++i)
        if (frames[i] < 0 || frames[i] > clip_frames) return "frames[c] outside [0, clip_frames]";
    return nullptr;
  }

  // out [n][out_stride], out_lens [n]: device pointers.  The states flip only after the last launch is
  // enqueued, so an error on the way leaves them as they were
  int run(mmla_ctx* c, bool dev, int16_t* out, int64_t out_stride, int32_t* out_lens) const {
    if (n == 0) return MMLA_OK;
    const int nch = c->cap_channels;
    void *pitem = nullptr, *pfr = nullptr, *praw = nullptr;
    CHK(ws_get(c, S_CAP_ITEM, (size_t)n * 2 * sizeof(int32_t), &pitem));
    const int32_t* dframes = frames;
    const int64_t row = (int64_t)clip_frames * nch;
    int64_t piece = n;
    if (!dev) {
      if (frames) {
        CHK(ws_get(c, S_CAP_FRAMES, (size_t)n * sizeof(int32_t), &pfr));
        HIPCHK(c, hipMemcpyAsync(pfr, frames, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        dframes = static_cast<const int32_t*>(pfr);
      }
      piece = std::max<int64_t>(ips, (int64_t)(kCapStageBytes / ((size_t)row * sizeof(int16_t))) / ips * ips);
      piece = std::min(piece, n);
      CHK(ws_get(c, S_CAP_RAW, (size_t)piece * row * sizeof(int16_t), &praw));
    }
    const int64_t ns = c->cap_streams;
    for (int64_t c0 = 0; c0 < n; c0 += piece) {
      const int64_t cnt = std::min(piece, n - c0), s0 = c0 / ips;
      CaptureArgs a{};
      if (dev) {
        a.pcm = pcm + c0 * stride;
        a.clip_stride = stride;
      } else {   // the next piece's copy waits on the stream for the kernels that read this one
        HIPCHK(c, hipMemcpy2DAsync(praw, row * sizeof(int16_t), pcm + c0 * stride, stride * sizeof(int16_t),
                                   row * sizeof(int16_t), cnt, hipMemcpyHostToDevice, c->stream));
        a.pcm = static_cast<const int16_t*>(praw);
        a.clip_stride = row;
      }
      a.frames = dframes ? dframes + c0 : nullptr;
      a.clip_frames = clip_frames;
      a.channels = nch;
      a.channel = c->cap_channel;
      a.ir = c->cap_ir;
      a.orr = c->cap_or;
      a.n_clips = cnt;
      a.items_per_stream = ips;
      if (!fresh) {
        a.state_in = c->cap_state + ((int64_t)c->cap_cur * ns + s0) * 2;
        a.state_out = c->cap_state + ((int64_t)(c->cap_cur ^ 1) * ns + s0) * 2;
      }
      a.item = static_cast<int32_t*>(pitem) + c0 * 2;
      a.out = out + c0 * out_stride;
      a.out_stride = out_stride;
      a.out_clip_len = out_clip_len;
      a.out_lens = out_lens + c0;
      LAUNCH(c, MMLA_STAGE_GLUE, (double)cnt * 16, capture_phase_launch(a, c->stream));
      LAUNCH(c, MMLA_STAGE_GLUE, (double)cnt * 2.0 * ((double)row + out_clip_len),
             capture_sample_launch(a, c->stream));
    }
    if (!fresh) c->cap_cur ^= 1;
    return MMLA_OK;
  }
};

// mmla_condition (kind FEATURES_OD) and mmla_{od,si,room}_pipeline_conditioned.  cap: the _capture calls,
// whose arguments describe the converted clips (the pointers only as non-null marks) -- every check first,
// then the conversion of all clips once, then the conditioned pipeline on the converted clips, which stay
// in the context's kept slots (internal.h)
int conditioned_call(mmla_ctx* c, CallKind kind, const Capture* cap, const int16_t* pcm, int64_t n,
                     int64_t stride, const int32_t* lens, int32_t clip_len, const int32_t* profile,
                     int32_t nr_passes, int32_t silence_remove, int64_t ips, int16_t* out_pcm,
                     int32_t* kept_len, const NetOut& o, uint32_t flags) {
  if (!c) return MMLA_E_INVALID;
  const bool dev = flags & MMLA_DEVICE_PTR;
  Conditioner cd{pcm, n, stride, lens, clip_len, profile, nr_passes, silence_remove, ips, out_pcm, kept_len,
                 (flags & MMLA_NR_NONSTATIONARY) != 0};
  if (const char* bad = cd.bad(c, dev)) return fail(c, MMLA_E_INVALID, "%s", bad);
  if (const char* m = missing_weights(c, kind)) return fail(c, MMLA_E_NOWEIGHTS, "%s weights not loaded", m);
  if (cap) {
    HIPCHK(c, hipSetDevice(c->device));
    void *pout = nullptr, *plens = nullptr;
    CHK(ws_get(c, S_CAP_CLIPS, (size_t)n * clip_len * sizeof(int16_t), &pout));
    CHK(ws_get(c, S_CAP_LENS, (size_t)n * sizeof(int32_t), &plens));
    CHK(cap->run(c, dev, static_cast<int16_t*>(pout), clip_len, static_cast<int32_t*>(plens)));
    cd.pcm = static_cast<const int16_t*>(pout);
    cd.lens = static_cast<const int32_t*>(plens);
    cd.pcm_dev = true;
  }
  return conditioned_body(c, kind, cd, o, flags);
}

int capture_pipeline(mmla_ctx* c, CallKind kind, const int16_t* pcm, int64_t n, int64_t stride,
                     const int32_t* frames, int32_t clip_frames, const int32_t* profile, int32_t nr_passes,
                     int32_t silence_remove, int64_t ips, int16_t* out_pcm, int32_t* kept_len,
                     const NetOut& o, uint32_t flags) {
  if (!c) return MMLA_E_INVALID;
  Capture cap{pcm, n, stride, frames, clip_frames, ips, false};
  if (const char* bad = cap.bad(c, flags & MMLA_DEVICE_PTR)) return fail(c, MMLA_E_INVALID, "%s", bad);
  const int32_t L = cap.out_clip_len;
  return conditioned_call(c, kind, &cap, pcm, n, L, nullptr, L, profile, nr_passes, silence_remove, ips,
                          out_pcm, kept_len, o, flags);
}

// ---- layered mixes (mix.hip): mmla_od_mix, mmla_od_pipeline_mixed ------------------------------------

static_assert(MIX_MAX_LAYERS == MMLA_MIX_MAX_LAYERS, "mix.h and mmla.h disagree");

// A mix call's pool and plan.  check() is every test that needs no device; stage() gives the device view
// (host mode: one upload per call into kept slots, which outlive a repeated micro-batch).
struct Mix {
  const int16_t* pool;
  int64_t pool_len, n;
  const int32_t* n_layers;
  const int64_t* src_off;
  const int32_t* src_len;
  const int32_t* pos;

  int check(mmla_ctx* c, bool dev) const {
    if (n < 0 || pool_len < 0 || (n > 0 && (!pool || !n_layers || !src_off || !src_len || !pos)))
      return fail(c, MMLA_E_INVALID, "bad mix args");
    if (dev) return MMLA_OK;   // a device plan cannot be seen here: the kernel reads inside the pool only
    for (int64_t i = 0; i < n; ++i) {
      if (n_layers[i] < 1 || n_layers[i] > MMLA_MIX_MAX_LAYERS)
        return fail(c, MMLA_E_INVALID, "mix clip %lld: %d layers outside 1..%d", (long long)i, n_layers[i],
                    MMLA_MIX_MAX_LAYERS);
      for (int l = 0; l < n_layers[i]; ++l) {
        const int64_t k = i * MMLA_MIX_MAX_LAYERS + l, off = src_off[k];
        const char* what = off < 0 ? "a negative offset" : src_len[k] < 0 ? "a negative length"
                           : pos[k] < 0 ? "a negative position"
                           : off > pool_len - src_len[k] ? "samples past the end of the pool" : nullptr;
        if (what)
          return fail(c, MMLA_E_INVALID, "mix clip %lld layer %d has %s (offset %lld, length %d, position %d, "
                      "pool %lld)", (long long)i, l, what, (long long)off, src_len[k], pos[k], (long long)pool_len);
      }
    }
    return MMLA_OK;
  }

  // -> a with pool and the four descriptor arrays as device pointers for clip 0
  int stage(mmla_ctx* c, bool dev, MixArgs* a) const {
    *a = MixArgs{};
    a->pool_len = pool_len;
    if (dev) {
      a->pool = pool;
      a->n_layers = n_layers;
      a->src_off = src_off;
      a->src_len = src_len;
      a->pos = pos;
      return MMLA_OK;
    }
    void *pp = nullptr, *pd = nullptr;
    CHK(ws_get(c, S_MIX_POOL, (size_t)pool_len * sizeof(int16_t), &pp));
    if (pool_len > 0)
      HIPCHK(c, hipMemcpyAsync(pp, pool, (size_t)pool_len * sizeof(int16_t), hipMemcpyHostToDevice, c->stream));
    // offsets first (8-byte aligned), then lengths, positions, layer counts
    const size_t m = (size_t)n * MMLA_MIX_MAX_LAYERS;
    CHK(ws_get(c, S_MIX_PLAN, m * 16 + (size_t)n * 4, &pd));
    char* d = static_cast<char*>(pd);
    const hipMemcpyKind k = hipMemcpyHostToDevice;
    HIPCHK(c, hipMemcpyAsync(d, src_off, m * 8, k, c->stream));
    HIPCHK(c, hipMemcpyAsync(d + m * 8, src_len, m * 4, k, c->stream));
    HIPCHK(c, hipMemcpyAsync(d + m * 12, pos, m * 4, k, c->stream));
    HIPCHK(c, hipMemcpyAsync(d + m * 16, n_layers, (size_t)n * 4, k, c->stream));
    a->pool = static_cast<const int16_t*>(pp);
    a->src_off = reinterpret_cast<const int64_t*>(d);
    a->src_len = reinterpret_cast<const int32_t*>(d + m * 8);
    a->pos = reinterpret_cast<const int32_t*>(d + m * 12);
    a->n_layers = reinterpret_cast<const int32_t*>(d + m * 16);
    return MMLA_OK;
  }
};

// clips [c0, c0 + cnt) of the staged plan `all` into out [cnt][out_stride], out_len [cnt] (device)
int mix_run(mmla_ctx* c, const MixArgs& all, int64_t c0, int64_t cnt, int32_t clip_len, int16_t* out,
            int64_t out_stride, int32_t* out_len) {
  MixArgs a = all;
  a.n_clips = cnt;
  a.n_layers += c0;
  a.src_off += c0 * MMLA_MIX_MAX_LAYERS;
  a.src_len += c0 * MMLA_MIX_MAX_LAYERS;
  a.pos += c0 * MMLA_MIX_MAX_LAYERS;
  a.clip_len = clip_len;
  a.out = out;
  a.out_stride = out_stride;
  a.out_len = out_len;
  // algorithmic bytes: the clip written, and at most one pool sample read per layer and sample
  LAUNCH(c, MMLA_STAGE_GLUE, (double)cnt * clip_len * 2.0 * (1 + MMLA_MIX_MAX_LAYERS), mix_launch(a, c->stream));
  return MMLA_OK;
}

}  // namespace

extern "C" {

int mmla_od_mix(mmla_ctx* c, const int16_t* pool, int64_t pool_len, int64_t n, const int32_t* n_layers,
                const int64_t* src_off, const int32_t* src_len, const int32_t* pos, int32_t clip_len,
                int16_t* out, int64_t out_stride, int32_t* out_len, uint32_t flags) {
  if (!c) return MMLA_E_INVALID;
  const bool dev0 = flags & MMLA_DEVICE_PTR;
  const Mix mix{pool, pool_len, n, n_layers, src_off, src_len, pos};
  if (clip_len < 1 || clip_len > 600000)
    return fail(c, MMLA_E_INVALID, "clip_len must be in [1, 600000]");
  if (n > 0 && (!out || out_stride < clip_len))
    return fail(c, MMLA_E_INVALID, "od_mix needs out and out_stride >= clip_len");
  CHK(mix.check(c, dev0));
  if (n == 0) return MMLA_OK;
  HIPCHK(c, hipSetDevice(c->device));
  MixArgs all;
  CHK(mix.stage(c, dev0, &all));
  return clip_call(c, FEATURES_OD, n, flags, nullptr, [&](int64_t c0, int64_t cnt, bool dev, const Arith&) -> int {
    if (dev) return mix_run(c, all, c0, cnt, clip_len, out + c0 * out_stride, out_stride, out_len ? out_len + c0 : nullptr);
    void *pm = nullptr, *pl = nullptr;
    CHK(ws_get(c, S_MIX, (size_t)cnt * clip_len * sizeof(int16_t), &pm));
    CHK(ws_get(c, S_MIX_LEN, (size_t)cnt * sizeof(int32_t), &pl));
    CHK(mix_run(c, all, c0, cnt, clip_len, static_cast<int16_t*>(pm), clip_len, static_cast<int32_t*>(pl)));
    HIPCHK(c, hipMemcpy2DAsync(out + c0 * out_stride, out_stride * sizeof(int16_t), pm, clip_len * sizeof(int16_t),
                               clip_len * sizeof(int16_t), cnt, hipMemcpyDeviceToHost, c->stream));
    if (out_len)
      HIPCHK(c, hipMemcpyAsync(out_len + c0, pl, (size_t)cnt * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    return MMLA_OK;
  });
}

int mmla_od_pipeline_mixed(mmla_ctx* c, const int16_t* pool, int64_t pool_len, int64_t n, const int32_t* n_layers,
                           const int64_t* src_off, const int32_t* src_len, const int32_t* pos, float* probs,
                           int32_t* argmax, uint8_t* silent, uint32_t flags) {
  if (!c) return MMLA_E_INVALID;
  const bool dev0 = flags & MMLA_DEVICE_PTR;
  const Mix mix{pool, pool_len, n, n_layers, src_off, src_len, pos};
  CHK(mix.check(c, dev0));
  if (const char* m = missing_weights(c, COND_OD)) return fail(c, MMLA_E_NOWEIGHTS, "%s weights not loaded", m);
  if (n == 0) return MMLA_OK;
  HIPCHK(c, hipSetDevice(c->device));
  MixArgs all;
  CHK(mix.stage(c, dev0, &all));
  // Per micro-batch: the mix into S_MIX / S_MIX_LEN, then mmla_od_pipeline's body on those clips with lens =
  // out_len under the range guard (a guard re-run repeats the network alone on the clips already mixed)
  return clip_call(c, COND_OD, n, flags, nullptr, [&](int64_t c0, int64_t cnt, bool dev, const Arith&) -> int {
    void *pm = nullptr, *pl = nullptr;
    CHK(ws_get(c, S_MIX, (size_t)cnt * MMLA_OD_CLIP * sizeof(int16_t), &pm));
    CHK(ws_get(c, S_MIX_LEN, (size_t)cnt * sizeof(int32_t), &pl));
    CHK(mix_run(c, all, c0, cnt, MMLA_OD_CLIP, static_cast<int16_t*>(pm), MMLA_OD_CLIP, static_cast<int32_t*>(pl)));
    const Pcm p{static_cast<const int16_t*>(pm), MMLA_OD_CLIP, static_cast<const int32_t*>(pl), MMLA_OD_CLIP, 0};
    return guarded(c, dev, c->od_f32_only, [&](const Arith& ar) -> int {
      return od_fe_net(c, ar, p, c0, cnt, dev, probs, argmax, silent);
    });
  });
}

int mmla_od_features(mmla_ctx* c, const int16_t* pcm, int64_t n, int64_t stride,
                     const int32_t* lens, int32_t clip_len, float* db, float* norm, float* zcr,
                     uint8_t* img, uint32_t flags) {
  return od_features_common(c, pcm, n, stride, lens, clip_len, db, norm, zcr, img, flags);
}

int mmla_od_features_f32(mmla_ctx* c, const float* y, int64_t n, int64_t stride,
                         const int32_t* lens, int32_t clip_len, float* db, float* norm, float* zcr,
                         uint8_t* img, uint32_t flags) {
  return od_features_common(c, y, n, stride, lens, clip_len, db, norm, zcr, img, flags);
}

int mmla_si_features(mmla_ctx* c, const int16_t* pcm, int64_t n, int64_t stride,
                     const int32_t* lens, int32_t clip_len, float* feat, uint8_t* silent,
                     uint32_t flags) {
  const bool bad = bad_pcm_args(pcm, n, stride, lens, clip_len) || (n > 0 && !feat);
  return clip_call(c, FEATURES_SI, n, flags, bad ? "bad pcm/feat args" : nullptr,
                   [&](int64_t c0, int64_t cnt, bool dev, const Arith&) -> int {
    Pcm p;
    CHK(stage_pcm(c, pcm, c0, cnt, stride, lens, clip_len, SI_NEED_SAMPLES, dev, &p));
    SiFeArgs a = si_fe_args(c, p);
    CHK(out_ptr(c, feat, c0 * SI_T * SI_D, cnt * SI_T * SI_D, dev, S_OUT0, &a.feat));
    CHK(out_ptr(c, silent, c0, cnt, dev, S_OUT1, &a.silent));
    LAUNCH(c, MMLA_STAGE_SI_FE, si_fe_bytes(cnt, a), si_fe_launch(a, cnt, c->stream));
    CHK(copy_back(c, feat, c0 * SI_T * SI_D, a.feat, cnt * SI_T * SI_D, dev));
    return copy_back(c, silent, c0, a.silent, cnt, dev);
  });
}

int mmla_si_features_seq(mmla_ctx* c, const int16_t* pcm, int64_t n_samples, int64_t n_windows,
                         float* feat, uint32_t flags) {
  if (!c) return MMLA_E_INVALID;
  if (n_samples < 1 || !pcm || !feat) return fail(c, MMLA_E_INVALID, "bad si_features_seq args");
  const int64_t T = n_samples <= 400 ? 1 : 1 + (n_samples - 400 + 159) / 160;
  if (n_windows != (T + SI_T - 1) / SI_T)
    return fail(c, MMLA_E_INVALID, "n_windows must be ceil(T/256) = %lld", (long long)((T + 255) / 256));
  HIPCHK(c, hipSetDevice(c->device));
  const bool dev = flags & MMLA_DEVICE_PTR;
  SiFeArgs a{};
  CHK(in_ptr(c, pcm, n_samples, dev, S_PCM, &a.pcm));
  a.seq_len = n_samples;
  a.tables = c->si_tables;
  CHK(out_ptr(c, feat, 0, n_windows * SI_T * SI_D, dev, S_OUT0, &a.feat));
  LAUNCH(c, MMLA_STAGE_SI_FE, (double)n_samples * 2 + (double)n_windows * SI_T * SI_D * 4,
         si_fe_launch(a, n_windows, c->stream));
  CHK(copy_back(c, feat, 0, a.feat, n_windows * SI_T * SI_D, dev));
  return finish(c, dev);
}

int mmla_si_features_seq_batch(mmla_ctx* c, const int16_t* pcm, int64_t n, int64_t stride, const int32_t* lens,
                               int32_t clip_len, float* feat, int32_t* n_windows, uint32_t flags) {
  if (!c) return MMLA_E_INVALID;
  if (n < 0 || n > 0x7fffffff || clip_len < 1 || (n > 0 && (!pcm || !feat)) || (n > 1 && stride < clip_len))
    return fail(c, MMLA_E_INVALID, "bad si_features_seq_batch args");
  const bool dev = flags & MMLA_DEVICE_PTR;
  if (n == 1) stride = std::max<int64_t>(stride, clip_len);   // one row: its width is clip_len
  // device-pointer lens cannot be seen here: the kernel clamps them into [0, clip_len]
  if (lens && !dev)
    for (int64_t i = 0; i < n; ++i)
      if (lens[i] < 0 || lens[i] > clip_len || lens[i] > stride)
        return fail(c, MMLA_E_INVALID, "lens[%lld] = %d outside [0, clip_len = %d]", (long long)i, lens[i], clip_len);
  if (n == 0) return MMLA_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const int64_t w_max = si_seq_windows(clip_len);
  SiFeArgs a{};
  a.pcm = pcm;
  a.clip_stride = stride;
  if (!dev) {   // the rows' first clip_len samples, dense
    void* dp = nullptr;
    CHK(ws_get(c, S_PCM, (size_t)n * clip_len * sizeof(int16_t), &dp));
    HIPCHK(c, hipMemcpy2DAsync(dp, (size_t)clip_len * sizeof(int16_t), pcm, (size_t)stride * sizeof(int16_t),
                               (size_t)clip_len * sizeof(int16_t), n, hipMemcpyHostToDevice, c->stream));
    a.pcm = static_cast<const int16_t*>(dp);
    a.clip_stride = clip_len;
  }
  CHK(in_ptr(c, lens, (size_t)n, dev, S_LENS, &a.lens));
  a.clip_len = clip_len;
  a.tables = c->si_tables;
  a.w_max = (int32_t)w_max;
  const size_t nf = (size_t)(n * w_max) * SI_T * SI_D;
  CHK(out_ptr(c, feat, 0, nf, dev, S_OUT0, &a.feat));
  CHK(out_ptr(c, n_windows, 0, (size_t)n, dev, S_OUT1, &a.n_windows));
  LAUNCH(c, MMLA_STAGE_SI_FE, (double)n * clip_len * 2 + (double)nf * 4, si_fe_launch(a, n, c->stream));
  CHK(copy_back(c, feat, 0, a.feat, nf, dev));
  CHK(copy_back(c, n_windows, 0, a.n_windows, (size_t)n, dev));
  return finish(c, dev);
}

int mmla_si_enrol_embed(mmla_ctx* c, const int16_t* pcm, int64_t n, int64_t stride, const int32_t* lens,
                        int32_t clip_len, const int32_t* profile, int32_t nr_passes, int32_t silence_remove,
                        int32_t vad_mode, int16_t* out_pcm, int32_t* kept_len, int32_t* n_windows, float* emb,
                        uint32_t flags) {
  if (!c) return MMLA_E_INVALID;
  const bool dev0 = flags & MMLA_DEVICE_PTR;
  Conditioner cd{pcm, n, stride, lens, clip_len, profile, nr_passes, silence_remove, 1, out_pcm, kept_len,
                 (flags & MMLA_NR_NONSTATIONARY) != 0};
  cd.enrol = true;
  cd.vad_mode = vad_mode;
  if (const char* bad = cd.bad(c, dev0)) return fail(c, MMLA_E_INVALID, "%s", bad);
  if (n > 0 && !emb) return fail(c, MMLA_E_INVALID, "null emb");
  if (const char* m = missing_weights(c, COND_SI)) return fail(c, MMLA_E_NOWEIGHTS, "%s weights not loaded", m);
  const int64_t w_max = si_seq_windows(clip_len);
  // Per micro-batch of recordings (SI's cap, counted in recordings): the conditioning, the batched
  // sequence front-end on the conditioned int16 with lens = kept_len, then SI-NET up to the BiLSTM on the
  // cnt * w_max windows in micro-batches of that many windows, each under mmla_si_embed's range guard.
  // A window's embedding does not depend on where it sits in a batch, so neither size enters the result
  return clip_call(c, COND_SI, n, flags, nullptr, [&](int64_t c0, int64_t cnt, bool dev, const Arith&) -> int {
    CHK(cd.run(c, c0, cnt, dev));
    const int64_t nwin = cnt * w_max;
    void *pf = nullptr, *pw = nullptr;
    CHK(ws_get(c, S_FEAT, (size_t)nwin * SI_T * SI_D * sizeof(float), &pf));
    CHK(ws_get(c, S_ENROL_NW, (size_t)cnt * sizeof(int32_t), &pw));
    SiFeArgs a{};
    a.pcm = cd.q;
    a.clip_stride = clip_len;
    a.lens = cd.kept;
    a.clip_len = clip_len;
    a.tables = c->si_tables;
    a.feat = static_cast<float*>(pf);
    a.ldf = SI_D;
    a.w_max = (int32_t)w_max;
    a.n_windows = static_cast<int32_t*>(pw);
    LAUNCH(c, MMLA_STAGE_SI_FE, (double)cnt * clip_len * 2 + (double)nwin * SI_T * SI_D * 4,
           si_fe_launch(a, cnt, c->stream));
    const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (n_windows)
      HIPCHK(c, hipMemcpyAsync(n_windows + c0, a.n_windows, (size_t)cnt * sizeof(int32_t), kind, c->stream));
    const int64_t mb = std::max<int64_t>(1, microbatch(c, false));
    for (int64_t w0 = 0; w0 < nwin; w0 += mb) {
      const int64_t wc = std::min(mb, nwin - w0);
      CHK(guarded(c, dev, c->si_f32_only, [&](const Arith& ar) -> int {
        const float* h = nullptr;
        CHK(run_si_net(c, ar, a.feat + w0 * SI_T * SI_D, wc, nullptr, nullptr, nullptr, SI_D, 11, &h));
        HIPCHK(c, hipMemcpyAsync(emb + (c0 * w_max + w0) * MMLA_SI_EMBED, h,
                                 (size_t)wc * MMLA_SI_EMBED * sizeof(float), kind, c->stream));
        return MMLA_OK;
      }));
    }
    return MMLA_OK;
  });
}

int mmla_od_forward(mmla_ctx* c, const float* x, int64_t n, float* probs, uint32_t flags) {
  return od_forward_common(c, x, nullptr, n, probs, flags);
}

int mmla_od_forward_u8(mmla_ctx* c, const uint8_t* img, int64_t n, float* probs, uint32_t flags) {
  return od_forward_common(c, nullptr, img, n, probs, flags);
}

int mmla_si_forward(mmla_ctx* c, const float* x, int64_t n, float* probs, uint32_t flags) {
  const bool bad = n < 0 || (n > 0 && (!x || !probs));
  return clip_call(c, NET_SI, n, flags, bad ? "bad si_forward args" : nullptr,
                   [&](int64_t c0, int64_t cnt, bool dev, const Arith& ar) -> int {
    const int k = c->si.k;
    const float* dx;
    CHK(in_ptr(c, x + c0 * SI_T * SI_D, cnt * SI_T * SI_D, dev, S_IN, &dx));
    float* dp;
    CHK(out_ptr(c, probs, c0 * k, cnt * k, dev, S_OUT0, &dp));
    CHK(run_si_net(c, ar, dx, cnt, dp, nullptr, nullptr));
    return copy_back(c, probs, c0 * k, dp, cnt * k, dev);
  });
}

int mmla_si_embed(mmla_ctx* c, const float* x, int64_t n, float* emb, uint32_t flags) {
  const bool bad = n < 0 || (n > 0 && (!x || !emb));
  return clip_call(c, NET_SI, n, flags, bad ? "bad si_embed args" : nullptr,
                   [&](int64_t c0, int64_t cnt, bool dev, const Arith& ar) -> int {
    const float *dx, *h = nullptr;
    CHK(in_ptr(c, x + c0 * SI_T * SI_D, cnt * SI_T * SI_D, dev, S_IN, &dx));
    CHK(run_si_net(c, ar, dx, cnt, nullptr, nullptr, nullptr, SI_D, 11, &h));
    // the BiLSTM's own output buffer (S_HOUT) handed out: one copy, to the device or to the host
    HIPCHK(c, hipMemcpyAsync(emb + c0 * MMLA_SI_EMBED, h, (size_t)cnt * MMLA_SI_EMBED * sizeof(float),
                             dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
    return MMLA_OK;
  });
}

int mmla_od_pipeline(mmla_ctx* c, const int16_t* pcm, int64_t n, int64_t stride,
                     const int32_t* lens, int32_t clip_len, float* probs, int32_t* argmax,
                     uint8_t* silent, uint32_t flags) {
  return od_pipeline_common(c, pcm, n, stride, lens, clip_len, false, 0, 0.0f, probs, argmax, silent,
                            nullptr, flags);
}

int mmla_od_pipeline_gated(mmla_ctx* c, const int16_t* pcm, int64_t n, int64_t stride,
                           const int32_t* lens, int32_t clip_len, int32_t nr_passes,
                           float ssim_threshold, float* probs, int32_t* argmax, uint8_t* silent,
                           float* ssim, uint32_t flags) {
  return od_pipeline_common(c, pcm, n, stride, lens, clip_len, true, nr_passes, ssim_threshold, probs,
                            argmax, silent, ssim, flags);
}

int mmla_ssim_u8(mmla_ctx* c, const uint8_t* a, const uint8_t* b, int64_t n, int32_t h, int32_t w,
                 int32_t ch, float* out, uint32_t flags) {
  if (!c) return MMLA_E_INVALID;
  if (h < SSIM_WIN || w < SSIM_WIN || (ch != 1 && ch != 3 && ch != 4))
    return fail(c, MMLA_E_INVALID, "ssim needs h, w >= 7 and 1, 3 or 4 channels (got %d x %d x %d)", h, w, ch);
  const int64_t per = (int64_t)h * w * ch;
  if (n < 0 || n > 0x7fffffff || (int64_t)w * ch > (1 << 30) || (n > 0 && (!a || !b || !out)))
    return fail(c, MMLA_E_INVALID, "bad ssim args");
  if (n == 0) return MMLA_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const bool dev = flags & MMLA_DEVICE_PTR;
  const uint8_t *da, *db;
  float* ds;
  CHK(in_ptr(c, a, (size_t)(n * per), dev, S_IMG, &da));
  CHK(in_ptr(c, b, (size_t)(n * per), dev, S_IMG2, &db));
  CHK(out_ptr(c, out, 0, (size_t)n, dev, S_OUT0, &ds));
  LAUNCH(c, MMLA_STAGE_OD_FE, (double)n * (2.0 * per + 4), ssim_u8_launch(da, db, n, h, w, ch, ds, c->stream));
  CHK(copy_back(c, out, 0, ds, (size_t)n, dev));
  return finish(c, dev);
}

int mmla_si_pipeline(mmla_ctx* c, const int16_t* pcm, int64_t n, int64_t stride,
                     const int32_t* lens, int32_t clip_len, float* probs, int32_t* argmax,
                     uint8_t* silent, uint32_t flags) {
  return si_pipeline_common(c, pcm, n, stride, lens, clip_len, probs, argmax, silent, flags);
}

int mmla_condition(mmla_ctx* c, const int16_t* pcm, int64_t n, int64_t stride, const int32_t* lens,
                   int32_t clip_len, const int32_t* profile, int32_t nr_passes, int32_t silence_remove,
                   int64_t items_per_stream, int16_t* out_pcm, int32_t* kept_len, uint32_t flags) {
  return conditioned_call(c, FEATURES_OD, nullptr, pcm, n, stride, lens, clip_len, profile, nr_passes,
                          silence_remove, items_per_stream, out_pcm, kept_len, NetOut{}, flags);
}

int mmla_od_pipeline_conditioned(mmla_ctx* c, const int16_t* pcm, int64_t n, int64_t stride,
                                 const int32_t* lens, int32_t clip_len, const int32_t* profile,
                                 int32_t nr_passes, int32_t silence_remove, int64_t items_per_stream,
                                 int16_t* out_pcm, int32_t* kept_len, float* probs, int32_t* argmax,
                                 uint8_t* silent, uint32_t flags) {
  return conditioned_call(c, COND_OD, nullptr, pcm, n, stride, lens, clip_len, profile, nr_passes,
                          silence_remove, items_per_stream, out_pcm, kept_len,
                          NetOut{probs, argmax, nullptr, nullptr, silent}, flags);
}

int mmla_si_pipeline_conditioned(mmla_ctx* c, const int16_t* pcm, int64_t n, int64_t stride,
                                 const int32_t* lens, int32_t clip_len, const int32_t* profile,
                                 int32_t nr_passes, int32_t silence_remove, int64_t items_per_stream,
                                 int16_t* out_pcm, int32_t* kept_len, float* probs, int32_t* argmax,
                                 uint8_t* silent, uint32_t flags) {
  return conditioned_call(c, COND_SI, nullptr, pcm, n, stride, lens, clip_len, profile, nr_passes,
                          silence_remove, items_per_stream, out_pcm, kept_len,
                          NetOut{nullptr, nullptr, probs, argmax, silent}, flags);
}

// Both detectors on one conditioning (conditioned_body)
int mmla_room_pipeline_conditioned(mmla_ctx* c, const int16_t* pcm, int64_t n, int64_t stride,
                                   const int32_t* lens, int32_t clip_len, const int32_t* profile,
                                   int32_t nr_passes, int32_t silence_remove, int64_t items_per_stream,
                                   int16_t* out_pcm, int32_t* kept_len, float* od_probs,
                                   int32_t* od_argmax, float* si_probs, int32_t* si_argmax,
                                   uint8_t* silent, uint32_t flags) {
  return conditioned_call(c, COND_ROOM, nullptr, pcm, n, stride, lens, clip_len, profile, nr_passes,
                          silence_remove, items_per_stream, out_pcm, kept_len,
                          NetOut{od_probs, od_argmax, si_probs, si_argmax, silent}, flags);
}

// ---- a room's capture format (resample.hip capture_*_kernel) ----------------------------------------

int mmla_capture_reset(mmla_ctx* c, int64_t n_streams, int32_t rate, int32_t channels, int32_t channel) {
  if (!c) return MMLA_E_INVALID;
  if (n_streams < 1) return fail(c, MMLA_E_INVALID, "n_streams must be >= 1");
  if (rate < 1 || rate > 384000) return fail(c, MMLA_E_INVALID, "capture rate %d outside 1..384000", rate);
  if (channels < 1 || channels > 8) return fail(c, MMLA_E_INVALID, "%d capture channels outside 1..8", channels);
  if (channel >= channels || channel < MMLA_CAPTURE_MEAN)
    return fail(c, MMLA_E_INVALID, "channel %d of %d", channel, channels);
  if (channel == MMLA_CAPTURE_MEAN && channels != 2)
    return fail(c, MMLA_E_INVALID, "MMLA_CAPTURE_MEAN needs 2 channels, got %d", channels);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const int g = std::gcd(rate, 16000);
  std::vector<int32_t> h((size_t)n_streams * 2);
  for (int64_t s = 0; s < n_streams; ++s) {   // a fresh audioop state: d = -outrate, prev = 0
    h[2 * s] = -(16000 / g);
    h[2 * s + 1] = 0;
  }
  if (c->cap_streams != n_streams) {
    if (c->cap_state) HIPCHK(c, hipFree(c->cap_state));
    c->cap_state = nullptr;
    c->cap_streams = 0;
    c->cap_rate = 0;
    if (hipMalloc(&c->cap_state, 4 * n_streams * sizeof(int32_t)) != hipSuccess) {
      (void)hipGetLastError();
      c->cap_state = nullptr;
      return fail(c, MMLA_E_OOM, "capture state for %lld streams", (long long)n_streams);
    }
  }
  HIPCHK(c, hipMemcpy(c->cap_state, h.data(), h.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  c->cap_cur = 0;
  c->cap_streams = n_streams;
  c->cap_rate = rate;
  c->cap_channels = channels;
  c->cap_channel = channel;
  c->cap_ir = rate / g;
  c->cap_or = 16000 / g;
  return MMLA_OK;
}

int mmla_capture_state(mmla_ctx* c, int32_t* d, int32_t* prev) {
  if (!c) return MMLA_E_INVALID;
  if (!c->cap_state || !c->cap_rate) return fail(c, MMLA_E_INVALID, "mmla_capture_reset must be called first");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::vector<int32_t> h((size_t)c->cap_streams * 2);
  HIPCHK(c, hipMemcpy(h.data(), c->cap_state + (int64_t)c->cap_cur * c->cap_streams * 2,
                      h.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  for (int64_t s = 0; s < c->cap_streams; ++s) {
    if (d) d[s] = h[2 * s];
    if (prev) prev[s] = h[2 * s + 1];
  }
  return MMLA_OK;
}

int mmla_capture_convert(mmla_ctx* c, const int16_t* pcm, int64_t n, int64_t stride, const int32_t* frames,
                         int32_t clip_frames, int64_t items_per_stream, int16_t* out, int64_t out_stride,
                         int32_t* out_lens, uint32_t flags) {
  if (!c) return MMLA_E_INVALID;
  const bool dev = flags & MMLA_DEVICE_PTR;
  Capture cap{pcm, n, stride, frames, clip_frames, items_per_stream, (flags & MMLA_CAPTURE_FRESH) != 0};
  if (const char* bad = cap.bad(c, dev)) return fail(c, MMLA_E_INVALID, "%s", bad);
  const int32_t L = cap.out_clip_len;
  if (n > 0 && (!out || !out_lens || out_stride < L))
    return fail(c, MMLA_E_INVALID, "capture_convert needs out, out_lens and out_stride >= out_clip_len = %d", L);
  if (n == 0) return MMLA_OK;
  HIPCHK(c, hipSetDevice(c->device));
  if (dev) {
    CHK(cap.run(c, true, out, out_stride, out_lens));
    return finish(c, true);
  }
  void *pout = nullptr, *plens = nullptr;
  CHK(ws_get(c, S_CAP_CLIPS, (size_t)n * L * sizeof(int16_t), &pout));
  CHK(ws_get(c, S_CAP_LENS, (size_t)n * sizeof(int32_t), &plens));
  CHK(cap.run(c, false, static_cast<int16_t*>(pout), L, static_cast<int32_t*>(plens)));
  HIPCHK(c, hipMemcpy2DAsync(out, out_stride * sizeof(int16_t), pout, L * sizeof(int16_t), L * sizeof(int16_t),
                             n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(out_lens, plens, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  return finish(c, false);
}

int mmla_od_pipeline_capture(mmla_ctx* c, const int16_t* pcm, int64_t n, int64_t stride,
                             const int32_t* frames, int32_t clip_frames, const int32_t* profile,
                             int32_t nr_passes, int32_t silence_remove, int64_t items_per_stream,
                             int16_t* out_pcm, int32_t* kept_len, float* probs, int32_t* argmax,
                             uint8_t* silent, uint32_t flags) {
  return capture_pipeline(c, COND_OD, pcm, n, stride, frames, clip_frames, profile, nr_passes, silence_remove,
                          items_per_stream, out_pcm, kept_len, NetOut{probs, argmax, nullptr, nullptr, silent},
                          flags);
}

int mmla_si_pipeline_capture(mmla_ctx* c, const int16_t* pcm, int64_t n, int64_t stride,
                             const int32_t* frames, int32_t clip_frames, const int32_t* profile,
                             int32_t nr_passes, int32_t silence_remove, int64_t items_per_stream,
                             int16_t* out_pcm, int32_t* kept_len, float* probs, int32_t* argmax,
                             uint8_t* silent, uint32_t flags) {
  return capture_pipeline(c, COND_SI, pcm, n, stride, frames, clip_frames, profile, nr_passes, silence_remove,
                          items_per_stream, out_pcm, kept_len, NetOut{nullptr, nullptr, probs, argmax, silent},
                          flags);
}

int mmla_room_pipeline_capture(mmla_ctx* c, const int16_t* pcm, int64_t n, int64_t stride,
                               const int32_t* frames, int32_t clip_frames, const int32_t* profile,
                               int32_t nr_passes, int32_t silence_remove, int64_t items_per_stream,
                               int16_t* out_pcm, int32_t* kept_len, float* od_probs, int32_t* od_argmax,
                               float* si_probs, int32_t* si_argmax, uint8_t* silent, uint32_t flags) {
  return capture_pipeline(c, COND_ROOM, pcm, n, stride, frames, clip_frames, profile, nr_passes, silence_remove,
                          items_per_stream, out_pcm, kept_len,
                          NetOut{od_probs, od_argmax, si_probs, si_argmax, silent}, flags);
}

int mmla_debug_od_trace(mmla_ctx* c, const float* x, int64_t n, int stage, float* out,
                        int64_t out_floats) {
  if (!c || !x || !out || n < 1 || stage < 0 || stage > 11) return MMLA_E_INVALID;
  if (!c->od_loaded) return fail(c, MMLA_E_NOWEIGHTS, "OD weights not loaded");
  HIPCHK(c, hipSetDevice(c->device));
  const float* dx;
  CHK(od_net_input(c, x, n, false, S_IN, &dx));
  auto body = [&](const Arith& ar) -> int {
    const float* tap = nullptr;
    int64_t tn = 0;
    CHK(run_od_net(c, ar, nullptr, dx, n, nullptr, nullptr, OdGate(), stage, &tap, &tn));
    if (tn > out_floats) return fail(c, MMLA_E_SHAPE, "trace stage %d needs %lld floats", stage, (long long)tn);
    HIPCHK(c, hipMemcpyAsync(out, tap, tn * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MMLA_OK;
  };
  // the trace shows what the selected arithmetic computes, unguarded.  MMLA_DEBUG_TRACE_GUARD=1 at
  // mmla_create: one host-pointer micro-batch under the range guard, like mmla_od_forward's -- an
  // operand out of range in a kernel up to `stage` re-runs the trace in exact f32 and counts in
  // mmla_range_check, so a test can tell which block's guard fired (the blocks behind `stage` do not run)
  return c->debug_trace_guard ? guarded(c, false, c->od_f32_only, body) : body(unguarded(c));
}

int mmla_debug_si_trace(mmla_ctx* c, const float* x, int64_t n, int stage, float* out,
                        int64_t out_floats) {
  if (!c || !x || !out || n < 1 || stage < 0 || stage > 12) return MMLA_E_INVALID;
  if (!c->si_loaded) return fail(c, MMLA_E_NOWEIGHTS, "SI weights not loaded");
  HIPCHK(c, hipSetDevice(c->device));
  const float* dx;
  CHK(in_ptr(c, x, n * SI_T * SI_D, false, S_IN, &dx));
  auto body = [&](const Arith& ar) -> int {
    const float* tap = nullptr;
    int64_t tn = 0;
    CHK(run_si_net(c, ar, dx, n, nullptr, nullptr, nullptr, SI_D, stage, &tap, &tn));
    // the logits: the first K columns of each cout_pad row
    const int64_t k = c->si.k, ld = stage == 12 ? c->si.dense.cout_pad : 0;
    if (stage == 12) tn = n * k;
    if (tn > out_floats) return fail(c, MMLA_E_SHAPE, "trace stage %d needs %lld floats", stage, (long long)tn);
    if (stage == 12)
      HIPCHK(c, hipMemcpy2DAsync(out, k * sizeof(float), tap, ld * sizeof(float), k * sizeof(float), n,
                                 hipMemcpyDeviceToHost, c->stream));
    else
      HIPCHK(c, hipMemcpyAsync(out, tap, tn * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MMLA_OK;
  };
  // mmla_debug_od_trace's two modes: unguarded, or (MMLA_DEBUG_TRACE_GUARD=1) one guarded host micro-batch
  return c->debug_trace_guard ? guarded(c, false, c->si_f32_only, body) : body(unguarded(c));
}

}  // extern "C"
