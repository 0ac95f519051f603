// libmmla C ABI, the auxiliary entry points: CRC-32C and PNG helpers (host only), the stationary and
// the non-stationary noise gate, silence removal, PCM conversion and the two resamplers.  The context, the weights, the
// network runners and the feature / pipeline entry points live in the files internal.h lists.
// See include/mmla.h for the contract and the reference call site each entry point replaces.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <numeric>

#include "fit_common.h"
#include "internal.h"
#include "resample.h"
#include "si_train.h"

using namespace mmla;

extern "C" {

// CRC-32C (Castagnoli, reflected polynomial 0x82F63B78), slice-by-8 tables built once
static uint32_t g_crc_tab[8][256];
static void crc32c_tables() {
  for (uint32_t i = 0; i < 256; ++i) {
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0x82F63B78u : c >> 1;
    g_crc_tab[0][i] = c;
  }
  for (uint32_t i = 0; i < 256; ++i)
    for (int t = 1; t < 8; ++t) g_crc_tab[t][i] = (g_crc_tab[t - 1][i] >> 8) ^ g_crc_tab[0][g_crc_tab[t - 1][i] & 255];
}

int mmla_crc32c(const void* data, int64_t n, uint32_t* crc) {
  if ((!data && n > 0) || n < 0 || !crc) return MMLA_E_INVALID;
  static const bool ready = (crc32c_tables(), true);
  (void)ready;
  const unsigned char* p = static_cast<const unsigned char*>(data);
  uint32_t c = 0xFFFFFFFFu;
  int64_t i = 0;
  for (; i + 8 <= n; i += 8) {
    uint32_t lo, hi;
    memcpy(&lo, p + i, 4);
    memcpy(&hi, p + i + 4, 4);
    lo ^= c;
    c = g_crc_tab[7][lo & 255] ^ g_crc_tab[6][(lo >> 8) & 255] ^ g_crc_tab[5][(lo >> 16) & 255] ^
        g_crc_tab[4][lo >> 24] ^ g_crc_tab[3][hi & 255] ^ g_crc_tab[2][(hi >> 8) & 255] ^
        g_crc_tab[1][(hi >> 16) & 255] ^ g_crc_tab[0][hi >> 24];
  }
  for (; i < n; ++i) c = g_crc_tab[0][(c ^ p[i]) & 255] ^ (c >> 8);
  *crc = c ^ 0xFFFFFFFFu;
  return MMLA_OK;
}

int mmla_debug_od_image_lut(int32_t type, uint8_t* rgb) {
  const uint32_t* lut = od_fe_lut(type);
  if (!lut || !rgb) return MMLA_E_INVALID;
  for (int i = 0; i < 256; ++i)
    for (int ch = 0; ch < 3; ++ch) rgb[3 * i + ch] = (uint8_t)(lut[i] >> (8 * ch));
  return MMLA_OK;
}

int mmla_png_unfilter(const uint8_t* raw, int64_t h, int64_t row_bytes, int32_t bpp, uint8_t* out) {
  if (h < 0 || row_bytes < 0 || bpp < 1 || bpp > 8 || ((!raw || !out) && h * row_bytes > 0))
    return MMLA_E_INVALID;
  const uint8_t* prev = nullptr;  // row above (all zero for the first row)
  for (int64_t r = 0; r < h; ++r) {
    const uint8_t* in = raw + r * (row_bytes + 1);
    uint8_t* cur = out + r * row_bytes;
    const int ft = in[0];
    ++in;
    switch (ft) {
      case 0:
        memcpy(cur, in, (size_t)row_bytes);
        break;
      case 1:  // Sub
        for (int64_t i = 0; i < row_bytes; ++i)
          cur[i] = (uint8_t)(in[i] + (i >= bpp ? cur[i - bpp] : 0));
        break;
      case 2:  // Up
        for (int64_t i = 0; i < row_bytes; ++i) cur[i] = (uint8_t)(in[i] + (prev ? prev[i] : 0));
        break;
      case 3:  // Average (floor of the 9-bit sum)
        for (int64_t i = 0; i < row_bytes; ++i) {
          const int a = i >= bpp ? cur[i - bpp] : 0, b = prev ? prev[i] : 0;
          cur[i] = (uint8_t)(in[i] + ((a + b) >> 1));
        }
        break;
      case 4:  // Paeth
        for (int64_t i = 0; i < row_bytes; ++i) {
          const int a = i >= bpp ? cur[i - bpp] : 0, b = prev ? prev[i] : 0;
          const int c = (prev && i >= bpp) ? prev[i - bpp] : 0;
          const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
          cur[i] = (uint8_t)(in[i] + ((pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c)));
        }
        break;
      default:
        return MMLA_E_INVALID;
    }
    prev = cur;
  }
  return MMLA_OK;
}

// ---- stationary noise gate ----------------------------------------------------

namespace {
constexpr int64_t kNrChunk = 600000, kNrPadding = 30000;   // noisereduce 2.0 defaults
constexpr int64_t kNrItemsPerLaunch = 512;                  // ~3.4 GB of scratch per launch (2.5 s)
}  // namespace

// the gate's device tables, built on first use by whichever gate comes first (the 33 x 7 smoothing
// filter is the same for every sample rate that has one)
static int nr_tables_ready(mmla_ctx* c, int32_t sr) {
  if (c->nr_tables) return MMLA_OK;
  NrTables t;
  nr_build_tables(&t, sr);
  if (t.ngf != NR_NGF || t.ngt != NR_NGT) return fail(c, MMLA_E_INVALID, "smoothing filter shape");
  HIPCHK(c, hipMalloc(&c->nr_tables, sizeof(NrTables)));
  HIPCHK(c, hipMemcpy(c->nr_tables, &t, sizeof(t), hipMemcpyHostToDevice));
  return MMLA_OK;
}

// the body of both profile setters: profile p = noise + p * stride, lens[p] (nullable: len) samples
static int nr_set_bank(mmla_ctx* c, const float* noise, int64_t n_profiles, int64_t stride,
                       const int32_t* lens, int64_t len, int32_t sr, uint32_t flags) {
  if (!noise || len < 2) return fail(c, MMLA_E_INVALID, "noise clip needs >= 2 samples");
  if (n_profiles < 1 || n_profiles > 65535 || (n_profiles > 1 && stride < len))
    return fail(c, MMLA_E_INVALID, "bad noise bank (%lld profiles of %lld samples at stride %lld)",
                (long long)n_profiles, (long long)len, (long long)stride);
  if (sr != 16000) return fail(c, MMLA_E_INVALID, "noise gate supports sr = 16000 (got %d)", sr);
  const bool dev = flags & MMLA_DEVICE_PTR;
  // device-pointer lens cannot be seen here: the kernels clamp them into [2, len]
  if (lens && !dev)
    for (int64_t p = 0; p < n_profiles; ++p)
      if (lens[p] < 2 || lens[p] > len)
        return fail(c, MMLA_E_INVALID, "noise lens[%lld] = %d outside [2, %lld]", (long long)p, lens[p],
                    (long long)len);
  HIPCHK(c, hipSetDevice(c->device));
  constexpr int64_t bins = NR_NFFT / 2 + 1;
  CHK(nr_tables_ready(c, sr));
  if (c->nr_profiles != n_profiles) {
    HIPCHK(c, hipStreamSynchronize(c->stream));   // a gate still reading the old bank
    if (c->nr_thresh) HIPCHK(c, hipFree(c->nr_thresh));
    c->nr_thresh = nullptr;
    c->nr_profiles = 0;
    c->nr_ready = false;
    HIPCHK(c, hipMalloc(&c->nr_thresh, (size_t)n_profiles * bins * sizeof(float)));
    c->nr_profiles = n_profiles;
  }
  const int64_t m = std::min(len, kNrChunk);   // clip_noise_stationary: y_noise[:chunk_size]
  const int64_t Tmax = 1 + m / NR_HOP;
  NrNoiseArgs a{};
  void *pdb = nullptr, *pmx = nullptr;
  CHK(in_ptr(c, noise, (size_t)((n_profiles - 1) * stride + m), dev, S_IN, &a.noise));
  CHK(in_ptr(c, lens, (size_t)n_profiles, dev, S_NR_PROF, &a.lens));
  CHK(ws_get(c, S_NR_FRAMES, (size_t)n_profiles * Tmax * bins * sizeof(float), &pdb));
  CHK(ws_get(c, S_NR_FMAX, (size_t)n_profiles * Tmax * sizeof(float), &pmx));
  a.stride = stride;
  a.m = m;
  a.n_profiles = (int)n_profiles;
  a.tables = c->nr_tables;
  a.db = static_cast<float*>(pdb);
  a.fmaxv = static_cast<float*>(pmx);
  a.n_std = 1.5f;
  a.thresh = c->nr_thresh;
  LAUNCH(c, MMLA_STAGE_NR, (double)n_profiles * m * 4, nr_noise_launch(a, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));   // one synchronisation per bank
  c->nr_ready = true;
  c->nr_bank_sr = sr;
  return MMLA_OK;
}

int mmla_nr_set_nonstationary(mmla_ctx* c, double time_constant_s, double thresh_n_mult,
                              double sigmoid_slope, int32_t sr) {
  if (!c) return MMLA_E_INVALID;
  if (!std::isfinite(time_constant_s) || time_constant_s <= 0 || !std::isfinite(sigmoid_slope) ||
      sigmoid_slope <= 0 || !std::isfinite(thresh_n_mult))
    return fail(c, MMLA_E_INVALID, "non-stationary gate: time_constant_s and sigmoid_slope must be finite and > 0, thresh_n_mult finite");
  if (sr <= 0) return fail(c, MMLA_E_INVALID, "non-stationary gate: sr = %d", sr);
  NrTables t;
  nr_build_tables(&t, sr);
  if (t.ngf != NR_NGF || t.ngt != NR_NGT)
    return fail(c, MMLA_E_INVALID, "non-stationary gate: the smoothing filter at sr = %d is %d x %d, not %d x %d",
                sr, t.ngf, t.ngt, NR_NGF, NR_NGT);
  if (c->nr_ready && c->nr_bank_sr != sr)
    return fail(c, MMLA_E_INVALID, "non-stationary gate: sr = %d differs from the noise bank's %d", sr,
                c->nr_bank_sr);
  c->ns_time_constant_s = time_constant_s;
  c->ns_thresh_n_mult = thresh_n_mult;
  c->ns_sigmoid_slope = sigmoid_slope;
  c->ns_sr = sr;
  return MMLA_OK;
}

int mmla_nr_set_noise(mmla_ctx* c, const float* noise, int64_t n_noise, int32_t sr, uint32_t flags) {
  if (!c) return MMLA_E_INVALID;
  // a bank of one, in slot 0 (only the first chunk_size samples enter the profile)
  return nr_set_bank(c, noise, 1, 0, nullptr, std::min(n_noise, kNrChunk), sr, flags);
}

int mmla_nr_set_noise_bank(mmla_ctx* c, const float* noise, int64_t n_profiles, int64_t stride,
                           const int32_t* lens, int32_t len, int32_t sr, uint32_t flags) {
  if (!c) return MMLA_E_INVALID;
  return nr_set_bank(c, noise, n_profiles, stride, lens, len, sr, flags);
}

int mmla_debug_nr_thresh(mmla_ctx* c, float* thresh, int64_t cap_floats, int64_t* n_profiles) {
  if (!c) return MMLA_E_INVALID;
  if (!c->nr_ready || !c->nr_thresh) return fail(c, MMLA_E_INVALID, "mmla_nr_set_noise must be called first");
  constexpr int64_t bins = NR_NFFT / 2 + 1;
  if (n_profiles) *n_profiles = c->nr_profiles;
  if (!thresh || cap_floats < c->nr_profiles * bins)
    return fail(c, MMLA_E_INVALID, "thresholds need %lld floats (got room for %lld)",
                (long long)(c->nr_profiles * bins), (long long)cap_floats);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(thresh, c->nr_thresh, (size_t)c->nr_profiles * bins * sizeof(float), hipMemcpyDeviceToHost));
  return MMLA_OK;
}

}  // extern "C"

// the gate of mmla_nr_reduce on device pointers; mmla_od_pipeline_gated runs its passes through it too
int mmla::nr_reduce_dev(mmla_ctx* c, const float* dy, int64_t n_signals, int64_t stride, int64_t len,
                        float* dout, const int32_t* dprofile, bool nonstationary) {
  if (!nonstationary && !c->nr_ready) return fail(c, MMLA_E_INVALID, "mmla_nr_set_noise must be called first");
  if (n_signals <= 0 || len <= 0) return MMLA_OK;
  NrNsParams ns{};
  if (nonstationary) {
    CHK(nr_tables_ready(c, c->ns_sr));
    ns.b = nr_ns_coefficient(c->ns_time_constant_s, c->ns_sr);
    ns.one_minus_b = -(ns.b - 1.0);   // scipy's lfilter forms -a[1] of a = [1, b - 1]
    ns.shift = c->ns_thresh_n_mult;
    ns.slope = c->ns_sigmoid_slope;
  }
  // SpectralGate.get_traces: one chunk of `len` when len <= chunk_size, else chunk_size pieces
  const int64_t keep = len <= kNrChunk ? len : kNrChunk;
  const int64_t per = (len + keep - 1) / keep;
  const int64_t L = keep + 2 * kNrPadding;
  const int T = (int)(1 + L / NR_HOP);
  const int64_t bins = NR_NFFT / 2 + 1;
  const int64_t cap = std::max<int64_t>(1, std::min<int64_t>(kNrItemsPerLaunch, (int64_t)(2e10 / ((double)T * (bins * 25 + NR_NFFT * 8 + 8)))));
  std::vector<NrItem> items;
  items.reserve(n_signals * per);
  for (int64_t sgl = 0; sgl < n_signals; ++sgl)
    for (int64_t k = 0; k < per; ++k)
      items.push_back(NrItem{sgl * stride, len, k * keep - kNrPadding, sgl * len + k * keep,
                             std::min(keep, len - k * keep), sgl});
  for (size_t i0 = 0; i0 < items.size(); i0 += cap) {
    const int64_t ni = std::min<int64_t>(cap, (int64_t)items.size() - (int64_t)i0);
    void *pS, *pB, *pM, *pF, *pI, *pR;
    CHK(ws_get(c, S_NR_S, (size_t)ni * T * bins * sizeof(double2), &pS));
    pB = pM = nullptr;   // the non-stationary gate has no threshold bits and no dB maxima
    if (!nonstationary) {
      CHK(ws_get(c, S_NR_BITS, (size_t)ni * T * bins, &pB));
      CHK(ws_get(c, S_NR_FMAX, (size_t)ni * (T + 1) * sizeof(double), &pM));
    }
    CHK(ws_get(c, S_NR_FRAMES, (size_t)ni * T * NR_NFFT * sizeof(double), &pF));
    CHK(ws_get(c, S_NR_ITEMS, (size_t)ni * sizeof(NrItem), &pI));
    CHK(ws_get(c, S_NR_ROWS, (size_t)ni * T * bins * sizeof(double), &pR));
    HIPCHK(c, hipMemcpyAsync(pI, items.data() + i0, ni * sizeof(NrItem), hipMemcpyHostToDevice,
                             c->stream));
    NrArgs a{};
    a.y = dy;
    a.items = static_cast<const NrItem*>(pI);
    a.n_items = ni;
    a.L = L;
    a.T = T;
    a.keep0 = kNrPadding;
    a.keep_len = keep;
    int t_hi = T - 1;
    nr_frame_range(items.data() + i0, ni, L, T, a.keep0, a.keep_len, &a.t_lo, &t_hi);
    a.t_n = t_hi - a.t_lo + 1;
    a.tables = c->nr_tables;
    a.thresh = nonstationary ? nullptr : c->nr_thresh;
    a.profile = nonstationary ? nullptr : dprofile;
    a.n_profiles = nonstationary ? 0 : (int)c->nr_profiles;
    a.prop_decrease = 1.0;
    a.S = static_cast<double2*>(pS);
    a.bits = static_cast<uint8_t*>(pB);
    a.fmax = static_cast<double*>(pM);
    a.gmax = pM ? static_cast<double*>(pM) + ni * T : nullptr;
    a.frames = static_cast<double*>(pF);
    a.rows = static_cast<double*>(pR);
    a.out = dout;
    double bytes = 0;
    for (int64_t i = 0; i < ni; ++i) bytes += 8.0 * items[i0 + i].out_len;   // f32 in + f32 out
    if (nonstationary) LAUNCH(c, MMLA_STAGE_NR, bytes, nr_ns_gate_launch(a, ns, c->stream));
    else LAUNCH(c, MMLA_STAGE_NR, bytes, nr_gate_launch(a, c->stream));
    // the item table / scratch of this launch must not be overwritten by the next one's upload
    if (i0 + cap < items.size()) HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return MMLA_OK;
}

extern "C" {

static int nr_reduce_common(mmla_ctx* c, const float* y, int64_t n_signals, int64_t stride, int64_t len,
                            const int32_t* profile, float* out, uint32_t flags, bool nonstationary = false) {
  if (n_signals < 0 || len < 0 || (n_signals > 0 && (!y || !out)) ||
      (n_signals > 1 && stride < len))
    return fail(c, MMLA_E_INVALID, "bad nr_reduce args");
  if (!nonstationary && !c->nr_ready) return fail(c, MMLA_E_INVALID, "mmla_nr_set_noise must be called first");
  const bool dev = flags & MMLA_DEVICE_PTR;
  // device-pointer profile indices cannot be seen here: the kernels clamp them into the bank
  if (profile && !dev)
    for (int64_t i = 0; i < n_signals; ++i)
      if (profile[i] < 0 || profile[i] >= c->nr_profiles)
        return fail(c, MMLA_E_INVALID, "profile[%lld] = %d outside the bank of %lld", (long long)i,
                    profile[i], (long long)c->nr_profiles);
  if (n_signals == 0 || len == 0) return MMLA_OK;
  HIPCHK(c, hipSetDevice(c->device));
  // signals: the caller's device pointer, or one host copy per call
  const float* dy;
  const int32_t* dprof;
  CHK(in_ptr(c, y, (n_signals - 1) * stride + len, dev, S_NR_Y, &dy));
  CHK(in_ptr(c, profile, (size_t)n_signals, dev, S_NR_PROF, &dprof));
  float* dout = out;
  if (!dev) {
    void* p = nullptr;
    CHK(ws_get(c, S_OUT0, (size_t)n_signals * len * sizeof(float), &p));
    dout = static_cast<float*>(p);
  }
  CHK(nr_reduce_dev(c, dy, n_signals, stride, len, dout, dprof, nonstationary));
  CHK(copy_back(c, out, 0, dout, (size_t)n_signals * len, dev));
  return finish(c, dev);
}

int mmla_nr_reduce(mmla_ctx* c, const float* y, int64_t n_signals, int64_t stride, int64_t len,
                   float* out, uint32_t flags) {
  if (!c) return MMLA_E_INVALID;
  return nr_reduce_common(c, y, n_signals, stride, len, nullptr, out, flags);
}

int mmla_nr_reduce_bank(mmla_ctx* c, const float* y, int64_t n_signals, int64_t stride, int64_t len,
                        const int32_t* profile, float* out, uint32_t flags) {
  if (!c) return MMLA_E_INVALID;
  return nr_reduce_common(c, y, n_signals, stride, len, profile, out, flags);
}

int mmla_nr_reduce_ns(mmla_ctx* c, const float* y, int64_t n_signals, int64_t stride, int64_t len,
                      float* out, uint32_t flags) {
  if (!c) return MMLA_E_INVALID;
  return nr_reduce_common(c, y, n_signals, stride, len, nullptr, out, flags, true);
}

// ---- silence removal: webrtcvad + vad_collector, soundfile PCM_16 ------------

int mmla_vad_reset(mmla_ctx* c, int64_t n_streams, int32_t mode) {
  if (!c) return MMLA_E_INVALID;
  if (n_streams < 1) return fail(c, MMLA_E_INVALID, "n_streams must be >= 1");
  VadState init;
  if (!vad_init_state(&init, mode)) return fail(c, MMLA_E_INVALID, "VAD mode must be 0..3, got %d", mode);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->vad_state) HIPCHK(c, hipFree(c->vad_state));
  c->vad_state = nullptr;
  c->vad_streams = 0;
  // twice the states: [n_streams, 2 n_streams) is the conditioned calls' snapshot (internal.h)
  if (hipMalloc(&c->vad_state, 2 * n_streams * sizeof(VadState)) != hipSuccess) {
    (void)hipGetLastError();
    return fail(c, MMLA_E_OOM, "VAD state for %lld streams", (long long)n_streams);
  }
  std::vector<VadState> h(n_streams, init);
  HIPCHK(c, hipMemcpy(c->vad_state, h.data(), n_streams * sizeof(VadState), hipMemcpyHostToDevice));
  c->vad_streams = n_streams;
  return MMLA_OK;
}

// shared body: speech == nullptr -> decisions from the context's VAD states, else the caller's
static int vad_run(mmla_ctx* c, const int16_t* pcm, int64_t n, int64_t stride, const int32_t* lens,
                   int32_t clip_len, int64_t items_per_stream, const uint8_t* speech_in,
                   uint8_t* speech_out, int32_t max_frames, int16_t* out, int32_t* out_lens,
                   uint32_t flags) {
  if (n < 0 || (n > 0 && (!pcm || !out || !out_lens)) || (!lens && clip_len < 0) ||
      (n > 1 && stride < (lens ? 1 : clip_len)) || (n > 0 && lens && stride < 1))
    return fail(c, MMLA_E_INVALID, "bad VAD args");
  if (n == 0) return MMLA_OK;
  // with lens the row width is the stride: an item longer than its row would read the next item
  // and its rewrite would run past the output; device-pointer lens are clamped in the
  // kernels instead
  if (lens && !(flags & MMLA_DEVICE_PTR))
    for (int64_t i = 0; i < n; ++i)
      if (lens[i] > stride)
        return fail(c, MMLA_E_INVALID, "lens[%lld] = %d exceeds the row width (stride %lld)",
                    (long long)i, lens[i], (long long)stride);
  const int64_t width = lens ? stride : std::max<int64_t>(clip_len, 1);
  if (max_frames <= 0) max_frames = std::max(1, vad_frames(width));
  if (max_frames > 4096) return fail(c, MMLA_E_INVALID, "more than 4096 frames (2 min) per item");
  HIPCHK(c, hipSetDevice(c->device));
  const bool dev = flags & MMLA_DEVICE_PTR;
  VadArgs a{};
  a.stride = n > 1 ? stride : width;
  a.clip_len = clip_len;
  a.n_items = n;
  a.items_per_stream = items_per_stream;
  a.max_frames = max_frames;
  a.state = c->vad_state;
  const size_t samples = (size_t)(n - 1) * a.stride + width;
  CHK(in_ptr(c, pcm, samples, dev, S_PCM, &a.pcm));
  CHK(in_ptr(c, lens, n, dev, S_LENS, &a.lens));
  void* ps = nullptr;
  const size_t sbytes = (size_t)n * max_frames;
  if (speech_in && dev) {
    a.speech = const_cast<uint8_t*>(speech_in);
  } else if (speech_out && dev) {
    a.speech = speech_out;
  } else {
    CHK(ws_get(c, S_VAD_SPEECH, sbytes, &ps));
    a.speech = static_cast<uint8_t*>(ps);
    if (speech_in) HIPCHK(c, hipMemcpyAsync(ps, speech_in, sbytes, hipMemcpyHostToDevice, c->stream));
  }
  CHK(out_ptr(c, out, 0, samples, dev, S_VAD_OUT, &a.out));
  CHK(out_ptr(c, out_lens, 0, n, dev, S_VAD_LENS, &a.out_lens));
  if (!speech_in) {
    if (!c->vad_state) return fail(c, MMLA_E_INVALID, "mmla_vad_reset must be called first");
    if (items_per_stream < 1 || n % items_per_stream || n / items_per_stream != c->vad_streams)
      return fail(c, MMLA_E_INVALID, "%lld items are not %lld streams x items_per_stream %lld",
                  (long long)n, (long long)c->vad_streams, (long long)items_per_stream);
    // the rewrite keeps a frame's bytes or drops it: outputs are never longer than inputs
    LAUNCH(c, MMLA_STAGE_GLUE, (double)n * width, vad_speech_launch(a, vad_use_wave(c, c->vad_streams), c->stream));
  }
  LAUNCH(c, MMLA_STAGE_GLUE, (double)n * width, vad_collect_launch(a, c->stream));
  CHK(copy_back(c, out, 0, a.out, samples, dev));
  CHK(copy_back(c, out_lens, 0, a.out_lens, n, dev));
  if (speech_out && !dev)
    HIPCHK(c, hipMemcpyAsync(speech_out, a.speech, sbytes, hipMemcpyDeviceToHost, c->stream));
  return finish(c, dev);
}

int mmla_vad_remove_silence(mmla_ctx* c, const int16_t* pcm, int64_t n_items, int64_t stride,
                            const int32_t* lens, int32_t clip_len, int64_t items_per_stream,
                            int16_t* out, int32_t* out_lens, uint8_t* speech, int32_t max_frames,
                            uint32_t flags) {
  if (!c) return MMLA_E_INVALID;
  return vad_run(c, pcm, n_items, stride, lens, clip_len, items_per_stream, nullptr, speech,
                 max_frames, out, out_lens, flags);
}

int mmla_debug_vad_path(mmla_ctx* c, int64_t n_streams, int32_t* wave) {
  if (!c || !wave) return MMLA_E_INVALID;
  if (n_streams < 1) return fail(c, MMLA_E_INVALID, "n_streams must be >= 1");
  *wave = vad_use_wave(c, n_streams) ? 1 : 0;
  return MMLA_OK;
}

int mmla_vad_collect(mmla_ctx* c, const int16_t* pcm, int64_t n_items, int64_t stride,
                     const int32_t* lens, int32_t clip_len, const uint8_t* speech, int32_t max_frames,
                     int16_t* out, int32_t* out_lens, uint32_t flags) {
  if (!c) return MMLA_E_INVALID;
  if (n_items > 0 && !speech) return fail(c, MMLA_E_INVALID, "speech flags required");
  return vad_run(c, pcm, n_items, stride, lens, clip_len, 1, speech, nullptr, max_frames, out,
                 out_lens, flags);
}

int mmla_pcm16(mmla_ctx* c, const float* y, int64_t n, int16_t* out, uint32_t flags) {
  if (!c) return MMLA_E_INVALID;
  if (n < 0 || (n > 0 && (!y || !out))) return fail(c, MMLA_E_INVALID, "bad pcm16 args");
  if (n == 0) return MMLA_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const bool dev = flags & MMLA_DEVICE_PTR;
  const float* dy;
  CHK(in_ptr(c, y, n, dev, S_IN, &dy));
  int16_t* d;
  CHK(out_ptr(c, out, 0, n, dev, S_VAD_OUT, &d));
  LAUNCH(c, MMLA_STAGE_GLUE, (double)n * 6, pcm16_launch(dy, n, d, c->stream));
  CHK(copy_back(c, out, 0, d, n, dev));
  return finish(c, dev);
}

// ---- rate conversion of the offline pre-conditioning (resample.hip) ------------------------------

int mmla_ratecv(mmla_ctx* c, const int16_t* pcm, int64_t n_frames, int32_t nch, int32_t inrate,
                int32_t outrate, int16_t* out, int64_t out_frames, uint32_t flags) {
  if (!c) return MMLA_E_INVALID;
  if (n_frames < 0 || nch < 1 || nch > 64 || inrate < 1 || outrate < 1 ||
      (n_frames > 0 && (!pcm || !out)))
    return fail(c, MMLA_E_INVALID, "bad ratecv args");
  const int g = std::gcd(inrate, outrate);
  const int64_t ir = inrate / g, orr = outrate / g;
  const int64_t want = n_frames > 0 ? (n_frames - 1) * orr / ir + 1 : 0;
  if (out_frames != want)
    return fail(c, MMLA_E_INVALID, "ratecv of %lld frames %d -> %d Hz gives %lld frames, not %lld",
                (long long)n_frames, inrate, outrate, (long long)want, (long long)out_frames);
  if (n_frames == 0) return MMLA_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const bool dev = flags & MMLA_DEVICE_PTR;
  const int16_t* din;
  CHK(in_ptr(c, pcm, (size_t)n_frames * nch, dev, S_PCM, &din));
  int16_t* d;
  CHK(out_ptr(c, out, 0, (size_t)want * nch, dev, S_VAD_OUT, &d));
  LAUNCH(c, MMLA_STAGE_GLUE, 2.0 * nch * (double)(n_frames + want),
         ratecv_launch(din, n_frames, nch, (int)ir, (int)orr, d, want, c->stream));
  CHK(copy_back(c, out, 0, d, (size_t)want * nch, dev));
  return finish(c, dev);
}

int mmla_resample_sinc(mmla_ctx* c, const float* x, int64_t n, int32_t sr_orig, int32_t sr_new,
                       const double* half_window, int64_t window_len, int32_t num_table, float* y,
                       int64_t n_out, uint32_t flags) {
  if (!c) return MMLA_E_INVALID;
  if (n < 0 || sr_orig < 1 || sr_new < 1 || window_len < 2 || num_table < 1 || !half_window ||
      (n > 0 && (!x || !y)))
    return fail(c, MMLA_E_INVALID, "bad resample args");
  const double ratio = (double)sr_new / (double)sr_orig;
  const int64_t want = (int64_t)((double)n * ratio);      // resampy: int(n * sample_ratio)
  if (n_out != want)
    return fail(c, MMLA_E_INVALID, "resampling %lld samples %d -> %d Hz gives %lld, not %lld",
                (long long)n, sr_orig, sr_new, (long long)want, (long long)n_out);
  if (n_out == 0) return MMLA_OK;
  const double scale = std::min(1.0, ratio);
  const int index_step = (int)(scale * num_table);
  if (index_step < 1) return fail(c, MMLA_E_INVALID, "ratio %g too small for the filter table", ratio);
  HIPCHK(c, hipSetDevice(c->device));
  const bool dev = flags & MMLA_DEVICE_PTR;
  // the filter as resampy prepares it: scaled by the ratio when downsampling, then its forward
  // difference (last entry 0), interleaved (win, delta) for one 16-B load per tap
  std::vector<double> wd(2 * window_len);
  for (int64_t i = 0; i < window_len; ++i) wd[2 * i] = ratio < 1 ? half_window[i] * ratio : half_window[i];
  for (int64_t i = 0; i < window_len; ++i)
    wd[2 * i + 1] = i + 1 < window_len ? wd[2 * i + 2] - wd[2 * i] : 0.0;
  // the time register of the sequential loop: repeated float64 addition of 1 / ratio
  std::vector<double> tr(n_out);
  const double inc = 1.0 / ratio;
  double t_reg = 0.0;
  for (int64_t t = 0; t < n_out; ++t) {
    tr[t] = t_reg;
    t_reg += inc;
  }
  void *ptr = nullptr, *pw = nullptr;
  CHK(ws_get(c, S_RS_TR, (size_t)n_out * sizeof(double), &ptr));
  CHK(ws_get(c, S_RS_WIN, wd.size() * sizeof(double), &pw));
  HIPCHK(c, hipMemcpyAsync(ptr, tr.data(), (size_t)n_out * sizeof(double), hipMemcpyHostToDevice,
                           c->stream));
  HIPCHK(c, hipMemcpyAsync(pw, wd.data(), wd.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  SincResampleArgs a{};
  CHK(in_ptr(c, x, (size_t)n, dev, S_IN, &a.x));
  a.n_orig = n;
  a.tr = static_cast<const double*>(ptr);
  a.win = static_cast<const double*>(pw);
  a.nwin = window_len;
  a.num_table = num_table;
  a.index_step = index_step;
  a.scale = scale;
  a.n_out = n_out;
  CHK(out_ptr(c, y, 0, (size_t)n_out, dev, S_OUT0, &a.y));
  LAUNCH(c, MMLA_STAGE_GLUE, 4.0 * (double)(n + n_out), sinc_resample_launch(a, c->stream));
  CHK(copy_back(c, y, 0, a.y, (size_t)n_out, dev));
  // the host vectors above are read by the async uploads: wait before they go out of scope
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return finish(c, dev);
}

// ---- speaker registration: the sigmoid-head trainer (si_train.hip) --------------------------------

int mmla_si_head_fit(mmla_ctx* c, const float* emb, const int32_t* labels, int64_t n_train,
                     const float* val_emb, const int32_t* val_labels, int64_t n_val,
                     int32_t n_classes, int32_t n_restarts, int32_t epochs, int32_t batch, float lr,
                     const float* w0, const float* b0, const int32_t* perm, float* w, float* b,
                     float* history, uint32_t flags) {
  if (!c) return MMLA_E_INVALID;
  if (n_classes < 1 || n_classes > MMLA_SI_TRAIN_MAX_CLASSES)
    return fail(c, MMLA_E_INVALID, "n_classes %d outside [1, %d]", n_classes, MMLA_SI_TRAIN_MAX_CLASSES);
  if (batch < 1) return fail(c, MMLA_E_INVALID, "batch %d < 1", batch);
  if (n_train < 1) return fail(c, MMLA_E_INVALID, "n_train %lld < 1", (long long)n_train);
  if (n_val < 0 || n_restarts < 1 || epochs < 0 || n_train > (1 << 24) || n_val > (1 << 24))
    return fail(c, MMLA_E_INVALID, "bad head_fit sizes (n_val %lld, n_restarts %d, epochs %d)",
                (long long)n_val, n_restarts, epochs);
  if (!emb || !labels || !w0 || !b0 || !w || !b || (epochs > 0 && !perm) ||
      (n_val > 0 && (!val_emb || !val_labels)))
    return fail(c, MMLA_E_INVALID, "head_fit: null pointer");
  Stager st{c, (flags & MMLA_DEVICE_PTR) != 0};
  const int K = n_classes, R = n_restarts;
  if (!st.dev) {   // device-pointer calls: the caller guarantees labels and permutations
    CHK(check_labels(c, "labels", labels, n_train, K));
    CHK(check_labels(c, "val_labels", val_labels, n_val, K));
    const int64_t row = bad_perm_row(perm, (int64_t)R * epochs, n_train);
    if (row >= 0)
      return fail(c, MMLA_E_INVALID, "perm row %lld (restart %lld, epoch %lld) is not a permutation of 0..%lld",
                  (long long)row, (long long)(row / epochs), (long long)(row % epochs), (long long)(n_train - 1));
  }
  HIPCHK(c, hipSetDevice(c->device));
  SiTrainArgs a{};
  a.n_train = (int)n_train;
  a.n_val = (int)n_val;
  a.k = K;
  a.epochs = epochs;
  a.batch = batch;
  a.lr = lr;
  const size_t nw = (size_t)R * MMLA_SI_EMBED * K, nb = (size_t)R * K, nh = (size_t)R * epochs * 4;
  // host pointers: every operand in one workspace slot
  CHK(carve_slot(c, S_TRAIN, [&](Carver& cv) -> int {
    CHK(st.in(cv, emb, (size_t)n_train * MMLA_SI_EMBED, &a.emb));
    CHK(st.in(cv, labels, (size_t)n_train, &a.labels));
    CHK(st.in(cv, val_emb, (size_t)n_val * MMLA_SI_EMBED, &a.val_emb));
    CHK(st.in(cv, val_labels, (size_t)n_val, &a.val_labels));
    CHK(st.in(cv, w0, nw, &a.w0));
    CHK(st.in(cv, b0, nb, &a.b0));
    CHK(st.in(cv, perm, (size_t)R * epochs * n_train, &a.perm));
    a.w = st.out(cv, w, nw);
    a.b = st.out(cv, b, nb);
    a.history = st.out(cv, history, nh);
    return MMLA_OK;
  }));
  // forward + gradient on the training set, forward on the validation set, per epoch and restart
  const double flops = (double)R * epochs * 2.0 * MMLA_SI_EMBED * K * (2.0 * n_train + n_val);
  LAUNCH(c, MMLA_STAGE_HEAD, flops, si_train_launch(a, R, c->stream));
  CHK(st.back(w, a.w, nw));
  CHK(st.back(b, a.b, nb));
  CHK(st.back(history, a.history, nh));
  return finish(c, st.dev);
}

}  // extern "C"
