// Rate conversion of the offline pre-conditioning chains, and of a live room's
// capture (capture_phase_kernel / capture_sample_kernel below: 44.1 / 48 kHz interleaved -> 16 kHz mono
// with audioop's state carried per stream).
//
// Replaces:
//   pydub AudioSegment.set_frame_rate(16000) = audioop.ratecv(data, 2, channels, rate, 16000, None)
//       OverlapDetection/scripts/overlap_detection_post_processing.py:120-121 (48 kHz stereo zoom
//       exports), SpeakerIdentification/scripts/speaker_identification_post_processing.py:159-160
//       (the 22.05 kHz PCM_16 file that librosa.load wrote)
//   librosa.load(path) at its default sr = 22050 = resampy.resample(filter='kaiser_best')
//       speaker_identification_post_processing.py:142
//
// ratecv_kernel: CPython's audioop.ratecv loop (weightA 1, weightB 0, fresh state) keeps a phase
// counter d = -outrate; every input frame adds outrate, every output frame subtracts inrate.  So
// output frame j is written right after input frame k = ceil(j inrate / outrate) was read, at
// d = k outrate - j inrate, and is a pure function of (j, frames k - 1 and k): one thread per output
// frame, bit-identical to the sequential C loop (the double products are exact; the one division is
// IEEE-rounded on both sides; (int) truncates; >> 16 floors as the C shift does).
//
// sinc_resample_kernel: resampy 0.2 resample_f for one channel, one thread per output sample: left
// then right wing of the linearly interpolated filter, each tap's float64 product added to a float32
// accumulator (numba stores y[t] as float32 after every tap).  The float64 time register of the
// sequential loop (repeated addition of 1 / ratio) comes from the host.  fp contraction is off so
// every multiply and add rounds as numpy / numba do.
#include "resample.h"

namespace {

__global__ void ratecv_kernel(const int16_t* __restrict__ in, int64_t n_frames, int nch, int ir,
                              int orr, int16_t* __restrict__ out, int64_t n_out) {
#pragma clang fp contract(off)
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_out) return;
  const int64_t k = (j * ir + orr - 1) / orr;       // ceil(j ir / or) <= n_frames - 1
  const int64_t d = k * orr - j * ir;               // [0, or)
  if (k >= n_frames) return;                        // (host sizes n_out so this never happens)
  for (int ch = 0; ch < nch; ++ch) {
    const int prev = k > 0 ? ((int)in[(k - 1) * nch + ch]) * 65536 : 0;   // GETSAMPLE32: x << 16
    const int cur = ((int)in[k * nch + ch]) * 65536;
    const double v = ((double)prev * (double)d + (double)cur * (double)(orr - d)) / (double)orr;
    const int o = (int)v;                                                   // C cast: truncation
    out[j * nch + ch] = (int16_t)(o >> 16);                                 // SETSAMPLE32
  }
}

__global__ void sinc_resample_kernel(SincResampleArgs a) {
#pragma clang fp contract(off)
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.n_out) return;
  const double2* __restrict__ wd = reinterpret_cast<const double2*>(a.win);   // (win, dwin) pairs
  const double tr = a.tr[t];
  // n <= n_orig - 1 for every rate pair (the last time is ~ n_orig - 1 / ratio); clamped anyway so a
  // time register that drifted past the input (ratios far beyond audio's) cannot read past x
  int64_t n = (int64_t)tr;
  n = n < a.n_orig ? n : a.n_orig - 1;
  double frac = a.scale * (tr - (double)n);
  double index_frac = frac * (double)a.num_table;
  int64_t offset = (int64_t)index_frac;
  double eta = index_frac - (double)offset;
  float y = 0.0f;
  const int64_t i_max = min(n + 1, (a.nwin - offset) / a.index_step);
  for (int64_t i = 0; i < i_max; ++i) {
    const double2 w = wd[offset + i * a.index_step];
    const double weight = w.x + eta * w.y;
    y = (float)((double)y + weight * (double)a.x[n - i]);
  }
  frac = a.scale - frac;
  index_frac = frac * (double)a.num_table;
  offset = (int64_t)index_frac;
  eta = index_frac - (double)offset;
  const int64_t k_max = min(a.n_orig - n - 1, (a.nwin - offset) / a.index_step);
  for (int64_t k = 0; k < k_max; ++k) {
    const double2 w = wd[offset + k * a.index_step];
    const double weight = w.x + eta * w.y;
    y = (float)((double)y + weight * (double)a.x[n + k + 1]);
  }
  a.y[t] = y;
}

// ---- streaming conversion of a room's capture to 16 kHz mono (mmla_capture_convert) ---------------
//
// audioop.ratecv(fragment, 2, 1, rate, 16000, state) per stream, the state (d, prev) carried from
// fragment to fragment, on the mono signal picked or averaged out of the interleaved capture.  The
// sequential loop adds `or` to d per input frame and subtracts `ir` per output frame, so for a fragment
// of n frames entered with (d0, prev):
//   m = floor((n or + d0) / ir) + 1 outputs (0 when n or + d0 < 0);
//   output j is written right after input frame k = ceil((j ir - d0) / or) - 1, at phase
//   d = d0 + (k + 1) or - j ir in [0, or), from frames k - 1 (or prev, for k = 0) and k;
//   the state left is (d0 + n or - m ir, x[n - 1]).
// capture_phase_kernel walks each stream's fragments with that recurrence (one thread per stream: a
// handful of integer operations per fragment); capture_sample_kernel then computes every output of
// every fragment independently, ratecv_kernel's expression bit for bit.

// mono frame k of an interleaved clip: channel `sel`, or audioop.tomono(data, 2, 0.5, 0.5) (sel < 0,
// two channels): floor(0.5 l + 0.5 r) in double, the sum exact
__device__ __forceinline__ int capture_mono(const int16_t* __restrict__ clip, int64_t k, int nch,
                                            int sel) {
  if (sel >= 0) return (int)clip[k * nch + sel];
  const double v = 0.5 * (double)clip[2 * k] + 0.5 * (double)clip[2 * k + 1];
  return (int)floor(v);
}

__device__ __forceinline__ int capture_frames(const CaptureArgs& a, int64_t c) {
  if (!a.frames) return a.clip_frames;
  const int n = a.frames[c];
  return n < 0 ? 0 : (n > a.clip_frames ? a.clip_frames : n);
}

__global__ void capture_phase_kernel(CaptureArgs a, int64_t n_streams) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_streams) return;
  int64_t d = -(int64_t)a.orr;   // a fresh audioop state
  int prev = 0;
  if (a.state_in) {
    d = a.state_in[2 * s];
    prev = a.state_in[2 * s + 1];
  }
  for (int64_t i = 0; i < a.items_per_stream; ++i) {
    const int64_t c = s * a.items_per_stream + i;
    const int n = capture_frames(a, c);
    a.item[2 * c] = (int32_t)d;
    a.item[2 * c + 1] = prev;
    const int64_t t = (int64_t)n * a.orr + d;
    const int64_t m = t >= 0 ? t / a.ir + 1 : 0;
    a.out_lens[c] = (int32_t)m;
    d = t - m * a.ir;   // [-max(ir, or), 0)
    if (n > 0) prev = capture_mono(a.pcm + c * a.clip_stride, n - 1, a.channels, a.channel);
  }
  if (a.state_out) {
    a.state_out[2 * s] = (int32_t)d;
    a.state_out[2 * s + 1] = prev;
  }
}

// grid: blocks_per_clip blocks of 256 outputs per clip, clip-major.  Neighbouring threads store
// neighbouring int16 and read frames ir / or apart (48 kHz stereo: 12 bytes), a few cache lines per wave
__global__ void capture_sample_kernel(CaptureArgs a, int blocks_per_clip) {
#pragma clang fp contract(off)
  const int64_t c = blockIdx.x / blocks_per_clip;
  const int64_t j = (int64_t)(blockIdx.x % blocks_per_clip) * blockDim.x + threadIdx.x;
  if (c >= a.n_clips || j >= a.out_clip_len) return;
  int16_t* __restrict__ out = a.out + c * a.out_stride;
  if (j >= a.out_lens[c]) {   // the zero tail up to the longest a fragment can become
    out[j] = 0;
    return;
  }
  const int64_t d0 = a.item[2 * c];
  const int64_t k = (j * a.ir - d0 + a.orr - 1) / a.orr - 1;   // 0 <= k <= n - 1 (j ir - d0 >= 1)
  const int64_t d = d0 + (k + 1) * a.orr - j * a.ir;           // [0, or)
  if (k < 0 || k >= capture_frames(a, c)) return;              // (out_lens makes this impossible)
  const int16_t* __restrict__ clip = a.pcm + c * a.clip_stride;
  const int pm = k > 0 ? capture_mono(clip, k - 1, a.channels, a.channel) : a.item[2 * c + 1];
  const int prev = pm * 65536;                                  // GETSAMPLE32: x << 16
  const int cur = capture_mono(clip, k, a.channels, a.channel) * 65536;
  const double v = ((double)prev * (double)d + (double)cur * (double)(a.orr - d)) / (double)a.orr;
  const int o = (int)v;                                         // C cast: truncation
  out[j] = (int16_t)(o >> 16);                                  // SETSAMPLE32
}

}  // namespace

// the geometry both kernels index by: every read stays inside a clip's clip_frames * channels
// samples, every store inside out_clip_len <= out_stride
static bool capture_args_ok(const CaptureArgs& a) {
  return a.items_per_stream >= 1 && a.n_clips % a.items_per_stream == 0 && a.ir >= 1 && a.orr >= 1 &&
         a.channels >= 1 && a.channel < a.channels && (a.channel >= 0 || a.channels == 2) &&
         a.clip_frames >= 1 && a.out_clip_len >= 1 && a.out_stride >= a.out_clip_len &&
         a.clip_stride >= (int64_t)a.clip_frames * a.channels && a.pcm && a.item && a.out && a.out_lens &&
         a.n_clips * (int64_t)((a.out_clip_len + 255) / 256) <= 0x7fffffffLL;
}

hipError_t capture_phase_launch(const CaptureArgs& a, hipStream_t s) {
  if (a.n_clips <= 0) return hipSuccess;
  if (!capture_args_ok(a)) return hipErrorInvalidValue;
  const int64_t n_streams = a.n_clips / a.items_per_stream;
  hipLaunchKernelGGL(capture_phase_kernel, dim3((unsigned)((n_streams + 63) / 64)), dim3(64), 0, s, a,
                     n_streams);
  return hipGetLastError();
}

hipError_t capture_sample_launch(const CaptureArgs& a, hipStream_t s) {
  if (a.n_clips <= 0) return hipSuccess;
  if (!capture_args_ok(a)) return hipErrorInvalidValue;
  const int bpc = (a.out_clip_len + 255) / 256;
  hipLaunchKernelGGL(capture_sample_kernel, dim3((unsigned)(a.n_clips * bpc)), dim3(256), 0, s, a, bpc);
  return hipGetLastError();
}

hipError_t ratecv_launch(const int16_t* in, int64_t n_frames, int nch, int inrate, int outrate,
                         int16_t* out, int64_t n_out, hipStream_t s) {
  if (n_out <= 0) return hipSuccess;
  if (nch < 1 || inrate < 1 || outrate < 1 || n_frames < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ratecv_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, s, in,
                     n_frames, nch, inrate, outrate, out, n_out);
  return hipGetLastError();
}

hipError_t sinc_resample_launch(const SincResampleArgs& a, hipStream_t s) {
  if (a.n_out <= 0) return hipSuccess;
  if (a.index_step < 1 || a.nwin < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sinc_resample_kernel, dim3((unsigned)((a.n_out + 255) / 256)), dim3(256), 0, s,
                     a);
  return hipGetLastError();
}
