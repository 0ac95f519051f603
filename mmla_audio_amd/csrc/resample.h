// Rate conversion of the offline pre-conditioning (resample.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

// audioop.ratecv(data, 2, nch, inrate, outrate, None) with inrate / outrate already divided by
// their gcd; in [n_frames][nch] int16, out [n_out][nch] int16
hipError_t ratecv_launch(const int16_t* in, int64_t n_frames, int nch, int inrate, int outrate,
                         int16_t* out, int64_t n_out, hipStream_t s);

// Streaming conversion of a room's interleaved capture to 16 kHz mono (mmla_capture_convert): stream s
// owns clips [s * items_per_stream, (s + 1) * items_per_stream), clip c = pcm + c * clip_stride holds
// frames[c] (nullable: clip_frames; clamped into [0, clip_frames]) frames of `channels` int16; the mono
// signal is channel `channel` (>= 0) or floor((l + r) / 2) (channel < 0, two channels).  ir / orr: the
// capture rate and 16000 divided by their gcd.  All pointers are device pointers.
//   capture_phase_launch   one thread per stream: item[c] = (d0, prev) on entry to clip c, out_lens[c],
//                          and the stream's state after its last clip.  state_in [n_streams][2] =
//                          (d, prev) (null: fresh states), state_out likewise (null: not kept); a
//                          thread reads its own state before it writes, so the two may be one array
//   capture_sample_launch  one thread per output sample: out [n_clips][out_stride] int16, zeros from
//                          out_lens[c] to out_clip_len
struct CaptureArgs {
  const int16_t* pcm;
  int64_t clip_stride;
  const int32_t* frames;
  int32_t clip_frames;
  int32_t channels, channel;
  int32_t ir, orr;
  int64_t n_clips, items_per_stream;
  const int32_t* state_in;
  int32_t* state_out;
  int32_t* item;   // [n_clips][2]
  int16_t* out;
  int64_t out_stride;
  int32_t out_clip_len;
  int32_t* out_lens;
};
hipError_t capture_phase_launch(const CaptureArgs& a, hipStream_t s);
hipError_t capture_sample_launch(const CaptureArgs& a, hipStream_t s);

// resampy.resample_f (one channel): y[t] for t < n_out from x[n_orig], the float64 time register
// tr[t] and the interpolated filter half-window as (win[i], win[i + 1] - win[i]) pairs, nwin of them
struct SincResampleArgs {
  const float* x;
  int64_t n_orig;
  const double* tr;
  const double* win;   // [nwin][2]
  int64_t nwin;
  int num_table;
  int index_step;
  double scale;
  float* y;
  int64_t n_out;
};
hipError_t sinc_resample_launch(const SincResampleArgs& a, hipStream_t s);
