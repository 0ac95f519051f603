// Silence removal of the reference's save_wave_file(silence_remove=True): webrtcvad.Vad(mode)
// decisions on 30 ms frames + vad_collector + the rewrite of the voiced frames.  See vad.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// One webrtcvad.Vad instance (WebRTC VadInstT, the 16 kHz path), kept in device memory.
struct VadState {
  int32_t ds[2];                    // 16 -> 8 kHz all-pass downsampler
  int32_t frame_counter;
  int16_t over_hang, num_of_speech;
  int16_t noise_means[12], speech_means[12], noise_stds[12], speech_stds[12];
  int16_t low_value[96], age[96];   // FindMinimum: 16 smallest features per channel and their age
  int16_t mean_value[6];
  int16_t upper[5], lower[5];       // splitting-filter all-pass states
  int16_t hp[4];                    // 80 Hz high-pass state
  int16_t oh1, oh2, individual, total;   // mode thresholds for 30 ms frames
};

struct VadArgs {
  const int16_t* pcm;      // item i at pcm + i * stride
  int64_t stride;
  const int32_t* lens;     // nullable: every item has clip_len samples
  int32_t clip_len;
  int64_t n_items;
  int64_t items_per_stream; // stream s owns items [s * ips, (s + 1) * ips), processed in order
  VadState* state;          // [n_items / ips]
  uint8_t* speech;          // [n_items][max_frames] per-frame decisions (written by the VAD kernel,
                            //   read by the collector)
  int32_t max_frames;
  int16_t* out;             // item i's voiced frames at out + i * stride
  int32_t* out_lens;        // [n_items]
};

// Host: a fresh webrtcvad.Vad(mode) (WebRtcVad_Init + set_mode); false for a mode outside 0..3.
bool vad_init_state(VadState* s, int mode);
// Frames of an item of `len` samples (frame_generator: k * 480 + 480 < len).
__host__ __device__ inline int vad_frames(int64_t len) { return len > 480 ? (int)((len - 1) / 480) : 0; }
// Stream counts up to this run on vad_speech_wave_kernel (one stream per wave), larger ones on
// vad_speech_kernel (one thread per stream); measured, DESIGN.md 4.10.
constexpr int64_t kVadWaveMaxStreams = 4096;
inline bool vad_wave_streams(int64_t n_streams) { return n_streams <= kVadWaveMaxStreams; }
// Per-frame decisions of every item, stream by stream: one stream per wave (wave) or per thread; the
// same decisions and states bit for bit.
hipError_t vad_speech_launch(const VadArgs& a, bool wave, hipStream_t s);
// vad_collector + the rewrite from `speech` (one wave per item).
hipError_t vad_collect_launch(const VadArgs& a, hipStream_t s);
// soundfile's PCM_16 write of float audio (libsndfile f2s: (short) lrintf(x * 0x7FFF)).
hipError_t pcm16_launch(const float* y, int64_t n, int16_t* out, hipStream_t s);
// The PCM_16 round trip of the denoise-and-compare gate (mmla_od_pipeline_gated), n clips of `len`
// samples, zeros from each clip's valid length (lens[i] clamped to [0, len]; null: len) on:
// pcm_f32: the read (x / 32768) of int16 clips at `stride` into y [n][len];
// requant: pcm16's write of y [n][len], as int16 into yq [n][len] or, with yq null, read back into yf.
hipError_t pcm_f32_launch(const int16_t* pcm, int64_t stride, const int32_t* lens, int len, int64_t n,
                          float* y, hipStream_t s);
hipError_t requant_launch(const float* y, const int32_t* lens, int len, int64_t n, float* yf,
                          int16_t* yq, hipStream_t s);
// mmla_condition (n clips of `len` samples, lens as above):
// pcm_i16: the clips at `stride` copied into q [n][len], zeros from each clip's valid length on;
// cond_finish: kept[c] = vad_lens[c] (silence removed: q's samples from there on are zeroed) or,
// with vad_lens null, the clip's valid length.
hipError_t pcm_i16_launch(const int16_t* pcm, int64_t stride, const int32_t* lens, int len, int64_t n,
                          int16_t* q, hipStream_t s);
hipError_t cond_finish_launch(int16_t* q, const int32_t* vad_lens, const int32_t* lens, int len,
                              int64_t n, int32_t* kept, hipStream_t s);
