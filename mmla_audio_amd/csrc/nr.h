// Spectral-gate noise reduction kernel interface, stationary and non-stationary (see nr.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"

constexpr int NR_NFFT = 1024;   // noisereduce 2.0 defaults: n_fft 1024, win_length = n_fft,
constexpr int NR_HOP = 256;     // hop = win_length // 4
constexpr int NR_NGF = 33;      // smoothing filter at 16 kHz: 2 * 16 + 1 bins (500 Hz) ...
constexpr int NR_NGT = 7;       // ... x 2 * 3 + 1 frames (50 ms)

struct NrTables {
  double win[NR_NFFT];          // periodic Hann
  cd w512[512];                 // W512^m
  double w1024[NR_NFFT / 2 + 1][2];   // W1024^k
  double gf[NR_NGF];            // smoothing filter = gf (x) gt (separable, each normalised)
  double gt[NR_NGT];
  int ngf, ngt;                 // taps the ramps actually have (must equal NR_NGF / NR_NGT)
};

// one buffer of L samples: buffer index u <-> signal index i1 + u (zeros outside [0, n));
// output = buffer [keep0, keep0 + out_len) -> out[out_off ..]; prof: the item's entry of
// NrArgs::profile (its signal's index), whose value selects the noise profile
struct NrItem {
  int64_t sig_off, n, i1, out_off, out_len, prof;
};

struct NrArgs {
  const float* y;               // signals (float32, as librosa.load returns)
  const NrItem* items;
  int64_t n_items;
  int64_t L;                    // buffer length: chunk + 2 * padding
  int T;                        // STFT frames per buffer: 1 + L / 256
  int t_lo, t_n;                // frames launched per item: every frame that is not an all-zero
                                // window or whose mask the gate needs (host: nr_frame_range)
  int64_t keep0, keep_len;      // kept interior of every buffer
  const NrTables* tables;
  const float* thresh;          // [n_profiles][513] noise thresholds (dB, float32)
  const int32_t* profile;       // nullable (profile 0): profile[item.prof] selects the item's
  int n_profiles;               //   threshold row, clamped into [0, n_profiles) by the kernels
  double prop_decrease;
  double2* S;                   // scratch [n_items][T][513] complex128
  uint8_t* bits;                // scratch [n_items][T][513] dB > thresh
  double* fmax;                 // scratch [n_items][T] frame max dB
  double* gmax;                 // scratch [n_items] max over the item's frames
  double* rows;                 // scratch [n_items][T][513] frequency-smoothed mask rows
  double* frames;               // scratch [n_items][T][1024] gated windowed frames
  float* out;
};

void nr_build_tables(NrTables* t, int sr);
// A bank of noise profiles in one launch sequence: profile p = noise + p * stride, its first
// m_p = clamp(lens[p], 2, m) samples (lens nullable: m), Tn_p = 1 + m_p / 256 frames.  With
// Tmax = 1 + m / 256: db_scratch [n_profiles][Tmax][513], fmax_scratch [n_profiles][Tmax]
// -> thresh [n_profiles][513].  Frames past a profile's Tn_p do nothing.
struct NrNoiseArgs {
  const float* noise;
  int64_t stride;
  const int32_t* lens;
  int64_t m;
  int n_profiles;
  const NrTables* tables;
  float* db;
  float* fmaxv;
  float n_std;
  float* thresh;
};
hipError_t nr_noise_launch(const NrNoiseArgs& a, hipStream_t s);
hipError_t nr_gate_launch(const NrArgs& a, hipStream_t s);
// The non-stationary gate (noisereduce's stationary=False; nr.hip) on the same items and
// scratch: thresh / profile / bits / fmax / gmax are not read (nullable).  The noise floor is the
// magnitude spectrogram smoothed along time per bin by filtfilt([b], [1, b - 1]); one_minus_b is
// -(b - 1) as scipy forms it; mask = 1 / (1 + exp(-((|S| - floor) / floor - shift) * slope)).
struct NrNsParams {
  double b, one_minus_b, shift, slope;
};
// b of a time constant in seconds at sample rate sr (noisereduce get_time_smoothed_representation)
double nr_ns_coefficient(double time_constant_s, int sr);
hipError_t nr_ns_gate_launch(const NrArgs& a, const NrNsParams& p, hipStream_t s);
// [t_lo, t_hi] covering, for every item, the frames whose window overlaps its signal and the frames
// within the time-smoothing halo of the kept interior
void nr_frame_range(const NrItem* items, int64_t n_items, int64_t L, int T, int64_t keep0,
                    int64_t keep_len, int* t_lo, int* t_hi);
