// The pyramid blur of OverlapDetector.augment_images (overlap_detector.py:198-220): extra copy number i of
// a feature image is cv.pyrDown then cv.pyrUp, i + 1 times, cropped once at the end with src[:, :-1].  See
// od_aug.hip; include/mmla.h states the arithmetic (OpenCV's published uint8 pyramid code; OpenCV is not
// available here: parity with OpenCV unpinned).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int ODA_MIN_H = 8, ODA_MAX_H = 128;    // h even
constexpr int ODA_MIN_W = 9, ODA_MAX_W = 151;    // w odd
constexpr int ODA_MAX_LEVELS = 8;                // = MMLA_OD_AUG_MAX_LEVELS

inline bool oda_size_ok(int h, int w) {
  return h >= ODA_MIN_H && h <= ODA_MAX_H && h % 2 == 0 && w >= ODA_MIN_W && w <= ODA_MAX_W && w % 2 == 1;
}

// out[k] [h, w, 3] = img[clamp(src[k], 0, n - 1)] blurred clamp(levels[k], 0, 8) times, k < m.  Device
// pointers; enqueues on `stream`, does not synchronise.  hipErrorInvalidValue unless oda_size_ok, n >= 1 and
// 0 <= m <= 2^24
hipError_t oda_augment(const uint8_t* img, int64_t n, int h, int w, const int32_t* src, const int32_t* levels,
                       int64_t m, uint8_t* out, hipStream_t stream);
