// Batched mean structural similarity of uint8 image pairs (see ssim.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int SSIM_WIN = 7;   // scikit-image's default window for uint8 input

// a, b [n,h,w,c] u8 -> out [n] f32: structural_similarity(a[i], b[i], multichannel=True) with the
// defaults (uniform 7 x 7 window, K1 0.01, K2 0.03, data_range 255, sample covariance, the map cropped
// by 3 pixels).  h, w >= 7 and c in {1, 3, 4} (the caller checks); one workgroup per pair, so a pair's
// result does not depend on n or on its position.
hipError_t ssim_u8_launch(const uint8_t* a, const uint8_t* b, int64_t n, int h, int w, int c,
                          float* out, hipStream_t s);
// out[i] = v, i < n (the similarity of a clip that was not denoised: 1)
hipError_t fill_f32_launch(float* out, int64_t n, float v, hipStream_t s);
