// The pyramid blur of OverlapDetector.augment_images (overlap_detector.py:198-220) as one kernel: every level
// of cv.pyrDown + cv.pyrUp of a feature image runs on chip, the crop src[:, :-1] once at the end.
//
// One workgroup per (output image, channel plane).  Three LDS buffers, sized for 128 x 151:
//   P  uint8  [h][w + 1]        the working plane; the first pyrUp makes it w + 1 wide and it stays so
//   T  uint16 [h][(w + 1) / 2]  pyrDown's horizontal pass, then [h / 2][w + 1] pyrUp's horizontal pass
//   D  uint8  [h / 2][(w + 1) / 2]  the half-size image
// 19 + 19 + 4.75 KiB, so three workgroups share a CU's LDS.  A level is four passes with a barrier after
// each; both filters are separable and all arithmetic is exact in integers (the largest intermediate is
// 256 * 255 + 128), so the separable result is the direct 5 x 5 sum's, bit for bit.  Global traffic is one
// read and one write of the image: the three planes of an image are three workgroups that read the same
// interleaved RGB lines, which meet in L2.
//
// Bounds: src and levels are clamped into [0, n) and [0, 8]; every LDS index is derived from h, w, which
// the launcher checks against the buffers' sizes; border taps are folded back inside (reflect-101 for
// pyrDown, reflect before / replicate behind for pyrUp).
#include "od_aug.h"

namespace {

#ifndef ODA_NT
#define ODA_NT 512   // threads per workgroup; 256: -3 %, 1024: -19 % (make variant VDEF=-DODA_NT=...)
#endif
constexpr int NT = ODA_NT;
constexpr int W1_MAX = ODA_MAX_W + 1;
constexpr int PLANE = ODA_MAX_H * W1_MAX;                 // bytes of P
constexpr int HALF = (ODA_MAX_H / 2) * (W1_MAX / 2);      // bytes of D

// BORDER_REFLECT_101 for taps at most two outside [0, n)
__device__ inline int r101(int i, int n) { return i < 0 ? -i : i >= n ? 2 * n - 2 - i : i; }

__global__ void __launch_bounds__(NT) augment_kernel(const uint8_t* __restrict__ img, int n, int h, int w,
                                                     const int32_t* __restrict__ src,
                                                     const int32_t* __restrict__ levels,
                                                     uint8_t* __restrict__ out) {
  __shared__ uint8_t P[PLANE];
  __shared__ uint16_t T[PLANE / 2];
  __shared__ uint8_t D[HALF];
  const int k = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
  const int s = min(max(src[k], 0), n - 1);
  const int L = min(max(levels[k], 0), ODA_MAX_LEVELS);
  const int w1 = w + 1, hh = h / 2, hw = w1 / 2;
  const uint8_t* in = img + (size_t)s * h * w * 3;
  for (int p = tid; p < h * w; p += NT) {
    const int y = p / w, x = p - y * w;
    P[y * w1 + x] = in[(size_t)p * 3 + c];
  }
  __syncthreads();
  for (int lvl = 0; lvl < L; ++lvl) {
    const int wc = lvl == 0 ? w : w1;   // the working width: the extra column is read from level 2 on
    // pyrDown, rows: T[y][x] = sum_j k[j] P[y][r(2 x + j)]
    for (int p = tid; p < h * hw; p += NT) {
      const int y = p / hw, x = p - y * hw;
      const uint8_t* row = P + y * w1;
      const int x2 = 2 * x;
      T[p] = (uint16_t)(row[r101(x2 - 2, wc)] + 4 * row[r101(x2 - 1, wc)] + 6 * row[x2] +
                        4 * row[r101(x2 + 1, wc)] + row[r101(x2 + 2, wc)]);
    }
    __syncthreads();
    // pyrDown, columns: D[y][x] = (sum_i k[i] T[r(2 y + i)][x] + 128) >> 8
    for (int p = tid; p < hh * hw; p += NT) {
      const int y = p / hw, x = p - y * hw;
      const int y2 = 2 * y;
      const int acc = T[r101(y2 - 2, h) * hw + x] + 4 * T[r101(y2 - 1, h) * hw + x] + 6 * T[y2 * hw + x] +
                      4 * T[r101(y2 + 1, h) * hw + x] + T[r101(y2 + 2, h) * hw + x];
      D[p] = (uint8_t)((acc + 128) >> 8);
    }
    __syncthreads();
    // pyrUp, rows: T[y][2 x] = D[x - 1] + 6 D[x] + D[x + 1], T[y][2 x + 1] = 4 (D[x] + D[x + 1]);
    // D[-1] = D[1], D[hw] = D[hw - 1]
    for (int p = tid; p < hh * hw; p += NT) {
      const int y = p / hw, x = p - y * hw;
      const uint8_t* row = D + y * hw;
      const int a = row[x == 0 ? 1 : x - 1], b = row[x], d = row[x == hw - 1 ? x : x + 1];
      T[y * w1 + 2 * x] = (uint16_t)(a + 6 * b + d);
      T[y * w1 + 2 * x + 1] = (uint16_t)(4 * (b + d));
    }
    __syncthreads();
    // pyrUp, columns, the same rule on T; P = (v + 32) >> 6
    for (int p = tid; p < hh * w1; p += NT) {
      const int y = p / w1, x = p - y * w1;
      const int a = T[(y == 0 ? 1 : y - 1) * w1 + x], b = T[p], d = T[(y == hh - 1 ? y : y + 1) * w1 + x];
      P[(2 * y) * w1 + x] = (uint8_t)((a + 6 * b + d + 32) >> 6);
      P[(2 * y + 1) * w1 + x] = (uint8_t)((4 * (b + d) + 32) >> 6);
    }
    __syncthreads();
  }
  uint8_t* o = out + (size_t)k * h * w * 3;
  for (int p = tid; p < h * w; p += NT) {
    const int y = p / w, x = p - y * w;
    o[(size_t)p * 3 + c] = P[y * w1 + x];   // column w, the crop, is left behind
  }
}

}  // namespace

hipError_t oda_augment(const uint8_t* img, int64_t n, int h, int w, const int32_t* src, const int32_t* levels,
                       int64_t m, uint8_t* out, hipStream_t stream) {
  if (!oda_size_ok(h, w) || n < 1 || n > (1 << 24) || m < 0 || m > (1 << 24)) return hipErrorInvalidValue;
  if (m == 0) return hipSuccess;
  hipLaunchKernelGGL(augment_kernel, dim3((unsigned)m, 3), dim3(NT), 0, stream, img, (int)n, h, w, src, levels, out);
  return hipGetLastError();
}
