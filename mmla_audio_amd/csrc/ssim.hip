// Mean structural similarity (SSIM) of uint8 image pairs: the silent check of the OD edge loop
// (OverlapDetection/scripts/record_on_pi.py:39-48), skimage.metrics.structural_similarity(im1, im2,
// multichannel=True) with its defaults for uint8 input, for a whole batch in one launch.
//
// Integer form.  Per channel and window position, with the 7 x 7 sums sx, sy, sxx, syy, sxy of x, y,
// x^2, y^2, xy (exact integers) and NP = 49:
//   A1 = 2 sx sy + NP^2 C1                    B1 = sx^2 + sy^2 + NP^2 C1
//   A2 = 2 (NP sxy - sx sy) + NP (NP-1) C2    B2 = (NP sxx - sx^2) + (NP syy - sy^2) + NP (NP-1) C2
//   S  = A1 A2 / (B1 B2)
// which is scikit-image's ((2 ux uy + C1)(2 vxy + C2)) / ((ux^2 + uy^2 + C1)(vx + vy + C2)) with
// numerator and denominator multiplied by NP^3 (NP - 1).  Every integer part is <= 312 250 050, so it
// is formed exactly in int32 and converted to float32 once; the rest is float32.  Two equal images give
// A1 == B1 and A2 == B2 bit for bit, hence S = 1 exactly.
//
// Dataflow: separable sliding sums.  One workgroup per pair; thread t owns the interleaved (column,
// channel) element e = e0 + t of a row and walks down the rows.  It keeps the last 7 rows' x and y
// bytes of its element in registers (a ring indexed at compile time: the row loop is unrolled by 7), so
// every input byte is read from HBM exactly once, coalesced along the row, and the five 7-row vertical
// sums are updated with one add and one subtract each.  From row 6 on the thread hands its vertical
// sums through a double-buffered LDS row (sx and sy packed into one word: both are < 2^16 even after
// the horizontal pass) to the horizontal pass: thread t sums the 7 taps t, t + c, ..., t + 6c and adds
// the window's S to its own running sum.  Rows wider than a workgroup are done in column chunks of
// NT - 6c outputs, one after the other.  The per-pair mean is reduced in a fixed order (each thread's
// rows in order, a butterfly per wave, the waves in order): no atomics, bit-reproducible.
// LDS: 2 x 4 x 512 x 4 B = 16 KB per workgroup of 8 waves; 69 VGPRs: three workgroups per CU.
// Measured: 0.57 ms for 4096 pairs of 128 x 151 x 3 (0.83 TB/s); the horizontal pass's
// 28 LDS words per window position are the limit, not HBM.
#include <type_traits>

#include "common.h"
#include "ssim.h"

namespace {

constexpr int NT = 512;
constexpr int NP = SSIM_WIN * SSIM_WIN;

// the full-rate integer multiply and multiply-add: both factors within 24 bits (signed), the low 32
// bits of the result.  (clang picks the quarter-rate v_mul_lo_u32 / v_mad_u64_u32 where it cannot
// prove the range, as for the ring's bytes)
MMLA_DEV int mul24(int a, int b) {
  int r;
  asm("v_mul_i32_i24 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
MMLA_DEV int mad24(int a, int b, int c) {
  int r;
  asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

__global__ __launch_bounds__(NT) void ssim_u8_kernel(const uint8_t* __restrict__ a,
                                                      const uint8_t* __restrict__ b, int h, int w, int c,
                                                      float* __restrict__ out) {
  __shared__ int rowbuf[2][4][NT];
  __shared__ float red[NT / 64];
  const int t = threadIdx.x;
  const int wc = w * c;
  const int nout = wc - 6 * c;   // window positions per row x channels
  const int step = NT - 6 * c;   // of them per column chunk
  const int64_t img = (int64_t)h * wc;
  const uint8_t* pa = a + (int64_t)blockIdx.x * img;
  const uint8_t* pb = b + (int64_t)blockIdx.x * img;
  // K1 = 0.01, K2 = 0.03, data_range 255
  constexpr float KC1 = (float)(NP * NP * (0.01 * 255) * (0.01 * 255));
  constexpr float KC2 = (float)(NP * (NP - 1) * (0.03 * 255) * (0.03 * 255));
  float acc = 0.0f;
  for (int e0 = 0; e0 < nout; e0 += step) {
    const int e = e0 + t;
    const bool ld = e < wc;                    // this thread's element exists
    const bool outp = t < step && e < nout;    // ... and is the left tap of a window of this chunk
    int rx[SSIM_WIN], ry[SSIM_WIN];
#pragma unroll
    for (int k = 0; k < SSIM_WIN; ++k) rx[k] = ry[k] = 0;
    int sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
    int nx = 0, ny = 0;   // the next row's bytes, loaded one row ahead
    if (ld) {
      nx = pa[e];
      ny = pb[e];
    }
    __syncthreads();   // the previous chunk's last row has been read
    // one row: r = the row, k = its place in the ring (r % 7, a compile-time constant at every call),
    // emit = a window's last row (r >= 6): hand the vertical sums to the horizontal pass.  The
    // products are 24-bit multiplies (full rate; every operand is below 2^24)
    auto row = [&](int r, auto K, bool emit) __attribute__((always_inline)) {
      constexpr int k = decltype(K)::value;
      const int x = nx, y = ny, ox = rx[k], oy = ry[k];
      if (ld && r + 1 < h) {
        nx = pa[(int64_t)(r + 1) * wc + e];
        ny = pb[(int64_t)(r + 1) * wc + e];
      }
      rx[k] = x;
      ry[k] = y;
      sx += x - ox;
      sy += y - oy;
      sxx = mad24(x - ox, x + ox, sxx);
      syy = mad24(y - oy, y + oy, syy);
      sxy = mad24(x, y, sxy) - mul24(ox, oy);
      if (!emit) return;
      int(*buf)[NT] = rowbuf[r & 1];
      buf[0][t] = sx | (sy << 16);
      buf[1][t] = sxx;
      buf[2][t] = syy;
      buf[3][t] = sxy;
      __syncthreads();   // one barrier per row: the next row writes the other buffer
      if (outp) {
        int pxy = 0, hxx = 0, hyy = 0, hxy = 0;
#pragma unroll
        for (int j = 0; j < SSIM_WIN; ++j) {
          const int i = t + j * c;   // <= step - 1 + 6c = NT - 1
          pxy += buf[0][i];
          hxx += buf[1][i];
          hyy += buf[2][i];
          hxy += buf[3][i];
        }
        const int hx = pxy & 0xffff, hy = (int)((unsigned)pxy >> 16);
        const int xy = mul24(hx, hy);
        const float A1 = (float)(2 * xy) + KC1;
        const float B1 = (float)(mul24(hx, hx) + mul24(hy, hy)) + KC1;
        const float A2 = (float)(2 * (mul24(NP, hxy) - xy)) + KC2;
        const float B2 = (float)(mul24(NP, hxx + hyy) - mul24(hx, hx) - mul24(hy, hy)) + KC2;
        acc += (A1 * A2) / (B1 * B2);
      }
    };
    auto rows7 = [&](int r0, int cnt, bool first) __attribute__((always_inline)) {   // rows r0 .. r0 + cnt - 1, r0 a multiple of 7
      auto one = [&](auto K) __attribute__((always_inline)) {
        constexpr int k = decltype(K)::value;
        if (k < cnt) row(r0 + k, K, !first || k == SSIM_WIN - 1);
      };
      one(std::integral_constant<int, 0>());
      one(std::integral_constant<int, 1>());
      one(std::integral_constant<int, 2>());
      one(std::integral_constant<int, 3>());
      one(std::integral_constant<int, 4>());
      one(std::integral_constant<int, 5>());
      one(std::integral_constant<int, 6>());
    };
    rows7(0, SSIM_WIN, true);   // h >= 7: the first window's rows, one output row
    int r0 = SSIM_WIN;
    for (; r0 + SSIM_WIN <= h; r0 += SSIM_WIN) rows7(r0, SSIM_WIN, false);
    if (r0 < h) rows7(r0, h - r0, false);
  }
  acc = wave_sum(acc);
  if ((t & 63) == 0) red[t >> 6] = acc;
  __syncthreads();
  if (t == 0) {
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) s += red[i];
    out[blockIdx.x] = s / (float)((int64_t)(h - 6) * nout);
  }
}

__global__ void fill_f32_kernel(float* __restrict__ out, int64_t n, float v) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = v;
}

}  // namespace

hipError_t ssim_u8_launch(const uint8_t* a, const uint8_t* b, int64_t n, int h, int w, int c,
                          float* out, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (h < SSIM_WIN || w < SSIM_WIN || (c != 1 && c != 3 && c != 4) || n > 0x7fffffff)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(ssim_u8_kernel, dim3((unsigned)n), dim3(NT), 0, s, a, b, h, w, c, out);
  return hipGetLastError();
}

hipError_t fill_f32_launch(float* out, int64_t n, float v, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(fill_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, out, n, v);
  return hipGetLastError();
}
