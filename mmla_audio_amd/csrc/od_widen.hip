// A one-channel OD model's images as the network reads them (nets.h od_widen_launch): g [n_pix] ->
// y [n_pix][3] = (g, g, g), what decode_png(gray png, 3) gives.  The loaded stem's rows 1 and 2 are zero
// (weights.cpp), so the three-channel kernels compute the one-channel network on it.  It runs only at the
// entries that take a caller's images (mmla_od_forward, _u8, the debug trace), never inside a pipeline.
// Kept out of nets.hip: built into that file, in front of mean_h4_kernel, the pipeline's mean-over-H launch
// measured 10 % slower.
#include "common.h"
#include "nets.h"

namespace {

// thread i writes element i of y [n_pix][3]
template <typename T>
__global__ void od_widen_kernel(const T* __restrict__ g, int64_t n_pix, T* __restrict__ y) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_pix * 3) return;
  y[i] = g[i / 3];
}

}  // namespace

hipError_t od_widen_launch(const uint8_t* g_u8, const float* g_f32, int64_t n_pix, void* y, hipStream_t s) {
  if (n_pix <= 0) return hipSuccess;
  if ((g_u8 == nullptr) == (g_f32 == nullptr) || !y) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((n_pix * 3 + 255) / 256));
  if (g_u8)
    hipLaunchKernelGGL(od_widen_kernel<uint8_t>, grid, dim3(256), 0, s, g_u8, n_pix, static_cast<uint8_t*>(y));
  else
    hipLaunchKernelGGL(od_widen_kernel<float>, grid, dim3(256), 0, s, g_f32, n_pix, static_cast<float*>(y));
  return hipGetLastError();
}
