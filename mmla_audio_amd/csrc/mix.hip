// Layered mixes of int16 recordings: pydub's AudioSegment.overlay chain (audioop.add per layer, each sum
// clamped to int16, so the order of the layers matters) for a batch of clips that all read one
// device-resident pool.  The rule is mix.h's; tests/mix_ref.py restates it in numpy.
//
// Memory-bound and small (at most (1 + layers) x 2 bytes per sample), so it is kept plain: a workgroup
// serves one clip, whose descriptors are therefore the same in every lane (read through the first lane,
// they live in scalar registers); a thread produces 8 consecutive samples and stores them as 16 bytes
// where the row's address allows.  Pool offsets are arbitrary, so the sources are read sample by sample
// (2-byte loads: the 8 loads of a wave cover one contiguous KB).
#include <hip/hip_runtime.h>

#include "mix.h"

namespace {

constexpr int NT = 256;   // threads of a workgroup
constexpr int SPT = 8;    // samples of a thread

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int64_t uni64(int64_t v) {
  const uint32_t lo = (uint32_t)uni((int)(uint32_t)v), hi = (uint32_t)uni((int)(v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// the samples of a layer that lie inside the pool: 0 for a descriptor that points outside it
__device__ __forceinline__ int layer_len(int64_t off, int len, int64_t pool_len) {
  if (off < 0 || len < 0 || off > pool_len) return 0;
  return (int)min((int64_t)len, pool_len - off);
}

// grid: bpc workgroups per clip, clips [clip0, clip0 + gridDim.x / bpc)
__global__ __launch_bounds__(NT) void mix_kernel(MixArgs a, int64_t clip0, int bpc) {
  const int64_t c = clip0 + blockIdx.x / bpc;
  const int s0 = (int)((blockIdx.x % bpc) * NT + threadIdx.x) * SPT;
  const int64_t d = c * MIX_MAX_LAYERS;
  const int nl = min(max(uni(a.n_layers[c]), 0), MIX_MAX_LAYERS);
  int64_t off0 = 0;
  int canvas_len = 0;
  if (nl > 0) {
    off0 = uni64(a.src_off[d]);
    canvas_len = min(layer_len(off0, uni(a.src_len[d]), a.pool_len), a.clip_len);
  }
  if (s0 == 0 && a.out_len) a.out_len[c] = canvas_len;
  if (s0 >= a.clip_len) return;

  int v[SPT];
#pragma unroll
  for (int j = 0; j < SPT; ++j) v[j] = s0 + j < canvas_len ? (int)a.pool[off0 + s0 + j] : 0;
  for (int l = 1; l < nl; ++l) {
    const int p = uni(a.pos[d + l]);
    const int64_t off = uni64(a.src_off[d + l]);
    if (p < 0 || p >= canvas_len) continue;
    const int n = min(layer_len(off, uni(a.src_len[d + l]), a.pool_len), canvas_len - p);
    const int k0 = s0 - p;   // the layer's sample under v[0]
    if (n <= 0 || k0 >= n || k0 + SPT <= 0) continue;
    const int16_t* src = a.pool + off;   // k in [0, n): off + k < off + len <= pool_len
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      const int k = k0 + j;
      if (k >= 0 && k < n) v[j] = min(max(v[j] + (int)src[k], -32768), 32767);
    }
  }

  int16_t* dst = a.out + c * a.out_stride + s0;
  if (s0 + SPT <= a.clip_len && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
    uint4 w;
    w.x = (uint32_t)(uint16_t)v[0] | ((uint32_t)(uint16_t)v[1] << 16);
    w.y = (uint32_t)(uint16_t)v[2] | ((uint32_t)(uint16_t)v[3] << 16);
    w.z = (uint32_t)(uint16_t)v[4] | ((uint32_t)(uint16_t)v[5] << 16);
    w.w = (uint32_t)(uint16_t)v[6] | ((uint32_t)(uint16_t)v[7] << 16);
    *reinterpret_cast<uint4*>(dst) = w;
  } else {
#pragma unroll
    for (int j = 0; j < SPT; ++j)
      if (s0 + j < a.clip_len) dst[j] = (int16_t)v[j];
  }
}

}  // namespace

hipError_t mix_launch(const MixArgs& a, hipStream_t s) {
  if (a.n_clips <= 0) return hipSuccess;
  if (a.clip_len < 1 || a.clip_len > 600000 || a.out_stride < a.clip_len) return hipErrorInvalidValue;
  const int bpc = ((a.clip_len + SPT - 1) / SPT + NT - 1) / NT;
  const int64_t per_launch = 0x7fffffff / bpc;   // clips within the grid's 2^31 - 1 workgroups
  for (int64_t c0 = 0; c0 < a.n_clips; c0 += per_launch) {
    const int64_t cnt = a.n_clips - c0 < per_launch ? a.n_clips - c0 : per_launch;
    hipLaunchKernelGGL(mix_kernel, dim3((unsigned)(cnt * bpc)), dim3(NT), 0, s, a, c0, bpc);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
