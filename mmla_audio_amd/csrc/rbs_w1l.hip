// OD-NET res_blocks 2-3 (64 x 76 x 32) as rolling column strips with GEMM 1's weights in LDS: the strip
// kernel of rbs_body.h (rbs.hip documents it) with RBS_W1L on.
//
// rbs.hip's kernel has every wave fetch the whole split 3x3 weight set from global memory in every
// chunk: 18 k-steps x (hi + lo) x 1 KB = 36.9 KB, the same fragments in all four waves, 1.18 MB per
// strip for 36.9 KB of distinct data -- 2 KB of vector loads per 3 MFMAs, which the CU's vector-memory
// path has to carry for both resident workgroups.  Here the workgroup copies the weights into LDS once
// per strip and GEMM 1 reads its fragments by ds_read_b128 at lane * 16 B, one k-step ahead: four LDS
// reads per three MFMAs per wave, and no vector load in the GEMM.  The kernel is register-limited to
// two workgroups per CU either way, so the extra LDS costs no occupancy: 45 952 B of rings and
// parameters + 17 of the 18 k-steps (34 816 B) = 80 768 B of the 81 920 B a workgroup may use; the
// last k-step's two fragments stay in registers for the strip.  Same MFMA sequence per accumulator,
// same bits.  Block 1 (51 072 B at three workgroups per CU) has no room for this.
#define RBS_KERNEL rbs_w1l_kernel
#define RBS_W1L true
#include "rbs_body.h"

#if RBS_TRACE
extern "C" int mmla_debug_rbs_w1l_trace(unsigned long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(rbs_trace_buf), sizeof(rbs_trace_buf)) == hipSuccess ? 0 : -2;
}
#endif

// the arguments are rbs_launch's, which has checked them
hipError_t rbs_w1l_launch(const ResBlkArgs& a, hipStream_t s) {
  using G = SG<64, 76, 32, false>;
  const int64_t blocks = (int64_t)a.n * G::STRIPS;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((rbs_w1l_kernel<64, 76, 32, false, false>), dim3((unsigned)blocks), dim3(NT), 0, s, a);
  return hipGetLastError();
}
