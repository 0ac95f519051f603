// OD-NET res_blocks 1-3 (overlap_detector_temp.py:253-277) as rolling column strips on gfx950
// 32x32x16 f16 MFMA, 3xFP16 products:
//
//   t1 = Conv2D(32, 3x3, same)(ELU(BN1(x)))                GEMM 1, K = 9 * CIN
//   t2 = Conv2D(32, (4,1), same)(ELU(BN2(t1)))             GEMM 2, K = 4 * 32
//   y  = x + t2                          (blocks 2-3: 64 x 76 x 32)
//   y  = MaxPool2D(2, same)(t2) + Conv2D(32, 1x1, stride 2)(x)
//                                        (block 1, whose x is the stem Conv2D(16, 1x1) of the image,
//                                         computed while staging: 128 x 151 x 3 -> 64 x 76 x 32)
//
// One workgroup (4 waves) owns a 16-column strip of one clip and walks down it in chunks of R = 8
// output rows.  The conv(4,1) is vertical and the 3x3 reaches one row up and down, so a chunk needs
// only R new input rows and R new t1 rows: the rows it shares with the previous chunk stay in two
// LDS rings (x: R + 2 rows of the 18-column halo, t1: R + 3 rows), so no t1 row is computed twice
// and the input is staged 18/16 times instead of the 21 x 18 / 16 x 16 of a 16 x 16 tile.  Per
// chunk: stage the R new x rows (BN1 + ELU + the 2^4 scale + fp16 hi / lo split, from registers
// loaded during the previous chunk) -> barrier -> GEMM 1 (wave w: t1 rows 2w, 2w + 1 of the chunk =
// one 32-pixel tile, as t1^T = W1^T X^T so a lane holds 4-channel quads of one pixel) -> BN2 + ELU
// + split into the t1 ring as 8-byte channel quads -> barrier -> GEMM 2 (wave w: output rows 2w,
// 2w + 1) -> epilogue straight from the accumulators:
//   * blocks 2-3: y^T again (a lane: 16 channels of one pixel), + bias + the raw residual (float4
//     loads issued under GEMM 2's last k-steps);
//   * block 1: y in pixel rows ordered so that a lane's register quad IS one 2x2 pool window;
//     max-pool in registers, + the 1x1 / 2 shortcut as a 3xFP16 MFMA whose A rows are the windows'
//     top-left stem pixels (replicated 4x so its accumulator layout equals the pooled one).
// 32x32x16 MFMAs hold the SIMD's issue port for 8 of their 32 cycles (16x16x32: 8 of 16), which
// leaves the staging / t1 VALU work room beside the matrix pipe.
//
// LDS (hi and lo planes): 16-B channel groups of a pixel XOR-swizzled by column (and, for block 1's
// t1 read in pool-window order, by row parity), rows padded to a multiple of 256 B, so every
// ds_read_b128 of the GEMMs is conflict-free (model: the MI355X guide's lane groups).  Blocks 2-3:
// 47 KB (rbs_w1l.hip, with GEMM 1's weights: 79 KB, two workgroups per CU either way); block 1: 51 KB,
// 16 KB of it GEMM 2's weights (sw2) -> three workgroups per CU (SG::MINB).
//
// 3xFP16 as conv_h3.hip: activations x 2^4 and weights x their power-of-two scale split into hi + lo,
// ONE f32 accumulator per tile (hi*lo + lo*hi + hi*hi); the 2^4 is folded into the BN coefficients
// (exact power-of-two scaling), ELU(u) * 16 = u16 > 0 ? u16 : 16 exp(u) - 16.
//
// The strip body is rbs_body.h.  This file holds the two kernels whose GEMM 1 streams its weights from
// global memory every chunk: block 1, and blocks 2-3 as they run under MMLA_NO_RBS_W1L=1.  By default
// blocks 2-3 run rbs_w1l.hip's kernel, which keeps GEMM 1's weights in LDS for the whole strip, and block 1
// runs rbs_tp.hip's, which pairs the clips' ragged tenth strips (MMLA_NO_RBS_TAILPAIR=1: this file's).
#define RBS_KERNEL rbs_kernel
#define RBS_W1L false
#include "rbs_body.h"

namespace {

template <int H, int W, int CIN, bool POOL, bool STEM>
hipError_t launch(const ResBlkArgs& a, hipStream_t s) {
  using G = SG<H, W, CIN, POOL>;
  const int64_t blocks = (int64_t)a.n * G::STRIPS;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((rbs_kernel<H, W, CIN, POOL, STEM>), dim3((unsigned)blocks), dim3(NT), 0, s, a);
  return hipGetLastError();
}

}  // namespace

#if RBS_TRACE
extern "C" int mmla_debug_rbs_trace(unsigned long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(rbs_trace_buf), sizeof(rbs_trace_buf)) == hipSuccess ? 0 : -2;
}
#endif

bool rbs_supported(int h, int w, int cin, int c, bool pool) {
  return c == 32 && ((h == 128 && w == 151 && cin == 16 && pool) || (h == 64 && w == 76 && cin == 32 && !pool));
}

hipError_t rbs_launch(const ResBlkArgs& a, int cin, int c, bool pool, bool w1_lds, bool tail_pair, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  if (!rbs_supported(a.h, a.w, cin, c, pool) || !a.y || !a.w1h || !a.w1l || !a.w2h || !a.w2l)
    return hipErrorInvalidValue;
  if (pool) {
    if (!a.wsh || !a.wsl || !a.bs) return hipErrorInvalidValue;
    if (a.img8 || a.imgf) return tail_pair ? rbs_tp_launch(a, s) : launch<128, 151, 16, true, true>(a, s);
    return hipErrorInvalidValue;   // block 1 runs with the stem fused
  }
  if (!a.x || a.x == a.y) return hipErrorInvalidValue;
  return w1_lds ? rbs_w1l_launch(a, s) : launch<64, 76, 32, false, false>(a, s);
}
