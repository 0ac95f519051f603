// OD-NET res_block 1 (128 x 151 x 3 image -> 64 x 76 x 32, stem fused) as rolling column strips with the
// ragged last strips paired: the strip kernel of rbs_body.h (rbs.hip documents it) with RBS_TAILPAIR on.
//
// 151 = 9 x 16 + 7: rbs.hip's kernel gives every clip a tenth workgroup that runs all 16 chunks, 54 + 24
// + 3 MFMAs per wave and chunk, for a 16-column strip of which 7 columns are in the image.  A workgroup's
// time does not depend on how many of its columns are live, so that is 9 of every 160 strip columns of
// the launch.  Here the tails of clips 2p and 2p + 1 share one workgroup: 9 n + ceil(n / 2) workgroups
// instead of 10 n (-5.0 % at even n).
//
//   ring column (18)   0 .. 8   image columns 143 .. 151 of clip 2p     (151: zero padding)
//                      9 .. 17  image columns 143 .. 151 of clip 2p + 1
//   tile column (16)   0 .. 6   outputs 144 .. 150 of clip 2p,     3x3 tap dx reads ring column c + dx
//                      8 .. 14  outputs 144 .. 150 of clip 2p + 1, tap dx reads ring column c + 1 + dx
//                      7, 15    junk: read the zero ring column of their half (8, 17) for every dx
//   pool window (8)    0 .. 3   pooled columns 72 .. 75 of clip 2p;  4 .. 7: of clip 2p + 1
//
// The second half starts at the even tile column 8 because a pool window is a register quad of tile
// columns 2 w, 2 w + 1.  Windows 3 and 7 hold output column 150 and a junk column: the 'same' pool's cut
// window (cc + 1 >= W) replaces the junk column exactly as it replaces column 151 in rbs.hip's kernel.
// Neither half reads a ring column of the other, both clips are contiguous in the image buffer and share
// one buffer descriptor, and with n odd the last pair's second clip does not exist: its ring half is
// zeroed, none of its tasks stage, its shortcut operand is zero and its stores are skipped.  Only the
// column tables computed before the chunk loop differ from rbs.hip's kernel; rings, swizzles, MFMA
// sequence and chunk loop are its own, so every output has the same bits.
//
// The 3xFP16 range flag keeps its meaning.  It is raised by the largest |operand| any thread splits.  The
// live columns split what they split in rbs.hip's kernel.  A junk column stages nothing; its t1 is
// ELU(BN2(b1)) per channel, the value every out-of-image t1 column (151 .. 159 of rbs.hip's tenth strip)
// already folds into the maximum; its shortcut window is a live window's.  An absent clip adds zeros.
//
// The shortcut's stem, once per window (RBS_SC_DEDUP, on; -DRBS_SC_DEDUP=false builds the A/B partner).
// The pool epilogue's shortcut MFMA wants 32 A rows and a wave has 8 pool windows, so A row m is window
// m >> 2 and rbs.hip's kernel has lanes n, n ^ 1, n ^ 2, n ^ 3 each compute the same eight stem channels
// of the same pixel, split them and fold them into the range maximum.  Here lane n computes channels
// 8 h + 2 j and 8 h + 2 j + 1 (j = n & 3) with the same expressions, splits the pair with split4's
// operations (one v_cvt_pk, one split_lo2), and the quad assembles the two operand register quads with
// eight DPP quad_perm broadcasts: 32 VALU instructions fewer per wave and chunk (660 -> 628 as
// compiled; rbs.hip's kernel: 656), the same operand bits, and the same set of values per wave in the range
// maximum.
//
// env MMLA_NO_RBS_TAILPAIR=1 at mmla_create runs rbs.hip's kernel instead (A/B, bit-identical).
#define RBS_KERNEL rbs_tp_kernel
#define RBS_W1L false
#define RBS_TAILPAIR true
#ifndef RBS_SC_DEDUP
#define RBS_SC_DEDUP true
#endif
#include "rbs_body.h"

#if RBS_TRACE
extern "C" int mmla_debug_rbs_tp_trace(unsigned long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(rbs_trace_buf), sizeof(rbs_trace_buf)) == hipSuccess ? 0 : -2;
}
#endif

// the arguments are rbs_launch's, which has checked them
hipError_t rbs_tp_launch(const ResBlkArgs& a, hipStream_t s) {
  using G = SG<128, 151, 16, true>;
  const int64_t blocks = (int64_t)a.n * (G::STRIPS - 1) + (a.n + 1) / 2;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((rbs_tp_kernel<128, 151, 16, true, true>), dim3((unsigned)blocks), dim3(NT), 0, s, a);
  return hipGetLastError();
}
