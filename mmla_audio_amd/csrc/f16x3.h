// The 3xFP16 operand contract shared by conv_h3.hip and the fused kernels that replace its launches
// (rbs.hip, odu.hip; siu.hip and resblk.hip take the types and constants): activations x 2^4 and
// weights x their power-of-two scale are split into fp16 hi + lo, and one f32 accumulator per tile
// takes hi*lo + lo*hi + hi*hi.  A fused kernel is bit-identical to the conv_h3 launches it replaces
// only while both stage the same operands, so everything that produces an operand lives here once.
// split_lo2 and elu16 moved here from common.h for that reason: they are part of this contract and
// nothing outside it uses them.
#pragma once
#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

constexpr float ACT_SCALE = 16.0f;     // 2^4: every staged activation
constexpr float SPLIT_MAX = 65504.0f;  // largest finite fp16 (operands are compared once scaled)

// lo halves of the 3xFP16 split of two scaled values a, b whose hi halves are the f16 pair `hi`
// (bits 0-15 = f16(a), 16-31 = f16(b)): f16(a - hi.a), f16(b - hi.b) by v_fma_mix -- the exact
// difference rounded once, bit-identical to cvt(a - f32(hi.a)) (a - hi is exact in f32); two VALU
// where clang emits cvt + sub + cvt per value.  a, b must be plain VALU results (no MFMA / trans
// producer hazard is visible to the compiler inside the asm).
MMLA_DEV uint32_t split_lo2(float a, float b, uint32_t hi) {
  uint32_t lo;
  asm("v_fma_mixlo_f16 %0, %1, 1.0, -%2 op_sel_hi:[0,0,1]\n\t"
      "v_fma_mixhi_f16 %0, %3, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
      : "=&v"(lo) : "v"(a), "v"(hi), "v"(b));
  return lo;
}

// 16 ELU(u) from u16 = 16 u (TF Elu: exp(x) - 1 for x < 0; the power-of-two scaling commutes with every
// rounding).  With e = 16 exp(u) - 16: u > 0 gives 0 < u < e (or e = inf), u <= 0 gives u <= e <= 0,
// so ELU is the median of (u, e, 0) -- one v_med3 instead of a compare and a select.  (Where the
// rounding of e puts it a hair below u, for |u16| ~ 1e-3, the median returns u: within 1e-6.)  Every
// 3xFP16 ELU (rbs, odu, conv_h3's PRO_BN_ELU) uses it, so the fused kernels stay bit-identical to the
// conv_h3 launches they replace.
MMLA_DEV float elu16(float u16) {
  constexpr float L2E_16 = 1.4426950408889634f / 16.0f;   // log2(e) / 2^4
  const float e = fmaf(__builtin_amdgcn_exp2f(u16 * L2E_16), 16.0f, -16.0f);
  return __builtin_amdgcn_fmed3f(u16, e, 0.0f);
}

// conv_h3's PRO_BN_ELU prologue x 2^4 (sc16, sh16 = 2^4 x the folded BatchNorm: exact)
MMLA_DEV float bn_elu16(float v, float sc16, float sh16) { return elu16(fmaf(v, sc16, sh16)); }
MMLA_DEV float4 x16(float4 v) { return make_float4(ACT_SCALE * v.x, ACT_SCALE * v.y, ACT_SCALE * v.z, ACT_SCALE * v.w); }

// (a, b, c, d), already x 2^4, = hi + lo, both fp16 (RNE); lo = f16(v - hi) rounded once (split_lo2)
MMLA_DEV void split4(float a, float b, float c, float d, f16x4& h, f16x4& l) {
  h[0] = (_Float16)a;
  h[1] = (_Float16)b;
  h[2] = (_Float16)c;
  h[3] = (_Float16)d;
  const uint2 hu = __builtin_bit_cast(uint2, h);
  l = __builtin_bit_cast(f16x4, make_uint2(split_lo2(a, b, hu.x), split_lo2(c, d, hu.y)));
}
MMLA_DEV void split4(float4 v, f16x4& h, f16x4& l) { split4(v.x, v.y, v.z, v.w, h, l); }

// the largest |operand| of a split quad, and folded into a running range maximum r (checked against
// SPLIT_MAX at the end of the kernel: ResBlkArgs / OduArgs::range_flag)
MMLA_DEV float amax4(float a, float b, float c, float d) {
  return fmaxf(fmaxf(fabsf(a), fabsf(b)), fmaxf(fabsf(c), fabsf(d)));
}
MMLA_DEV float amax4(float r, float4 v) { return fmaxf(r, amax4(v.x, v.y, v.z, v.w)); }

// A caller's float input (image pixel, feature cell) is the only way a NaN or an inf enters the 3xFP16
// path: finite in-range operands and finite weights give finite sums, and an overflow gives inf, which
// the folds above catch.  They do not catch NaN (fmaxf returns its other argument, elu16's median turns
// NaN into 0), so every kernel that reads such an input tests it once, here: x * 0 is NaN for NaN and
// +-inf and 0 otherwise.  true: the micro-batch must be flagged (range_flag) like an operand out of range
MMLA_DEV bool nonfinite3(float a, float b, float c) {
  const float s = fmaf(a, 0.0f, fmaf(b, 0.0f, c * 0.0f));
  return s != s;
}

// A split weight tensor (conv_h3_split_weights order) through a wave-uniform buffer descriptor: a
// fragment load is voffset = the lane's 32-bit offset, soffset = the uniform (tap, k-step) offset, so
// no load costs 64-bit address VALU
MMLA_DEV __amdgpu_buffer_rsrc_t w_rsrc(const void* p) {
  const uint64_t u = reinterpret_cast<uint64_t>(p);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)u);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(u >> 32));
  return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((uint64_t)hi << 32) | lo), (short)0,
                                           (int)0x7fffffff, 0x00020000);
}
// 16 B of a split weight: wave-uniform half index uoff + this lane's lofs
MMLA_DEV f16x8 w_frag(__amdgpu_buffer_rsrc_t r, size_t uoff, int lofs) {
  return __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(r, (uint32_t)lofs * 2u, (int)(uoff * 2), 0));
}

// An LDS operand pipeline's issue order, for the scheduler.  A group is the fragments of one (tap,
// k-step, tile) and its three MFMAs; the fragments are read LA groups ahead, and each group is pinned
// as "NR LDS reads (a later group's fragments), then 3 MFMAs".  The sched_barrier ends the region:
// without it the scheduler fits the groups of the whole unrolled loop at once, sinks the reads below
// the MFMAs again and shares their registers.  LA = 0 (fragments read right before their MFMAs) pins
// nothing and leaves the order to the scheduler.
template <int LA, int NR>
MMLA_DEV void pin_group() {
  if constexpr (LA > 0) {
    if constexpr (NR > 0) __builtin_amdgcn_sched_group_barrier(0x100, NR, 0);   // DS_READ
    __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);                          // MFMA
    __builtin_amdgcn_sched_barrier(0);
  }
}
