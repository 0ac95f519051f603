// SpeakerIdentification res units, one to three of them per fused kernel launch.  See siu.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct SiuArgs {
  const float* x;          // [n * t, C] the unit's input (raw: also its residual), rows of all clips
  float* y;                // [n * t, C] x + Conv1D_b(ReLU(BN_mid(Conv1D_a(ReLU(BN_in(x)))))), y != x
  const uint16_t* wah;     // the two Conv1D(C, 3) weights, conv_h3_split_weights layout (cin = cout = C)
  const uint16_t* wal;
  const uint16_t* wbh;
  const uint16_t* wbl;
  const float* ba;         // biases [C]
  const float* bb;
  const float* s_in;       // folded BatchNorms [C]: v * s + t
  const float* t_in;
  const float* s_mid;
  const float* t_mid;
  float ua, ub;            // 1 / (2^4 x the weight tensor's split scale), conv_h3's unscale
  int n, t;                // clips, rows per clip (pool units: pooled rows, (t_src + 1) / 2)
  int* range_flag;         // nullable: an operand split into fp16 left the fp16 range
  // pool units only: x is [n * t_src, CIN]; the shortcut Conv1D(C, 1, strides=2)
  int t_src;
  const uint16_t* wsh;     // its weight, conv_h3_split_weights layout (cin = CIN, cout = C)
  const uint16_t* wsl;
  const float* bs;         // its bias [C]
  float us;                // its unscale
  // seq set (the last unit of the net, siu_chain_supported's fin): instead of y, seq [n * t / 4, C] =
  // AveragePooling1D(4)(ReLU(x_out * fs + ft)) (the final BatchNormalization, folded)
  float* seq;
  const float* fs;
  const float* ft;
  uint32_t tdiv_m, tdiv_s;   // set by the launcher: row / t as a multiply-high (callers leave 0)
};

// A chain of consecutive units as one launch: with `pool` a pool unit (cin -> c channels) first, then
// units without pooling (c channels).  units[0].x is the chain's input and the last unit's y (or seq:
// fin) its output; the x / y in between are unused, the intermediates stay on chip.  Chains: a pool
// unit alone or with the two units after it, and one or two units without pooling.
bool siu_chain_supported(int cin, int c, bool pool, int n_units, bool fin);
hipError_t siu_chain_launch(const SiuArgs* units, int n_units, bool pool, int cin, int c, hipStream_t stream);
