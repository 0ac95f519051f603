// Layered mixes of int16 recordings (mix.hip): the overlay chain of the reference's overlap synthesis
// (OverlapDetection/scripts/data_augmentation.py:20-34, pydub AudioSegment.overlay = audioop.add).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

constexpr int MIX_MAX_LAYERS = 8;   // MMLA_MIX_MAX_LAYERS

// Clip c of n_clips is n_layers[c] layers (clamped into [0, MIX_MAX_LAYERS]; 0 gives an empty clip) of
// the pool [pool_len] int16; layer l of clip c reads src_len[c][l] samples from pool + src_off[c][l] and
// lands at sample pos[c][l] of the clip (layer 0, the canvas, at 0 whatever pos holds).
//   canvas_len = min(src_len[c][0], clip_len)
//   s < canvas_len:  v = pool[off_0 + s]; for l = 1 .. n_layers - 1 in order, where
//                    pos_l <= s < pos_l + min(len_l, canvas_len - pos_l):  v = clamp16(v + pool[off_l + s - pos_l])
//   canvas_len <= s < clip_len:  0
// out [n_clips][out_stride] int16 (only [0, clip_len) of a row is written), out_len [n_clips] = canvas_len
// (nullable).  All pointers are device pointers; clip_len in [1, 600000].  Whatever the descriptors hold,
// nothing outside [0, pool_len) is read: a layer is clipped to the pool, and one with a negative offset,
// length or position (or an offset past the pool) is skipped (a canvas like that is empty).
struct MixArgs {
  const int16_t* pool;
  int64_t pool_len;
  int64_t n_clips;
  const int32_t* n_layers;   // [n_clips]
  const int64_t* src_off;    // [n_clips][MIX_MAX_LAYERS]
  const int32_t* src_len;    // likewise
  const int32_t* pos;        // likewise
  int32_t clip_len;
  int16_t* out;
  int64_t out_stride;
  int32_t* out_len;
};
hipError_t mix_launch(const MixArgs& a, hipStream_t s);
