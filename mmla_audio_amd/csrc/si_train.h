// The sigmoid-head trainer of speaker registration (transfer_learning stage 1) as one persistent
// kernel.  See si_train.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct SiTrainArgs {
  const float* emb;          // [n_train, 512] frozen-base embeddings (mmla_si_embed)
  const int32_t* labels;     // [n_train] in [0, k)
  const float* val_emb;      // [n_val, 512] (unused when n_val == 0)
  const int32_t* val_labels; // [n_val]
  const float* w0;           // [R, 512, k] initial heads
  const float* b0;           // [R, k]
  const int32_t* perm;       // [R, epochs, n_train] sample order of every epoch
  float* w;                  // [R, 512, k] trained heads
  float* b;                  // [R, k]
  float* history;            // [R, epochs, 4] loss, acc, val_loss, val_acc (nullable)
  int n_train, n_val, k, epochs, batch;
  float lr;
};

// grid = n_restarts workgroups; k <= MMLA_SI_TRAIN_MAX_CLASSES, every size >= 1 (the caller checks)
hipError_t si_train_launch(const SiTrainArgs& a, int n_restarts, hipStream_t stream);
