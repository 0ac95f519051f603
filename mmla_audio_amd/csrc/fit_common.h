// libmmla: what the whole-network trainers share (si_finetune.cpp, od_finetune.cpp, capi.cpp's head trainer).
// Host code only: carving one workspace slot, staging host-pointer operands in it, the argument checks and the
// fit driver -- the epochs == 0 identity, the epoch / batch / validation loops, the two Keras callbacks and the
// final copies.  An entry supplies its engine's carving and its launches.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "internal.h"

namespace mmla __attribute__((visibility("hidden"))) {

// ---- carving a workspace slot --------------------------------------------------------------------------

// hands out 256-byte aligned pieces of one allocation; with a null base it only measures
struct Carver {
  char* base;
  size_t total = 0;
  template <typename T>
  T* take(size_t count) {
    const size_t at = total;
    total += (count * sizeof(T) + 255) & ~(size_t)255;
    return base ? reinterpret_cast<T*>(base + at) : nullptr;
  }
};

// fn(Carver&) -> int runs twice: on a null base to measure, then on `slot` grown to that size.  A pass
// that takes what the other did not would overlap buffers or leave the allocation: that is an error here,
// before anything uses the pointers.
template <typename Fn>
int carve_slot(mmla_ctx* c, int slot, Fn&& fn) {
  Carver measure{nullptr};
  CHK(fn(measure));
  void* p = nullptr;
  CHK(ws_get(c, slot, measure.total, &p));
  Carver cv{static_cast<char*>(p)};
  CHK(fn(cv));
  if (cv.total != measure.total)
    return fail(c, MMLA_E_HIP, "workspace slot %d: carved %zu bytes of the %zu measured", slot, cv.total,
                measure.total);
  return MMLA_OK;
}

// ---- staged operands -----------------------------------------------------------------------------------

// A call's operands are device pointers (MMLA_DEVICE_PTR) or host pointers; the latter get a device copy
// carved from the call's slot.  Each method names an operand once; the ones that take run in both passes
// of carve_slot and enqueue their upload in the pass that has memory.
struct Stager {
  mmla_ctx* c;
  bool dev;
  hipMemcpyKind kind_in() const { return dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice; }
  hipMemcpyKind kind_out() const { return dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost; }
  // a device copy of `count` host elements, whatever the mode
  template <typename T>
  int up(Carver& cv, const T* host, size_t count, const T** d) {
    T* copy = cv.take<T>(count);
    *d = copy;
    if (copy && count)
      HIPCHK(c, hipMemcpyAsync(copy, host, count * sizeof(T), hipMemcpyHostToDevice, c->stream));
    return MMLA_OK;
  }
  // an input: the caller's device pointer, or the copy of a host one (non-null, count > 0)
  template <typename T>
  int in(Carver& cv, const T* user, size_t count, const T** d) {
    *d = user;
    return dev || !user || !count ? MMLA_OK : up(cv, user, count, d);
  }
  // an output: the caller's device pointer, or a device buffer that back() copies out
  template <typename T>
  T* out(Carver& cv, T* user, size_t count) {
    return dev || !user ? user : cv.take<T>(count);
  }
  template <typename T>
  int back(T* user, const T* d, size_t count) {
    if (dev || !user || !count) return MMLA_OK;
    HIPCHK(c, hipMemcpyAsync(user, d, count * sizeof(T), hipMemcpyDeviceToHost, c->stream));
    return MMLA_OK;
  }
};

// ---- argument checks (host pointers; device-pointer callers guarantee their labels and permutations) ----

// perm [rows, n]: the first row that repeats or leaves out a value of 0..n-1, or -1
inline int64_t bad_perm_row(const int32_t* perm, int64_t rows, int64_t n) {
  std::vector<uint8_t> seen(n > 0 ? n : 0);
  for (int64_t r = 0; r < rows; ++r) {
    std::fill(seen.begin(), seen.end(), 0);
    const int32_t* p = perm + (size_t)r * n;
    for (int64_t i = 0; i < n; ++i) {
      if (p[i] < 0 || p[i] >= n || seen[p[i]]) return r;
      seen[p[i]] = 1;
    }
  }
  return -1;
}

inline int check_perm(mmla_ctx* c, const char* who, const int32_t* perm, int64_t rows, int64_t n) {
  const int64_t bad = bad_perm_row(perm, rows, n);
  if (bad < 0) return MMLA_OK;
  return fail(c, MMLA_E_INVALID, "%s: perm row %d is not a permutation of 0..%lld", who, (int)bad,
              (long long)(n - 1));
}

// l [n] in 0..K-1; `set`: how the message names that range (null: "[0, K)")
inline int check_labels(mmla_ctx* c, const char* what, const int32_t* l, int64_t n, int K,
                        const char* set = nullptr) {
  for (int64_t i = 0; i < n; ++i) {
    if (l[i] >= 0 && l[i] < K) continue;
    if (set) return fail(c, MMLA_E_INVALID, "%s[%lld] = %d outside %s", what, (long long)i, l[i], set);
    return fail(c, MMLA_E_INVALID, "%s[%lld] = %d outside [0, %d)", what, (long long)i, l[i], K);
  }
  return MMLA_OK;
}

// ---- pieces both engines set up the same way -------------------------------------------------------------

// the BiLSTM's weights and their gradients inside the blob's copy W and its gradient G; off has lk, lr, lb
template <typename Lstm, typename Off>
void wire_lstm(Lstm& l, const Off& off, float* W, float* G) {
  for (int d = 0; d < 2; ++d) {
    l.wk[d] = W + off.lk[d];
    l.wr[d] = W + off.lr[d];
    l.bias[d] = W + off.lb[d];
    l.dwk[d] = G + off.lk[d];
    l.dwr[d] = G + off.lr[d];
    l.dbias[d] = G + off.lb[d];
  }
}

// mask: moving_mean / moving_variance of the BatchNorm at offset bn (gamma, beta, mean, variance) are not trained
inline int freeze_bn(mmla_ctx* c, uint8_t* mask, size_t bn, int ch) {
  HIPCHK(c, hipMemsetAsync(mask + bn + 2 * ch, 0, 2 * (size_t)ch, c->stream));
  return MMLA_OK;
}

// mask [off.total]: trainable = all of the blob except the moving statistics of the nine units' BatchNorms
template <typename Off>
int mark_trainable(mmla_ctx* c, uint8_t* mask, const Off& off) {
  HIPCHK(c, hipMemsetAsync(mask, 1, off.total, c->stream));
  for (int i = 0; i < 9; ++i) {
    CHK(freeze_bn(c, mask, off.u[i].bn_in, off.u[i].cin));
    CHK(freeze_bn(c, mask, off.u[i].bn_mid, off.u[i].cout));
  }
  return MMLA_OK;
}

// ---- the fit driver ----------------------------------------------------------------------------------

enum { FIT_STOP = 1, FIT_CKPT = 2 };   // FitCall::callbacks

// one fit as its entry point was called, and what differs between the entries as values
struct FitCall {
  const char *who, *unit;   // "si_finetune", "windows"
  int slot;                 // the workspace slot of the engine and the staged operands
  int max_batch;            // samples per pass the engine takes
  int val_chunk;            // the validation set runs in chunks of min(n_val, val_chunk) at least
  int hist_w;               // floats per history row: loss, acc, val_loss, val_acc[, ...]
  // which Keras callbacks the entry has: EarlyStopping(val_loss, patience) and the epochs_run word;
  // ModelCheckpoint(val_acc, max, period) with best_out and the best_epoch word
  int callbacks;
  int n_classes;
  const char* label_set;    // check_labels' `set`
  bool dev;
  const float* packed;
  size_t n_floats;
  const void *x, *val_x;    // [n, row_bytes]
  size_t row_bytes;
  const int32_t *labels, *val_labels, *perm;
  int64_t n_train, n_val;
  int32_t epochs, batch, patience, ckpt_period;
  float *packed_out, *history, *best_out;
  int32_t *epochs_run, *best_epoch;
  // rows after an early stop: what writes NaN over the n floats of the history before the fit (null: nothing)
  hipError_t (*nan_fill)(float* hist, size_t n, hipStream_t s);

  int cap() const {   // samples per pass the engine is carved for
    return (int)std::max<int64_t>(std::min<int64_t>(batch, n_train), std::min<int64_t>(n_val, val_chunk));
  }
  bool stopping() const { return (callbacks & FIT_STOP) && patience > 0 && n_val > 0; }
  bool ckpt() const { return (callbacks & FIT_CKPT) && ckpt_period > 0 && n_val > 0; }
};

// the arguments every fit entry has; the entry adds its values and the callbacks' arguments
template <typename X>
FitCall fit_call(const char* who, const float* packed, int64_t n_floats, const X* x, const int32_t* labels,
                 int64_t n_train, const X* val_x, const int32_t* val_labels, int64_t n_val, int32_t epochs,
                 int32_t batch, const int32_t* perm, float* packed_out, float* history, uint32_t flags) {
  FitCall a{};
  a.who = who;
  a.dev = (flags & MMLA_DEVICE_PTR) != 0;
  a.packed = packed;
  a.n_floats = (size_t)n_floats;
  a.x = x;
  a.val_x = val_x;
  a.labels = labels;
  a.val_labels = val_labels;
  a.perm = perm;
  a.n_train = n_train;
  a.n_val = n_val;
  a.epochs = epochs;
  a.batch = batch;
  a.packed_out = packed_out;
  a.history = history;
  return a;
}

// device views of a fit's operands: the caller's pointers or the staged copies
struct FitBufs {
  float* blob = nullptr;   // the engine's copy of the blob (its carve sets it)
  const void *x = nullptr, *val_x = nullptr;
  const int32_t *labels = nullptr, *val_labels = nullptr, *perm = nullptr;
  float *hist = nullptr, *best = nullptr;

  int stage_in(const FitCall& a, Carver& cv, Stager& st) {
    const uint8_t *bx = nullptr, *bvx = nullptr;
    CHK(st.in(cv, static_cast<const uint8_t*>(a.x), (size_t)a.n_train * a.row_bytes, &bx));
    CHK(st.in(cv, a.labels, (size_t)a.n_train, &labels));
    CHK(st.in(cv, static_cast<const uint8_t*>(a.val_x), (size_t)a.n_val * a.row_bytes, &bvx));
    CHK(st.in(cv, a.val_labels, (size_t)a.n_val, &val_labels));
    CHK(st.in(cv, a.perm, (size_t)a.epochs * a.n_train, &perm));
    x = bx;
    val_x = bvx;
    return MMLA_OK;
  }
  void stage_out(const FitCall& a, Carver& cv, Stager& st) {
    hist = st.out(cv, a.history, (size_t)a.epochs * a.hist_w);
    best = st.out(cv, a.ckpt() ? a.best_out : nullptr, a.n_floats);
  }
};

// the size and null-pointer rules of every fit, then (host pointers) the labels and the permutations
inline int fit_check(mmla_ctx* c, const FitCall& a) {
  const char* who = a.who;
  if (a.batch < 1) return fail(c, MMLA_E_INVALID, "%s: batch %d < 1", who, a.batch);
  if (a.n_train < 1) return fail(c, MMLA_E_INVALID, "%s: n_train %lld < 1", who, (long long)a.n_train);
  if (a.n_val < 0 || a.epochs < 0 || a.patience < 0 || a.ckpt_period < 0 || a.n_train > (1 << 24) ||
      a.n_val > (1 << 24)) {
    std::string more;
    if (a.callbacks & FIT_STOP) more += ", patience " + std::to_string(a.patience);
    if (a.callbacks & FIT_CKPT) more += ", ckpt_period " + std::to_string(a.ckpt_period);
    return fail(c, MMLA_E_INVALID, "%s: bad sizes (n_val %lld, epochs %d%s)", who, (long long)a.n_val, a.epochs,
                more.c_str());
  }
  if (std::min<int64_t>(a.batch, a.n_train) > a.max_batch)
    return fail(c, MMLA_E_INVALID, "%s: a batch of more than %d %s", who, a.max_batch, a.unit);
  if (!a.packed || !a.x || !a.labels || !a.packed_out || ((a.callbacks & FIT_STOP) && !a.epochs_run) ||
      ((a.callbacks & FIT_CKPT) && !a.best_epoch) || (a.epochs > 0 && (!a.perm || !a.history)) ||
      (a.n_val > 0 && (!a.val_x || !a.val_labels)) || (a.epochs > 0 && a.ckpt() && !a.best_out))
    return fail(c, MMLA_E_INVALID, "%s: null pointer", who);
  if (a.dev) return MMLA_OK;
  CHK(check_labels(c, "labels", a.labels, a.n_train, a.n_classes, a.label_set));
  CHK(check_labels(c, "val_labels", a.val_labels, a.n_val, a.n_classes, a.label_set));
  return check_perm(c, who, a.perm, a.epochs, a.n_train);
}

// The whole fit of a checked call.  The entry's callables, all -> int:
//   carve(Carver&, Stager&, FitBufs&)   its engine (sets blob), then stage_in, stage_out and its own operands
//   begin()                             the optimiser's state, after the blob's upload
//   step(d, ep, order, b0, nb)          one training step on samples order[b0 .. b0 + nb) of epoch ep
//   validate(d, v0, nb)                 the forward of validation samples v0 .. v0 + nb
//   end_epoch(ep, row)                  the history row of epoch ep (device)
// Nothing here waits for the device unless a callback is live: then one history row is read back per epoch.
template <typename Carve, typename Begin, typename Step, typename Validate, typename EndEpoch>
int fit(mmla_ctx* c, const FitCall& a, Carve&& carve, Begin&& begin, Step&& step, Validate&& validate,
        EndEpoch&& end_epoch) {
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  Stager st{c, a.dev};
  const size_t wbytes = a.n_floats * sizeof(float);
  int ran = 0, best_ep = -1;
  auto word = [&](int32_t* p, int v) -> int {   // host or device words like every other output
    if (!p) return MMLA_OK;
    if (a.dev)
      HIPCHK(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p), v, 1, s));
    else
      *p = v;
    return MMLA_OK;
  };
  auto report = [&]() -> int {
    CHK(word(a.callbacks & FIT_STOP ? a.epochs_run : nullptr, ran));
    return word(a.callbacks & FIT_CKPT ? a.best_epoch : nullptr, best_ep);
  };
  if (a.epochs == 0) {   // the input blob, unchanged
    const bool same = a.packed_out == a.packed;
    if (!a.dev) {
      if (!same) std::memcpy(a.packed_out, a.packed, wbytes);
      return report();
    }
    if (same && !a.callbacks) return MMLA_OK;   // nothing was enqueued
    if (!same) HIPCHK(c, hipMemcpyAsync(a.packed_out, a.packed, wbytes, st.kind_in(), s));
    CHK(report());
    return finish(c, a.dev);
  }
  FitBufs d;
  CHK(carve_slot(c, a.slot, [&](Carver& cv) { return carve(cv, st, d); }));
  HIPCHK(c, hipMemcpyAsync(d.blob, a.packed, wbytes, st.kind_in(), s));
  CHK(begin());
  const size_t W = a.hist_w;
  if (a.nan_fill) HIPCHK(c, a.nan_fill(d.hist, (size_t)a.epochs * W, s));
  const bool stopping = a.stopping(), ckpt = a.ckpt();
  const int cap = a.cap();
  float best_loss = INFINITY, best_acc = -INFINITY;
  int wait = 0;
  for (int ep = 0; ep < a.epochs; ++ep) {
    const int32_t* order = d.perm + (size_t)ep * a.n_train;
    for (int64_t b0 = 0; b0 < a.n_train; b0 += a.batch)
      CHK(step(d, ep, order, (int)b0, (int)std::min<int64_t>(a.batch, a.n_train - b0)));
    for (int64_t v0 = 0; v0 < a.n_val; v0 += cap)
      CHK(validate(d, (int)v0, (int)std::min<int64_t>(cap, a.n_val - v0)));
    float* row = d.hist + ep * W;
    CHK(end_epoch(ep, row));
    ran = ep + 1;
    if (!stopping && !ckpt) continue;
    float hrow[8];
    HIPCHK(c, hipMemcpyAsync(hrow, row, W * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    // ModelCheckpoint(val_acc, save_best_only, mode 'max', period)
    if (ckpt && (ep + 1) % a.ckpt_period == 0 && hrow[3] > best_acc) {
      best_acc = hrow[3];
      best_ep = ep;
      HIPCHK(c, hipMemcpyAsync(d.best, d.blob, wbytes, hipMemcpyDeviceToDevice, s));
    }
    // EarlyStopping(val_loss, patience)
    if (!stopping) continue;
    if (hrow[2] < best_loss) {
      best_loss = hrow[2];
      wait = 0;
    } else if (++wait >= a.patience) {
      break;
    }
  }
  HIPCHK(c, hipMemcpyAsync(a.packed_out, d.blob, wbytes, st.kind_out(), s));
  CHK(st.back(a.history, d.hist, (size_t)a.epochs * W));
  if (best_ep >= 0) CHK(st.back(a.best_out, d.best, a.n_floats));
  CHK(report());
  return finish(c, a.dev);
}

}  // namespace mmla
