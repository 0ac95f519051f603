// libmmla context: errors, the per-stage profiler, the workspace slots, and the entry points that
// create, configure and inspect a context.  See include/mmla.h for the contract.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>

#include "internal.h"

using namespace mmla;

namespace mmla __attribute__((visibility("hidden"))) {

int fail(mmla_ctx* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (c) c->err = buf;
  return code;
}

// ---- tracing: hipEvents around each launch when enabled ---------------------------------------
static hipEvent_t prof_event(mmla_ctx* c) {
  if (!c->prof_pool.empty()) {
    hipEvent_t e = c->prof_pool.back();
    c->prof_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}

int prof_begin(mmla_ctx* c, int stage) {
  if (!c->prof_on) return -1;
  ProfRec r{stage, prof_event(c), prof_event(c), 0.0};
  (void)hipEventRecord(r.a, c->stream);
  c->prof_pending.push_back(r);
  return (int)c->prof_pending.size() - 1;
}

void prof_end(mmla_ctx* c, int idx, double work) {
  if (idx < 0) return;
  ProfRec& r = c->prof_pending[idx];
  r.work = work;
  (void)hipEventRecord(r.b, c->stream);
}

int prof_collect(mmla_ctx* c) {
  for (ProfRec& r : c->prof_pending) {
    HIPCHK(c, hipEventSynchronize(r.b));
    float ms = 0.0f;
    HIPCHK(c, hipEventElapsedTime(&ms, r.a, r.b));
    c->prof_ms[r.stage] += ms;
    c->prof_work[r.stage] += r.work;
    c->prof_n[r.stage] += 1;
    c->prof_pool.push_back(r.a);
    c->prof_pool.push_back(r.b);
  }
  c->prof_pending.clear();
  return MMLA_OK;
}

// growable device workspace slots
// Debug aid: with MMLA_WS_GUARD=1 in the environment each slot allocated from then on is framed by
// 4 MiB guard bands filled with kGuardByte, and finish() fails the call if a kernel wrote into one
// (out-of-bounds stores that would otherwise land silently in a neighbouring allocation).
constexpr size_t kGuardBytes = 4u << 20;
constexpr int kGuardByte = 0xA5;

int ws_get(mmla_ctx* c, int slot, size_t bytes, void** out) {
  const bool kept = slot_kept(slot);
  if (kept && bytes < 256) bytes = 256;
  if ((int)c->ws.size() <= slot) {
    c->ws.resize(slot + 1, nullptr);
    c->ws_size.resize(slot + 1, 0);
    c->ws_guard.resize(slot + 1, 0);
  }
  const char* ge = std::getenv("MMLA_WS_GUARD");
  const size_t guard = ge && ge[0] == '1' ? kGuardBytes : 0;
  // guarded slots are re-framed whenever the size changes, so the trailing band always sits right
  // behind the live tensor (not behind the largest one ever requested)
  if (c->ws_size[slot] < bytes || (guard && c->ws_size[slot] != bytes)) {
    if (c->ws[slot]) {
      HIPCHK(c, hipStreamSynchronize(c->stream));
      HIPCHK(c, hipFree(static_cast<char*>(c->ws[slot]) - c->ws_guard[slot]));
      c->ws[slot] = nullptr;
      c->ws_size[slot] = 0;
    }
    void* p = nullptr;
    if (c->debug_fail_allocs > 0 && !kept) {   // the hook: a workspace allocation inside a micro-batch
      --c->debug_fail_allocs;
      return fail(c, MMLA_E_OOM, "workspace slot %d: injected allocation failure (MMLA_DEBUG_FAIL_ALLOC)", slot);
    }
    if (hipMalloc(&p, bytes + 2 * guard) != hipSuccess) {
      (void)hipGetLastError();   // clear the sticky allocation error
      return fail(c, MMLA_E_OOM, "hipMalloc(%zu) failed for workspace slot %d", bytes, slot);
    }
    if (guard) {   // on the context stream: ordered before the kernels that follow
      HIPCHK(c, hipMemsetAsync(p, kGuardByte, guard, c->stream));
      HIPCHK(c, hipMemsetAsync(static_cast<char*>(p) + guard + bytes, kGuardByte, guard, c->stream));
    }
    // Debug aid: MMLA_WS_POISON=<byte> fills every new slot with that byte (0xff: float NaN), so a
    // kernel that reads workspace memory no earlier launch wrote shows up in its results
    const char* pe = std::getenv("MMLA_WS_POISON");
    if (pe && pe[0])
      HIPCHK(c, hipMemsetAsync(static_cast<char*>(p) + guard, (int)std::strtol(pe, nullptr, 0) & 255,
                               bytes, c->stream));
    c->ws[slot] = static_cast<char*>(p) + guard;
    c->ws_size[slot] = bytes;
    c->ws_guard[slot] = guard;
  }
  *out = c->ws[slot];
  return MMLA_OK;
}

int ws_release(mmla_ctx* c, bool kept_too) {
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < c->ws.size(); ++i)
    if (c->ws[i] && (kept_too || !slot_kept((int)i))) {
      HIPCHK(c, hipFree(static_cast<char*>(c->ws[i]) - c->ws_guard[i]));
      c->ws[i] = nullptr;
      c->ws_size[i] = 0;
      c->ws_guard[i] = 0;
    }
  return MMLA_OK;
}

static int ws_check_guards(mmla_ctx* c) {
  std::vector<unsigned char> h(kGuardBytes);
  for (size_t slot = 0; slot < c->ws.size(); ++slot) {
    const size_t g = c->ws_guard[slot];
    if (!c->ws[slot] || !g) continue;
    for (int side = 0; side < 2; ++side) {
      const char* d = static_cast<const char*>(c->ws[slot]) + (side ? c->ws_size[slot] : -(ptrdiff_t)g);
      HIPCHK(c, hipMemcpy(h.data(), d, g, hipMemcpyDeviceToHost));
      for (size_t i = 0; i < g; ++i)
        if (h[i] != kGuardByte)
          return fail(c, MMLA_E_HIP, "workspace slot %zu: %s guard overwritten at byte %zu", slot,
                      side ? "trailing" : "leading", side ? i : g - i);
    }
  }
  return MMLA_OK;
}

int finish(mmla_ctx* c, bool dev) {
  HIPCHK(c, hipGetLastError());
  bool guarded = false;
  for (size_t g : c->ws_guard) guarded |= g != 0;
  if (!dev || guarded) HIPCHK(c, hipStreamSynchronize(c->stream));
  if (guarded) return ws_check_guards(c);
  return MMLA_OK;
}

// device bytes per clip of one micro-batch (workspace slots of run_od_net / run_si_net + FE I/O)
constexpr double kOdBytesPerClip = 3.0 * 128 * 151 * 32 * 4 + 128 * 151 * 3 + 128 * 151 * 4 +
                                   19 * 128 * 4 + 512 * 4 + 64;
constexpr double kSiBytesPerClip = 4.0 * 256 * 32 * 4 + 256 * 39 * 4 + 8 * 128 * 4 + 512 * 4 +
                                   1024 * 4 + 64;

// clips per micro-batch: the user's cap, else what the device's free memory holds (the slots this
// context already owns and a retry would free, so not the kept ones, count as free), capped at the default
int64_t microbatch(mmla_ctx* c, bool od) {
  const int64_t user = od ? c->od_mb : c->si_mb;
  if (user > 0) return user;
  const int64_t cap = od ? c->od_mb_cap : c->si_mb_cap;
  size_t fr = 0, tot = 0;
  if (hipMemGetInfo(&fr, &tot) != hipSuccess) {
    (void)hipGetLastError();
    return cap;
  }
  double held = 0;
  for (size_t i = 0; i < c->ws_size.size(); ++i)
    if (!slot_kept((int)i)) held += (double)c->ws_size[i];
  int64_t fit = (int64_t)(((double)fr + held) * 0.9 / (od ? kOdBytesPerClip : kSiBytesPerClip));
  fit = fit / kMinMicrobatch * kMinMicrobatch;
  return std::max(kMinMicrobatch, std::min(cap, fit));
}

}  // namespace mmla

// the MMLA_* switches read at create (mmla_ctx documents each)
struct EnvSwitch {
  const char* name;
  bool mmla_ctx::*no;   // inverted boolean (1 turns the member off), or
  int mmla_ctx::*num;   // integer
};
static const EnvSwitch kEnvSwitches[] = {
    {"MMLA_DEBUG_FAIL_ALLOC", nullptr, &mmla_ctx::debug_fail_allocs},
    {"MMLA_NO_SIU", &mmla_ctx::siu, nullptr},
    {"MMLA_NO_SIPU", &mmla_ctx::sipu, nullptr},
    {"MMLA_NO_SIFIN", &mmla_ctx::sifin, nullptr},
    {"MMLA_NO_SIPAIR", &mmla_ctx::sipair, nullptr},
    {"MMLA_NO_SICHAIN", &mmla_ctx::sichain, nullptr},
    {"MMLA_NO_LSTM_SPLIT", &mmla_ctx::lstm_split, nullptr},
    {"MMLA_LSTM_SPLIT_MAX", nullptr, &mmla_ctx::lstm_split_max},
    {"MMLA_DEBUG_LSTM_SPIN", nullptr, &mmla_ctx::lstm_spin},
    {"MMLA_DEBUG_TRACE_GUARD", nullptr, &mmla_ctx::debug_trace_guard},
    {"MMLA_NO_SIPAD", &mmla_ctx::si_pad_feat, nullptr},
    {"MMLA_NO_ODU", &mmla_ctx::odu, nullptr},
    {"MMLA_NO_ODW", &mmla_ctx::odw, nullptr},
    {"MMLA_NO_VADW", &mmla_ctx::vadw, nullptr},
    {"MMLA_VADW", nullptr, &mmla_ctx::vadw_all},
    {"MMLA_RB_TILE", &mmla_ctx::rbs, nullptr},   // 1 selects the tiles: the strips off
    {"MMLA_NO_RBS_W1L", &mmla_ctx::rbs_w1l, nullptr},
    {"MMLA_NO_RBS_TAILPAIR", &mmla_ctx::rbs_tailpair, nullptr},
    {"MMLA_NO_PIN_OUT", &mmla_ctx::pin_small, nullptr},   // takes effect where create makes the pinned buffers
};

extern "C" {

int mmla_abi_version(void) { return MMLA_ABI_VERSION; }

int mmla_create(int device, mmla_ctx** out) {
  if (!out) return MMLA_E_INVALID;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return MMLA_E_HIP;
  if (device < 0 || device >= ndev) return MMLA_E_INVALID;
  if (hipSetDevice(device) != hipSuccess) return MMLA_E_HIP;
  mmla_ctx* c = new mmla_ctx();
  c->device = device;
  for (const EnvSwitch& s : kEnvSwitches)
    if (const char* v = std::getenv(s.name)) {
      if (s.no) c->*s.no = std::atoi(v) == 0;
      else c->*s.num = std::atoi(v);
    }
  // a BLOCKING stream: it orders with the legacy default (NULL) stream, on which PyTorch's default
  // stream enqueues -- so a device-pointer call sees tensors a torch kernel or copy just produced
  // without an explicit synchronisation (a non-blocking stream raced them: a 65 536-clip call read
  // the last clips before torch had written them)
  if (hipStreamCreateWithFlags(&c->own_stream, hipStreamDefault) != hipSuccess) {
    delete c;
    return MMLA_E_HIP;
  }
  c->stream = c->own_stream;
  if (hipMalloc(&c->range_dev, RW_COUNT * sizeof(int)) != hipSuccess ||
      hipMemset(c->range_dev, 0, RW_COUNT * sizeof(int)) != hipSuccess ||
      hipHostMalloc(&c->range_host, 2 * sizeof(int), hipHostMallocDefault) != hipSuccess) {
    mmla_destroy(c);
    return MMLA_E_HIP;
  }
  if (c->pin_small) {
    const unsigned fl = hipHostMallocMapped | hipHostMallocCoherent;
    if (hipHostMalloc(reinterpret_cast<void**>(&c->range_map), 64, fl) != hipSuccess ||
        hipHostGetDevicePointer(reinterpret_cast<void**>(&c->range_map_dev), c->range_map, 0) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(&c->pin_out), kPinSlots * kPinSlotBytes, fl) != hipSuccess ||
        hipHostGetDevicePointer(reinterpret_cast<void**>(&c->pin_out_dev), c->pin_out, 0) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(&c->pin_in), kPinInBytes, hipHostMallocDefault) != hipSuccess) {
      mmla_destroy(c);
      return MMLA_E_HIP;
    }
    c->range_map[0] = c->range_map[1] = 0;
  }
  OdFeTables ot;
  od_fe_build_tables(&ot);
  if (!od_fe_tables_ok(ot)) {   // the mel schedule exceeds the front-end kernel's LDS rows / fragments
    mmla_destroy(c);
    return MMLA_E_INVALID;
  }
  SiFeTables st;
  si_fe_build_tables(&st);
  if (!si_fe_tables_ok(st)) {   // filterbank segments exceed the front-end kernel's unrolled loops
    mmla_destroy(c);
    return MMLA_E_INVALID;
  }
  if (hipMalloc(&c->od_tables, sizeof(OdFeTables)) != hipSuccess ||
      hipMalloc(&c->si_tables, sizeof(SiFeTables)) != hipSuccess ||
      hipMemcpy(c->od_tables, &ot, sizeof(ot), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(c->si_tables, &st, sizeof(st), hipMemcpyHostToDevice) != hipSuccess) {
    mmla_destroy(c);
    return MMLA_E_HIP;
  }
  *out = c;
  return MMLA_OK;
}

int mmla_destroy(mmla_ctx* c) {
  if (!c) return MMLA_E_INVALID;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  free_allocs(c->od_allocs);
  free_allocs(c->si_allocs);
  free_allocs(c->si_head_allocs);
  for (size_t i = 0; i < c->ws.size(); ++i)
    if (c->ws[i]) (void)hipFree(static_cast<char*>(c->ws[i]) - c->ws_guard[i]);
  if (c->od_tables) (void)hipFree(c->od_tables);
  if (c->si_tables) (void)hipFree(c->si_tables);
  if (c->nr_tables) (void)hipFree(c->nr_tables);
  if (c->nr_thresh) (void)hipFree(c->nr_thresh);
  if (c->range_dev) (void)hipFree(c->range_dev);
  if (c->vad_state) (void)hipFree(c->vad_state);
  if (c->cap_state) (void)hipFree(c->cap_state);
  if (c->range_host) (void)hipHostFree(c->range_host);
  if (c->range_map) (void)hipHostFree(c->range_map);
  if (c->pin_out) (void)hipHostFree(c->pin_out);
  if (c->pin_in) (void)hipHostFree(c->pin_in);
  (void)prof_collect(c);
  for (hipEvent_t e : c->prof_pool) (void)hipEventDestroy(e);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  delete c;
  return MMLA_OK;
}

const char* mmla_last_error(const mmla_ctx* c) { return c ? c->err.c_str() : "null context"; }

int mmla_set_stream(mmla_ctx* c, void* s) {
  if (!c) return MMLA_E_INVALID;
  hipStream_t ns = s ? static_cast<hipStream_t>(s) : c->own_stream;
  if (ns != c->stream) {
    // work already enqueued on the old stream still reads and writes this context's workspaces:
    // the new stream waits for it before the next call reuses them
    HIPCHK(c, hipSetDevice(c->device));
    hipEvent_t e = nullptr;
    HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    const hipError_t r1 = hipEventRecord(e, c->stream);
    const hipError_t r2 = r1 == hipSuccess ? hipStreamWaitEvent(ns, e, 0) : r1;
    (void)hipEventDestroy(e);
    HIPCHK(c, r2);
  }
  c->stream = ns;
  return MMLA_OK;
}

int mmla_range_check(mmla_ctx* c, int64_t* f32_reruns) {
  if (!c) return MMLA_E_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (f32_reruns) *f32_reruns = c->range_reruns;
  int flag = 0, timeout = 0;
  HIPCHK(c, hipMemcpy(&flag, c->range_dev + RW_DEV_RANGE, sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(&timeout, c->range_dev + RW_DEV_TIMEOUT, sizeof(int), hipMemcpyDeviceToHost));
  if (timeout) {
    HIPCHK(c, hipMemset(c->range_dev + RW_DEV_TIMEOUT, 0, sizeof(int)));
    return fail(c, MMLA_E_HIP,
                "a device-pointer call since the last check ran the split BiLSTM and one of its "
                "workgroups timed out waiting for the others: its probabilities are NaN; re-run it");
  }
  if (flag) {
    HIPCHK(c, hipMemset(c->range_dev + RW_DEV_RANGE, 0, sizeof(int)));
    return fail(c, MMLA_E_RANGE,
                "a device-pointer call since the last check split an operand outside the fp16 "
                "range (|x| >= 65504): its results are not valid; re-run it with MMLA_PREC_F32");
  }
  return MMLA_OK;
}

int mmla_debug_counters(mmla_ctx* c, int64_t* f32_reruns, int64_t* lstm_split_reruns) {
  if (!c) return MMLA_E_INVALID;
  if (f32_reruns) *f32_reruns = c->range_reruns;
  if (lstm_split_reruns) *lstm_split_reruns = c->lstm_split_reruns;
  return MMLA_OK;
}

int mmla_synchronize(mmla_ctx* c) { return mmla_range_check(c, nullptr); }

int mmla_get_microbatch(mmla_ctx* c, int64_t* od_clips, int64_t* si_clips) {
  if (!c) return MMLA_E_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  if (od_clips) *od_clips = microbatch(c, true);
  if (si_clips) *si_clips = microbatch(c, false);
  return MMLA_OK;
}

int mmla_release_workspace(mmla_ctx* c) {
  if (!c) return MMLA_E_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  return ws_release(c, true);   // the kept slots too; the capture and detector states stay
}

int mmla_set_precision(mmla_ctx* c, int mode) {
  if (!c || (mode != MMLA_PREC_F32 && mode != MMLA_PREC_F16X3)) return MMLA_E_INVALID;
  c->precision = mode;
  return MMLA_OK;
}

int mmla_set_microbatch(mmla_ctx* c, int64_t od, int64_t si) {
  if (!c || od < 0 || si < 0) return MMLA_E_INVALID;
  c->od_mb = od;   // 0 = sized from free memory (mmla.h)
  c->si_mb = si;
  c->od_mb_cap = kOdMicrobatch;
  c->si_mb_cap = kSiMicrobatch;
  return MMLA_OK;
}

int mmla_debug_ws_slot(mmla_ctx* c, int slot, void** ptr, size_t* bytes) {
  if (!c || !ptr || !bytes || slot < 0) return MMLA_E_INVALID;
  const bool have = slot < (int)c->ws.size() && c->ws[slot];
  *ptr = have ? c->ws[slot] : nullptr;
  *bytes = have ? c->ws_size[slot] : 0;
  return MMLA_OK;
}

int mmla_profile_enable(mmla_ctx* c, int on) {
  if (!c) return MMLA_E_INVALID;
  c->prof_on = on != 0;
  return MMLA_OK;
}

int mmla_profile_read(mmla_ctx* c, double* ms, int64_t* launches, double* work, int reset) {
  if (!c) return MMLA_E_INVALID;
  CHK(prof_collect(c));
  for (int i = 0; i < MMLA_NSTAGES; ++i) {
    if (ms) ms[i] = c->prof_ms[i];
    if (launches) launches[i] = c->prof_n[i];
    if (work) work[i] = c->prof_work[i];
    if (reset) {
      c->prof_ms[i] = 0.0;
      c->prof_n[i] = 0;
      c->prof_work[i] = 0.0;
    }
  }
  return MMLA_OK;
}

}  // extern "C"
