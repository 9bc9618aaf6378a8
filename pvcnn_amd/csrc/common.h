// common.h -- shared host/device helpers of libpvcnn_hip.so (gfx950 only, wave64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "../../include/pvcnn_hip.h"
#include "switches.h"

namespace pvcnn {

constexpr int kWave = 64;                      // CDNA wavefront
constexpr int kLdsBytesPerCU = 160 * 1024;     // gfx950 LDS per CU (and max per workgroup)
constexpr int kNumCU = 256;                    // MI355X

// thread-local error string (api.hip)
void set_error(const char *fmt, ...);
// hipGetLastError() -> return code (+ error string); 0 when clean
int check_launch(const char *what);

__host__ __device__ inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
// log2(R) when R is a power of two >= 4 (grid rows can then be staged padded in LDS, slab.h), else 0
inline int grid_pad_shift(int R) { int s = 0; while ((1 << s) < R) ++s; return ((1 << s) == R && R >= 4) ? s : 0; }
__host__ __device__ inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// tables longer than this keep the separate reduce launch (one wave peeks a folded table: 64 words per step)
constexpr long kFoldTableMax = 1024;
// out[0] = max over out[1 .. T] of an amax buffer whose table has just been written on stream s (conv3d_bf16.hip)
int launch_amax_reduce(uint32_t *out, long T, hipStream_t s);

// One weight of a batched image refresh (pvcnn_conv3d_weight_split_pair_batch / pvcnn_pwconv_weight_split_pair_batch): ten int64 words
// in device memory, filled on the host by pvcnn_*_weight_split_pair_entry.  Workgroups [row_begin, row_begin + rows_f + rows_b) of the
// launch write this weight's forward and backward-data images, one (padded) output row each.
struct SplitEntry {
  const float *w;
  uint16_t *wts_f;
  int *wexp_f;
  uint16_t *wts_b;
  int *wexp_b;
  long long Co, Ci, rows_f, tm /* 1x1 only: TM_f | TM_b << 32 */, row_begin;
};
static_assert(sizeof(SplitEntry) == 80, "ten 8-byte words");

#ifdef __HIPCC__
// The entry that owns workgroup `blk` of a batched image refresh: a scan of the row_begin column (uniform scalar loads).
__device__ __forceinline__ SplitEntry split_entry_of(const SplitEntry *__restrict__ tab, int n, long long blk) {
  int i = 0;
  while (i + 1 < n && tab[i + 1].row_begin <= blk) ++i;
  return tab[i];
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also waits for every outstanding GLOBAL store of the
// wave (s_waitcnt vmcnt(0): its release fence), which serialises "store a tile, barrier, load the next one" loops on the
// full write latency; kernels whose global stores are never read back in the same launch use this instead, so the stores
// drain while the next phase runs.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// "Last workgroup done" WITHOUT fences.  VALIDATED ON gfx950 ONLY: what orders a published word before the ticket is that returning
// device-scope atomics are performed where all XCDs meet -- an observed property of this chip, not the HIP memory model's wording.  A workgroup PUBLISHES the few words the finalize step needs with returning device-scope
// atomics (publish32 / publish64: an exchange executes at the level where all XCDs meet and its return says it has), then takes a
// ticket; the workgroup that takes the last of `total` tickets reads the published words with device-scope atomic loads (peek32 /
// peek64: they do not hit in this XCD's L2) and finishes the job.  No __threadfence(): on gfx950 an agent-scope release fence writes
// back the XCD's whole L2 -- measured (profiles/ab/r05c_last_workgroup_fences.md): with one fence per workgroup the folded kernels of a
// PVCNN step (~100 k workgroups) cost 6.3 ms MORE than the ~26 launches of ~5 us they replaced.  *ticket must be 0 when the launch starts and is 0
// again when it ends (the last workgroup resets it: graph replays and later launches reuse the word).
// ticket_take: every workgroup, AFTER its published words have returned; contains __syncthreads(); true in every thread of exactly one
// workgroup.
__device__ __forceinline__ void publish32(uint32_t *p, uint32_t v) {
  const uint32_t old = atomicExch(p, v);
  asm volatile("" ::"v"(old) : "memory");                   // the exchange has returned (performed) before anything below is issued
}
__device__ __forceinline__ void publish64(unsigned long long *p, unsigned long long v) {
  const unsigned long long old = atomicExch(p, v);
  asm volatile("" ::"v"(old) : "memory");
}
__device__ __forceinline__ uint32_t peek32(const uint32_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long peek64(const unsigned long long *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// ticket_take_wave: the same for ONE wave of the workgroup (all 64 lanes call it, after their publishes have returned; the other waves
// have left: a workgroup of short-lived waves must not wait at a barrier for two atomic round trips -- measured, r05d)
__device__ __forceinline__ bool ticket_take_wave(unsigned *ticket, unsigned total) {
  unsigned t = 0u;
  if ((threadIdx.x & 63) == 0) {
    t = atomicAdd(ticket, 1u);
    if (t == total - 1u) atomicExch(ticket, 0u);
  }
  return (unsigned)__builtin_amdgcn_readfirstlane((int)t) == total - 1u;
}
__device__ __forceinline__ bool ticket_take(unsigned *ticket, unsigned total) {
  __shared__ int s_last_workgroup;
  __syncthreads();                                           // every thread's publishes have returned
  if (threadIdx.x == 0) {
    const unsigned t = atomicAdd(ticket, 1u);
    s_last_workgroup = (t == total - 1u) ? 1 : 0;
    if (t == total - 1u) atomicExch(ticket, 0u);
  }
  __syncthreads();
  return s_last_workgroup != 0;
}
#endif

}  // namespace pvcnn

// ---- phase clocks (tools/probe/: a SEPARATE build of a kernel's translation unit with -DPVCNN_PHASE_PROBE; the library itself never
// defines it, there these macros are nothing).  s_memtime per wave at named points of a kernel, the time since the previous point
// added to the slot's accumulator (scalar registers); at the end lane 0 of every wave adds its accumulators to
// pvcnn::phase_probe_buf[slot] and counts itself in slot 31.  A stamp waits for the wave's outstanding LDS / scalar loads
// (s_waitcnt lgkmcnt(0)): an instrumented kernel runs ~10 % slower than the real one; the SHARES are what is read.
#ifdef PVCNN_PHASE_PROBE
namespace pvcnn { static __device__ unsigned long long *phase_probe_buf = nullptr; }     // (one kernel translation unit per probe build)
#ifdef PVCNN_PHASE_PROBE_SETTER
extern "C" __attribute__((visibility("default"))) int pvcnn_probe_set_buffer(void *device_ptr) {
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(pvcnn::phase_probe_buf), &device_ptr, sizeof(device_ptr));
}
#endif
#define PVCNN_PROBE_BEGIN() unsigned long long probe_t_ = __builtin_amdgcn_s_memtime(); unsigned probe_acc_[16] = {}
#define PVCNN_PROBE(k) do { const unsigned long long probe_n_ = __builtin_amdgcn_s_memtime(); probe_acc_[k] += (unsigned)(probe_n_ - probe_t_); probe_t_ = probe_n_; } while (0)
#define PVCNN_PROBE_END()                                                                                              \
  do {                                                                                                                   \
    if ((threadIdx.x & 63) == 0 && pvcnn::phase_probe_buf != nullptr) {                                                  \
      for (int probe_k_ = 0; probe_k_ < 16; ++probe_k_) atomicAdd(pvcnn::phase_probe_buf + probe_k_, (unsigned long long)probe_acc_[probe_k_]); \
      atomicAdd(pvcnn::phase_probe_buf + 31, 1ull);                                                                      \
    }                                                                                                                    \
  } while (0)
#else
#define PVCNN_PROBE_BEGIN() do { } while (0)
#define PVCNN_PROBE(k) do { } while (0)
#define PVCNN_PROBE_END() do { } while (0)
#endif

#define PVCNN_REQUIRE(cond, msg)                                       \
  do {                                                                 \
    if (!(cond)) {                                                     \
      pvcnn::set_error("%s: %s", __func__, msg);                       \
      return PVCNN_ERR_INVALID_ARGUMENT;                               \
    }                                                                  \
  } while (0)

#define PVCNN_HIP_TRY(expr)                                            \
  do {                                                                 \
    hipError_t e_ = (expr);                                            \
    if (e_ != hipSuccess) {                                            \
      pvcnn::set_error("%s: %s failed: %s", __func__, #expr, hipGetErrorString(e_)); \
      return static_cast<int>(e_);                                     \
    }                                                                  \
  } while (0)
