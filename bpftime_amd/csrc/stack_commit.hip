// bpftime_amd: k_stack_commit, the second half of bpf_get_stackid in a
// parallel batch (dev_helpers.hpp helper_stackid, DESIGN.md §6 "Stack traces").
//
// During the batch every call that met a slot empty before the batch lowered
// the slot's claim word to its serial-order key (common.hpp st_claim_key:
// global unit, the unit's call number, the call's skip).  The smallest key is
// the call the reference's serial run would have let fill the slot -- later
// calls keep what is there, whatever their length, since a parallel launch
// never carries BPF_F_REUSE_STACKID.  This kernel, queued behind the batch on
// its stream, stores that call's frames: one wave per slot, grid-stride over
// max_entries, two passes of 64 lanes over the (at most 127) frames.
//
//   claimed, not full   frames after the skip from the batch's stack arrays,
//                       zeros to value_size, nframes, full = 1, claim reset
//   claimed, full       claim reset only (a failed launch may have left one)
//   unclaimed           nothing
//
// No barrier: a wave owns its slot, and a slot's words are written by one
// instruction each after the loads they depend on.  Plain vector stores only.
#include <hip/hip_runtime.h>

#include "common.hpp"

namespace bpftime_amd {

constexpr uint32_t kCommitBlock = 256;

__global__ __launch_bounds__(kCommitBlock) void k_stack_commit(uint64_t data, uint32_t max_entries, uint32_t slot_size,
                                                               uint32_t cap, StackSrc src, uint64_t first_unit,
                                                               uint64_t count) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t waves = gridDim.x * (kCommitBlock / 64);
  for (uint32_t s = blockIdx.x * (kCommitBlock / 64) + threadIdx.x / 64; s < max_entries; s += waves) {
    const uint64_t slot = data + (uint64_t)s * slot_size;
    // (every lane reads the same two words: one line)
    const uint64_t claim = *(const volatile uint64_t *)slot;
    if (claim == kStNoClaim) continue;
    const uint32_t full = *(const volatile uint32_t *)(slot + 12);
    const uint64_t unit = (claim >> 16) - first_unit;
    // (a claim names a unit of this batch; one that does not is dropped)
    if (!full && src.arr && unit < count) {
      const uint32_t skip = (uint32_t)(claim & 0xff), depth = st_depth(src, unit);
      uint32_t n = depth > skip ? depth - skip : 0;
      n = n < cap ? n : cap;
      for (uint32_t k = lane; k < cap; k += 64)
        *(volatile uint64_t *)(slot + kStHdr + 8ull * k) = k < n ? st_frame(src, unit, skip + k) : 0;
      if (lane == 0) *(volatile uint64_t *)(slot + 8) = (uint64_t)n | 1ull << 32;
    }
    if (lane == 0) *(volatile uint64_t *)slot = kStNoClaim;
  }
}

}  // namespace bpftime_amd

using namespace bpftime_amd;

// Queues k_stack_commit for the STACK_TRACE map `m` behind the batch whose
// recorded stacks are `src` (units first_unit .. first_unit + count).
extern "C" hipError_t bpftime_amd_launch_stack_commit(const DMap *m, const StackSrc *src, uint64_t first_unit,
                                                      uint64_t count, hipStream_t stream) {
  if (!m || m->type != MT_STACK_TRACE || !m->max_entries) return hipErrorInvalidValue;
  const uint32_t per = kCommitBlock / 64;
  uint32_t grid = (m->max_entries + per - 1) / per;
  if (grid > 1024) grid = 1024;
  hipLaunchKernelGGL(k_stack_commit, dim3(grid), dim3(kCommitBlock), 0, stream, m->data, m->max_entries, m->slot_size,
                     m->value_size / 8, *src, first_unit, count);
  return hipGetLastError();
}
