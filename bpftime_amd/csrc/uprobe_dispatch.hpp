// bpftime_amd: what uprobe_dispatch.cpp hands its kernels (uprobe_dispatch.hip).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace bpftime_amd {

// A gathered row: the record's pt_regs (21 u64), its caller's pid_tgid, the
// clock of the attachment's phase, the record's index -- 24 u64, 192 B
constexpr uint32_t kRegsWords = 21, kRowWords = 24, kRowBytes = 8 * kRowWords;
constexpr uint32_t kRowPidOff = 168, kRowClockOff = 176, kRowIndexWord = 23;

// One attachment's gather over the recorded calls.  Records are taken in
// chunks of 64 (a wave each); chunk c's matches go to rows [offsets[c],
// offsets[c + 1]) in record order.
struct UGather {
  const uint64_t *regs;   // n x 21 u64: the phase's pt_regs
  const uint64_t *func;   // n: the called function
  const uint64_t *pid;    // n, or null: pid_default
  const uint64_t *clock;  // n x {entry ns, return ns}, or null: 0 (the batch reads the device clock)
  uint64_t pid_default;
  uint64_t target;        // the attachment's function
  uint64_t n;
  uint32_t phase;         // 0: the entry clock, 1: the return clock
  uint32_t chunks;        // ceil(n / 64)
  uint32_t *counts;       // [chunks]: matches per chunk, then (k_ug_scan) their exclusive prefix sums
  uint32_t *total;        // every match
  // k_ug_gather's outputs: `cap` rows (= *total as the host read it; nothing
  // is written past them, whatever `func` holds by then)
  uint64_t *rows;
  uint64_t cap;
  // the recorded stacks (include/ebpf-vm.h ebpf_batch::stack_*), or null arr;
  // out: a row of max_depth frames per match (zero past its depth) and its
  // clamped depth
  const uint8_t *stack_arr;
  uint64_t stack_unit_stride, stack_frame_stride;
  const uint32_t *stack_depths;
  uint32_t stack_fixed_depth, stack_max_depth;
  uint64_t *stack_rows;
  uint32_t *stack_depths_out;
};

}  // namespace bpftime_amd

extern "C" {
// counts the matches per chunk and in all (g.counts, g.total; total zeroed
// here) and turns the counts into offsets
hipError_t bpftime_amd_launch_ug_count(const bpftime_amd::UGather *g, hipStream_t stream);
hipError_t bpftime_amd_launch_ug_gather(const bpftime_amd::UGather *g, hipStream_t stream);
// override kinds: row j's state / value back to its record (rows' index word).
// replace: the value is the program's r0 (`vals`, always set); else vals[j]
// where state[j] bit 0 is set
hipError_t bpftime_amd_launch_ug_scatter(const uint64_t *rows, uint64_t m, uint64_t n, const uint32_t *state,
                                         const int64_t *vals, int replace, uint32_t *out_state, int64_t *out_rets,
                                         hipStream_t stream);
// The event list (bpftime_amd_uprobe_dispatch_events), n words (record << 1) |
// phase.  _event_keys: keys[e] = pid[record of events[e]] for the thread
// grouping (null keys: none are written) and *bad = the events whose record is
// not below nrec (zeroed here; such an event gets key 0 and is not
// dereferenced).  _event_words: the grouping's perm, indexes into the list,
// rewritten in place to the event words
hipError_t bpftime_amd_launch_ug_event_keys(const uint32_t *events, uint64_t n, const uint64_t *pid, uint64_t nrec,
                                            uint64_t *keys, uint32_t *bad, hipStream_t stream);
hipError_t bpftime_amd_launch_ug_event_words(uint32_t *perm, const uint32_t *events, uint64_t n, hipStream_t stream);
}
