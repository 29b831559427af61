// bpftime_amd: the launch plan of one exec_batch (vm_plan.cpp plan_launch).
// Host arithmetic only: it needs neither the HIP runtime nor the registry, so
// tests/cpp/launch_plan_test.cpp links vm_plan.cpp alone.
#pragma once
#include <functional>

#include "common.hpp"

namespace bpftime_amd {

// What the plan depends on: the batch, the program form it launches, the maps
// that exist.
struct PlanIn {
  uint32_t kind = CTX_RAW;  // CTX_* the kernel runs
  bool ordered = false;     // EBPF_BATCH_ORDERED
  uint64_t n = 0;           // units
  bool big_stack = false;
  uint32_t stack_size = 0;
  uint32_t comb_entries = 0;    // LoadOut::comb_entries (0: no deferred counter adds)
  uint32_t comb_hint = 0;       // FastForm::comb_hint (~0u: unbounded)
  uint32_t lcache_sets = 0;     // the form's lookup cache: lcache_sets(), 0 without one
  bool needs_ctx = false;       // an XDP form that reads its ctx beyond data / data_end
  bool tail = false;            // a tail-call image
  uint32_t tail_max_live = 0, tail_ctx_mask = 0, tail_stack_mask = 0;  // FastForm's frame layout
  bool rings = false;           // ring-buffer maps exist
  uint32_t stage_need = 0;      // loader.hpp stage_need of the form
  bool aligned = false;         // ... and whether the units allow a staged window
  uint32_t ncpu = 0;
};

// The shape of the launch.  plan_launch is the only writer.
struct LaunchPlan {
  bool ordered, greg, gctx, image, rb_stage;
  uint32_t block, lcache, comb_entries, tail_lds, stage, grid;
  int occupancy;  // resident blocks per CU; < 1: the block does not fit the CU's LDS (nothing past tail_lds is set)
  uint64_t full_q, full_r;
  uint32_t step_cpu;
  uint32_t log_words;  // the block-end flush log (0: none)
  uint32_t miss_cap;   // the opt-in miss log's records per block and partition (0: none)
  uint32_t dbg;
  // its fields of the kernel's parameters
  void into(KParams &p) const;
};

// resident blocks per CU of a block with `dyn_lds` bytes of dynamic LDS (< 1:
// it does not fit), and the device's CUs
using OccFn = std::function<int(size_t dyn_lds, bool greg, uint32_t block)>;
using CusFn = std::function<int()>;

// Combining-table entries for the loader's hint: hint / 32 granules, a power
// of two in [2 * kComb, kCombMax]; 1024 when the loader cannot bound the
// addresses
uint32_t comb_entries_for_hint(uint32_t hint);

LaunchPlan plan_launch(const PlanIn &in, const OccFn &occ, const CusFn &cus);

}  // namespace bpftime_amd
