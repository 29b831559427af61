// bpftime_amd: the launch plan of one exec_batch -- asm variant, block size,
// lookup-cache sets, combining-table entries, LDS tail-call depths, grid.
#include "vm_plan.hpp"

#include <stdlib.h>

#include <algorithm>
#include <map>
#include <mutex>

namespace bpftime_amd {

// Off by default: measured on one box (profiles/r06_ab_lane_pad.txt) the
// padding halves flow-hash's LDS bank conflicts but costs the lines LDS
// (residency, table reach, LDS tail-call frames): tail-call 1.186 -> 1.277
// ms, lpm-route 0.454 -> 0.471, flow-hash 0.670 -> 0.682, syscount equal
bool lane_pad() {
  static const bool on = getenv("BPFTIME_AMD_LANE_PAD") && atoi(getenv("BPFTIME_AMD_LANE_PAD")) != 0;
  return on;
}

namespace {
// The overrides of a launch, read on every launch (tests switch them inside
// one process)
struct PlanEnv {
  static uint32_t num(const char *name) {
    const char *e = getenv(name);
    return e ? (uint32_t)atoi(e) : 0;
  }
  static uint32_t pos(const char *name) {  // (a positive int, else 0)
    const char *e = getenv(name);
    return e && atoi(e) > 0 ? (uint32_t)atoi(e) : 0;
  }
  const bool block256 = getenv("BPFTIME_AMD_BLOCK") && atoi(getenv("BPFTIME_AMD_BLOCK")) == (int)kBlock;
  const bool lcache_set = getenv("BPFTIME_AMD_LCACHE_SETS") != nullptr;
  const bool comb_set = getenv("BPFTIME_AMD_COMB_ENTRIES") != nullptr;
  const uint32_t comb = num("BPFTIME_AMD_COMB_ENTRIES") & ~7u;
  // (at most that many depths in LDS; 0 = every frame in global memory)
  const uint32_t tail_most = getenv("BPFTIME_AMD_TAIL_LDS") ? std::min(num("BPFTIME_AMD_TAIL_LDS"), kTailLdsMax) : kTailLdsMax;
  const uint32_t grid_mult = pos("BPFTIME_AMD_GRID_MULT");
  const uint32_t max_grid = pos("BPFTIME_AMD_MAX_GRID");
  const bool lds_regs = getenv("BPFTIME_AMD_LDS_REGS") != nullptr;
  const bool lds_ctx = getenv("BPFTIME_AMD_LDS_CTX") != nullptr;
  const bool no_staging = getenv("BPFTIME_AMD_NO_STAGING") != nullptr;
  const bool no_rb_stage = getenv("BPFTIME_AMD_NO_RB_STAGE") != nullptr;
  const bool no_merge = getenv("BPFTIME_AMD_NO_MERGE") != nullptr;
  const bool miss_log = pos("BPFTIME_AMD_MISS_LOG") != 0;
  const char *const miss_cap = getenv("BPFTIME_AMD_MISS_CAP");  // (tests: overflow)
  const uint32_t dbg = getenv("BPFTIME_AMD_DBG") ? (uint32_t)strtoul(getenv("BPFTIME_AMD_DBG"), nullptr, 0) & ~kDbgXlat : 0;
};
}  // namespace

// The table's reach: a counter that finds no entry is a device atomic
// (memory-side, ~10 G/s chip-wide for scattered 8-byte adds), so the table
// should hold the hot part of the counter granules a block's adds can reach
// (the loader's hint), even at a block fewer per CU.  Measured with the
// register copy in global memory (k_interp G, one MI355X): flow-hash (65536
// flows) 512 entries at 3 blocks / CU 2.71 ms, 1024 at 3 1.71, 2048 at 2 1.34;
// syscall-agg (8192 ids) 256 at 4 1.40, 512 at 4 0.68, 1024 at 3 0.74;
// tail-call (per-CPU counters) 256 and 512 at 4 1.63, 1024 2.41.  So: hint /
// 32 granules, a power of two in [512, kCombMax] (1024 when the loader cannot
// bound the addresses)
uint32_t comb_entries_for_hint(uint32_t hint) {
  if (hint == ~0u) return 1024;
  uint32_t e = 2 * kComb;
  while (e < kCombMax && 32ull * e < hint) e *= 2;
  return e;
}

// The grid of a block shape that fits, the split of the units over it, and
// the logs behind the blocks' tables
static void plan_grid(const PlanIn &in, const PlanEnv &env, const CusFn &cus, LaunchPlan &pl) {
  pl.grid = 1;
  if (!in.ordered) {
    const uint64_t want_blocks = (in.n + pl.block - 1) / pl.block;
    // one wave per resident wave slot (x 1): every wave launch writes the
    // kernel's register spills (ScratchSize ~200 B / lane) once, and at x 4
    // those writes were 12 B of memory-side traffic per packet
    // (tools/grid_write_probe.sh, xdp-counter WRITE_SIZE 39.1 / 42.3 / 48.5 /
    // 61.0 B per packet at x 1 / 2 / 4 / 8; 0.467 / 0.479 / 0.496 / 0.484 ms;
    // lpm-route 0.467 / 0.479 / 0.506 ms at x 1 / 2 / 4); a combining table
    // is flushed once per block (flow-hash 0.60 -> 1.09 ms at x 4).  Ring
    // staging too, with an 8-KiB budget per block (common.hpp kRbStageRec;
    // ringbuf-sample 1.10 / 1.21 / 1.47 ms at x 1 / 2 / 4; with the 2-KiB
    // budget 7.46 / 4.03 / 1.43).  BPFTIME_AMD_GRID_MULT overrides.
    const uint32_t mult = env.grid_mult ? env.grid_mult : 1;
    const uint64_t cap = (uint64_t)cus() * (uint64_t)pl.occupancy * mult;
    pl.grid = (uint32_t)(want_blocks < cap ? want_blocks : cap);
    // (tests: few blocks, so that small batches take many units per lane)
    if (env.max_grid && pl.grid > env.max_grid) pl.grid = env.max_grid;
    if (in.tail && pl.grid > kTailGrid) pl.grid = kTailGrid;  // one frame stack per lane of the grid
  }
  const uint64_t ustep = (uint64_t)pl.grid * pl.block;
  pl.full_q = in.n >= 64 ? (in.n - 64) / ustep : 0;
  pl.full_r = in.n >= 64 ? (in.n - 64) % ustep : 0;
  pl.step_cpu = in.ordered ? 0 : (uint32_t)((ustep / 64) % (in.ncpu ? in.ncpu : 1));
  // a block-end flush log when the blocks hold per-lane counter tables:
  // merged by a second launch instead of every block adding its table
  if (pl.comb_entries && pl.grid > kMergeGroup && !env.no_merge) pl.log_words = log_words_for(pl.comb_entries, pl.block);
  // the combining tables' miss log (common.hpp kMissParts): records per
  // block and partition for a quarter of the block's units missing with a
  // pair each, at most 256 MiB of log.  Opt-in (BPFTIME_AMD_MISS_LOG=1):
  // measured on flow-hash, the interpreter kernel gains 0.06 ms per 2^24
  // frames (0.89 -> 0.83) but k_miss_merge costs 0.18 ms -- the misses of
  // moderately hot flows reach one merge block from every source block and
  // serialize on its LDS atomics -- so by default misses add directly
  if (pl.comb_entries && pl.grid > 1 && env.miss_log) {
    const uint64_t upb = (in.n + pl.grid - 1) / pl.grid;
    uint64_t cap = upb * 2 / 4 / kMissParts;
    const uint64_t most = (256ull << 20) / ((uint64_t)pl.grid * kMissParts * 16);
    cap = cap < 16 ? 16 : cap;
    cap = cap > most ? most : cap;
    if (env.miss_cap) cap = strtoull(env.miss_cap, nullptr, 0);
    cap &= ~1ull;
    if (cap >= 2) pl.miss_cap = (uint32_t)cap;
  }
}

LaunchPlan plan_launch(const PlanIn &in, const OccFn &occ, const CusFn &cus) {
  const PlanEnv env;
  const uint32_t kind = in.kind;
  LaunchPlan pl{};
  pl.ordered = in.ordered;
  pl.dbg = env.dbg;
  // staged window: what the static packet / slot accesses need, when every
  // slot is 16-B aligned and at least that long (a window never reaches into
  // the next unit)
  pl.stage = in.stage_need && in.aligned && !env.no_staging ? in.stage_need : 0;
  pl.lcache = in.lcache_sets;  // (sized below)
  // ORDERED: every counter add goes straight to memory (link_fast), no table
  pl.comb_entries = in.ordered ? 0 : in.comb_entries;
  // launches holding a combining table or lookup cache keep the C++ tier's
  // register copy in global memory (k_interp G): their units stay in the asm
  // tier, and the LDS goes to resident blocks (latency-bound: more waves
  // hide the packet and probe loads)
  pl.greg = !in.ordered && !in.big_stack && (pl.comb_entries || pl.lcache) && !env.lds_regs;
  // ... and an XDP program that reads its ctx only through the specialised
  // data / data_end loads (the loader's escape analysis) keeps the ctx there
  // too: only the C++ tier reads it (48 B of LDS per lane)
  pl.gctx = pl.greg && kind == CTX_XDP && !in.needs_ctx && !in.tail && !env.lds_ctx;
  pl.rb_stage = in.rings && !in.ordered && !env.no_rb_stage;
  // G launches without a tail-call image or ring staging run kBigBlock-lane
  // blocks (common.hpp): one table and lookup cache per 16 waves
  // (BPFTIME_AMD_BLOCK=256 keeps 4-wave blocks)
  pl.block = pl.greg && !in.tail && !pl.rb_stage && !env.block256 ? kBigBlock : kBlock;
  pl.image = in.tail && !in.big_stack;  // (bpftime_amd_launch_interp)
  // the lookup cache: 1024 sets, or 2048 in a 1024-lane block whose
  // combining table would stay below 2048 entries (the LDS is there:
  // syscall-agg 0.645 -> 0.61 ms; flow-hash, whose table fills the CU, is
  // best at 1024: 2048 sets 1.08 ms, 512 0.93, 1024 0.89)
  const uint32_t want = in.comb_entries ? comb_entries_for_hint(in.comb_hint) : 0;
  if (pl.lcache && pl.block == kBigBlock && want < 2048 && !env.lcache_set) pl.lcache = 2 * kLcacheSets;
  // a 1024-lane block must fit the CU with the smallest table it may get
  // (lanes' ctx and stacks, lookup cache, launch constants): drop the
  // doubled lookup cache first, then fall back to 256-lane blocks
  if (pl.block == kBigBlock) {
    const uint32_t e_min = in.comb_entries ? kComb : 0;
    auto fits = [&](uint32_t lc) {
      return occ(dyn_lds_for(kind, in.big_stack, in.stack_size, e_min, lc, !pl.gctx, kBigBlock), pl.greg, kBigBlock) >= 1;
    };
    if (!fits(pl.lcache) && pl.lcache > kLcacheSets && !env.lcache_set) pl.lcache = kLcacheSets;
    if (!fits(pl.lcache)) {
      pl.block = kBlock;
      if (!env.lcache_set) pl.lcache = in.lcache_sets;
    }
  }
  // resident blocks with `e` table entries and the LDS frames `tail_lds`
  auto dyn_of = [&](uint32_t e, uint32_t tail_lds) {
    return dyn_lds_for(kind, in.big_stack, in.stack_size, e, pl.lcache, !pl.gctx, pl.block, tail_lds);
  };
  auto occ_of = [&](uint32_t e, uint32_t tail_lds) { return occ(dyn_of(e, tail_lds), pl.greg, pl.block); };
  if (pl.comb_entries) {
    uint32_t e = want;
    // (a block must still fit the CU's LDS beside the lanes' ctx and stacks;
    // the sets may be any count, gen_fast.py comb_add.  Measured: trading
    // reach for a resident block does not pay -- flow-hash 2048 entries at 2
    // blocks / CU 1.32 ms, 1792 at 3 1.57, 1536 at 3 1.42 -- nor does reach
    // beyond hint / 32 at the same residency: flow-hash 3072 1.29,
    // syscall-agg 768 / 984 0.672 / 0.677 against 512 0.664)
    while (e > kComb && occ_of(e, 0) < 1) e /= 2;
    // one 1024-lane block per CU: a table that wants 2048 entries or more
    // takes the rest of the CU's LDS (multiples of 8 ways), since every
    // counter it misses is a memory-side atomic.  Measured (flow-hash, one
    // MI355X, same box): 2048 entries 1.027 ms, 2560 0.980, 3072 0.945,
    // 3584 0.914, 3840 0.898, 4032 0.891
    if (pl.block == kBigBlock && e >= 2048) {
      static std::mutex fill_mu;
      static std::map<size_t, uint32_t> fill;  // (dyn_of(0), ctx kind) -> the largest table that fits
      std::lock_guard<std::mutex> g(fill_mu);
      const size_t key = dyn_of(0, 0) * 4 + kind;
      auto it = fill.find(key);
      if (it == fill.end()) {
        uint32_t f = kCombMax;
        while (f > e && occ_of(f, 0) < 1) f -= 32;
        it = fill.emplace(key, f).first;
      }
      e = it->second > e ? it->second : e;
    }
    // (an override that does not fit the CU fails the batch, named)
    if (env.comb_set) e = env.comb;
    pl.comb_entries = e;
  }
  // XDP images: the asm tier's frames of the first depths in LDS, as many
  // depths (kTailLdsMax at most) as keep the block's residency
  if (pl.image && kind == CTX_XDP && !(pl.dbg & 8)) {
    const uint32_t sw = in.stack_size / 8;
    const uint32_t words = 1 + in.tail_max_live + (uint32_t)__builtin_popcount(in.tail_ctx_mask & 0x3f) +
                           (uint32_t)__builtin_popcount(in.tail_stack_mask & (sw >= 16 ? 0xffffu : (1u << sw) - 1));
    const uint32_t most = env.tail_most;
    const int occ0 = occ_of(pl.comb_entries, 0);
    auto depths = [&](uint32_t e) -> uint32_t {
      for (uint32_t dl = most; dl >= 1 && occ0 >= 1; dl--)
        if (occ_of(e, dl | words << 8) >= occ0) return dl;
      return 0;
    };
    uint32_t dl = depths(pl.comb_entries);
    // a combining table above the size its counters need (the loader's hint:
    // kComb entries hold them) gives way to a deeper LDS frame stack
    if (dl < most && pl.comb_entries > kComb && 32ull * kComb >= in.comb_hint && !env.comb_set) {
      const uint32_t dl2 = depths(kComb);
      if (dl2 > dl) {
        dl = dl2;
        pl.comb_entries = kComb;
      }
    }
    pl.tail_lds = dl ? dl | words << 8 : 0;
  }
  // every block of the launch must fit the CU's LDS (env overrides of the
  // table / cache sizes included): a launch that needs more fails, named
  // (vm_upkeep.cpp lds_fit_error), instead of running at an occupancy of zero
  pl.occupancy = occ_of(pl.comb_entries, pl.tail_lds);
  if (pl.occupancy < 1) return pl;
  plan_grid(in, env, cus, pl);
  return pl;
}

void LaunchPlan::into(KParams &p) const {
  p.stage = stage;
  p.lcache = lcache;
  p.comb_entries = comb_entries;
  p.tail_lds = tail_lds;
  p.full_q = full_q;
  p.full_r = full_r;
  p.step_cpu = step_cpu;
  p.log_words = log_words;
  p.miss_cap = miss_cap;
  p.dbg = dbg;
}

}  // namespace bpftime_amd
