// Host check of the launch plan (csrc/vm_plan.cpp plan_launch), linked alone:
// no GPU, no HIP runtime.  Occupancy is a model that depends only on LDS -- 0
// when a block's dynamic + static LDS exceeds the CU's, else CU / block capped
// at 8 -- with a static LDS and a CU count chosen here.  The expectations are
// the rules as DESIGN.md and the planner's comments state them, worked out
// here from common.hpp's sizes, never read back from the planner.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <string>

#include "../../bpftime_amd/csrc/vm_plan.hpp"

using namespace bpftime_amd;

static int g_failed = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);         \
      g_failed++;                                                 \
    }                                                             \
  } while (0)

static constexpr size_t kStatic = 8192;  // the model kernel's static LDS
static constexpr int kCus = 256;

static int occ_model(size_t dyn, bool, uint32_t) {
  const size_t need = dyn + kStatic;
  return need > kCuLds ? 0 : (int)std::min<size_t>(8, kCuLds / need);
}
static int cus_model() { return kCus; }

static const char *const kVars[] = {"BLOCK", "LCACHE_SETS", "COMB_ENTRIES", "TAIL_LDS", "GRID_MULT", "MAX_GRID", "LDS_REGS",
                                    "LDS_CTX", "NO_STAGING", "NO_RB_STAGE", "NO_MERGE", "MISS_LOG", "MISS_CAP", "DBG"};
// a launch with exactly these overrides ("NAME=value ...", separated by spaces)
static LaunchPlan plan(const PlanIn &in, const char *env = "") {
  for (const char *v : kVars) unsetenv((std::string("BPFTIME_AMD_") + v).c_str());
  std::string e = env;
  for (size_t at = 0; at < e.size();) {
    const size_t end = std::min(e.find(' ', at), e.size()), eq = e.find('=', at);
    setenv(("BPFTIME_AMD_" + e.substr(at, eq - at)).c_str(), e.substr(eq + 1, end - eq - 1).c_str(), 1);
    at = end + 1;
  }
  return plan_launch(in, occ_model, cus_model);
}

// a counter program on the raw ctx: a combining table, no lookup cache
static PlanIn counters(uint32_t hint, uint32_t stack = 8) {
  PlanIn in;
  in.kind = CTX_RAW;
  in.n = 1 << 20;
  in.stack_size = stack;
  in.comb_entries = kComb;
  in.comb_hint = hint;
  in.ncpu = 64;
  return in;
}
// flow-hash's shape: XDP, ctx only through data / data_end, table and lookup cache
static PlanIn flows(uint32_t hint, uint32_t stack, bool needs_ctx, uint32_t sets = kLcacheSets) {
  PlanIn in = counters(hint, stack);
  in.kind = CTX_XDP;
  in.needs_ctx = needs_ctx;
  in.lcache_sets = sets;
  return in;
}
// xdp-counter's shape: nothing in LDS but the lanes' ctx and stacks
static PlanIn plain(uint64_t n) {
  PlanIn in;
  in.kind = CTX_XDP;
  in.needs_ctx = true;
  in.n = n;
  in.stack_size = 8;
  in.ncpu = 64;
  return in;
}

static void table_entries() {
  // hint / 32 granules, a power of two in [2 * kComb, kCombMax]; 1024 unbounded
  CHECK(comb_entries_for_hint(0) == 512);
  CHECK(comb_entries_for_hint(32 * 512) == 512);
  CHECK(comb_entries_for_hint(32 * 512 + 1) == 1024);
  CHECK(comb_entries_for_hint(32 * 2048) == 2048);
  CHECK(comb_entries_for_hint(~0u) == 1024);
  CHECK(comb_entries_for_hint(32 * 8192) == kCombMax && comb_entries_for_hint(0x7fffffff) == kCombMax);
  // ... and a launch gets them (a table launch keeps its registers in global
  // memory and runs 1024-lane blocks)
  for (const uint32_t hint : {0u, 32u * 512, 32u * 512 + 1, ~0u}) {
    const LaunchPlan pl = plan(counters(hint));
    CHECK(pl.greg && pl.block == kBigBlock && pl.occupancy >= 1);
    CHECK(pl.comb_entries == (hint == 0 || hint == 32 * 512 ? 512u : 1024u));
  }
  // a 1024-lane block whose table wants 2048 entries or more takes the rest
  // of the CU's LDS, in steps of 32 entries down from kCombMax (64-B stacks)
  {
    const LaunchPlan pl = plan(counters(32 * 2048, 64));
    uint32_t most = kCombMax;
    while (most > 2048 && dyn_lds_for(CTX_RAW, false, 64, most, 0, true, kBigBlock) + kStatic > kCuLds) most -= 32;
    CHECK(pl.block == kBigBlock && pl.comb_entries == most && most > 2048 && most < kCombMax && pl.occupancy == 1);
  }
  // entries halve until a block fits: 256 lanes x 32 B, 3200 cache sets
  // (128000 B), constants and static leave 18336 B: 2048 entries (45056 B) and
  // 1024 (22528 B) do not fit, 512 (11264 B) do
  {
    const LaunchPlan pl = plan(flows(32 * 2048, 32, false, 3200), "LCACHE_SETS=3200");
    CHECK(comb_bytes(1024) == 22528 && comb_bytes(512) == 11264);
    CHECK(pl.block == kBlock && pl.lcache == 3200 && pl.comb_entries == 512 && pl.occupancy == 1);
  }
  // the override wins, rounded down to 8 ways
  CHECK(plan(counters(0), "COMB_ENTRIES=263").comb_entries == 256);
}

static void lookup_cache() {
  // doubled only in a 1024-lane block whose table wants fewer than 2048 entries
  CHECK(plan(flows(32 * 512, 32, false)).lcache == 2 * kLcacheSets);
  CHECK(plan(flows(32 * 512, 32, false)).block == kBigBlock);
  CHECK(plan(flows(32 * 2048, 32, false)).lcache == kLcacheSets);
  CHECK(plan(flows(32 * 512, 32, false), "BLOCK=256").lcache == kLcacheSets);
  CHECK(plan(flows(32 * 512, 32, false), "BLOCK=256").block == kBlock);
  CHECK(plan(flows(32 * 512, 32, false), "LCACHE_SETS=8").lcache == kLcacheSets);
  // dropped before the block falls back to 256 lanes: 1024 lanes x (48 B ctx +
  // 24 B stack) = 73728 B; with 2048 sets (81920 B), constants, the smallest
  // table (5632 B) and static that is 170592 B > 163840; with 1024 sets 129632
  {
    const LaunchPlan pl = plan(flows(32 * 512, 24, true));
    CHECK(!pl.gctx && pl.block == kBigBlock && pl.lcache == kLcacheSets && pl.occupancy >= 1);
  }
  // ... and 1024 lanes x (48 + 64) B = 114688 B do not fit with 1024 sets either
  {
    const LaunchPlan pl = plan(flows(32 * 512, 64, true));
    CHECK(pl.block == kBlock && pl.lcache == kLcacheSets && pl.greg && pl.occupancy >= 1);
  }
}

static void ordered() {
  for (PlanIn in : {counters(32 * 2048), flows(32 * 512, 32, false), plain(1 << 20)}) {
    in.ordered = true;
    const LaunchPlan pl = plan(in);
    CHECK(pl.ordered && pl.grid == 1 && pl.comb_entries == 0 && !pl.greg && !pl.gctx && pl.block == kBlock);
    CHECK(pl.step_cpu == 0 && pl.log_words == 0 && !pl.rb_stage);
  }
}

static void grid() {
  // 256 lanes x (48 + 8) B + constants + static = 23648 B: 6 blocks per CU
  const uint32_t occ = 6;
  CHECK(dyn_lds_for(CTX_XDP, false, 8, 0) + kStatic == 23648);
  LaunchPlan pl = plan(plain(1 << 20));
  CHECK(pl.block == kBlock && pl.occupancy == (int)occ && pl.grid == kCus * occ);  // the cap binds: 4096 wanted
  CHECK(plan(plain(1 << 20), "GRID_MULT=2").grid == 2 * kCus * occ);
  CHECK(plan(plain(1 << 20), "GRID_MULT=4").grid == 4096);  // the units bind
  CHECK(plan(plain(1 << 20), "MAX_GRID=5").grid == 5);
  CHECK(plan(plain(1000)).grid == 4 && plan(plain(1024)).grid == 4 && plan(plain(1025)).grid == 5);
  // images: one frame stack per lane of at most kTailGrid blocks
  {
    PlanIn in = plain(1 << 22);
    in.tail = true;
    pl = plan(in, "TAIL_LDS=0");
    CHECK(pl.image && pl.tail_lds == 0 && (uint64_t)kCus * pl.occupancy > kTailGrid && pl.grid == kTailGrid);
  }
  // the first 64 units are the head; the rest splits into whole grid steps
  // (full_q) and a remainder (full_r)
  struct {
    uint64_t n, q, r;
  } const splits[] = {{1, 0, 0}, {63, 0, 0}, {64, 0, 0}, {65, 0, 1}, {3 * 256 + 64, 1, 0}, {3 * 256 + 64 + 7, 1, 7}};
  for (const auto &s : splits) {
    pl = plan(plain(s.n), "MAX_GRID=3");
    CHECK(pl.grid == std::min<uint64_t>(3, (s.n + 255) / 256));
    CHECK(pl.full_q == s.q && pl.full_r == s.r);
  }
  // a flush log only past kMergeGroup blocks of tables
  CHECK(plan(counters(0)).log_words == log_words_for(512, kBigBlock));
  CHECK(plan(counters(0), "MAX_GRID=16").log_words == 0 && plan(counters(0), "NO_MERGE=1").log_words == 0);
}

static void lds_fit() {
  // flow-hash's override shape: 1024 lanes x 32 B, 2048 sets, 2000 entries
  // (44000 B): 159808 B + static > 163840; the smallest table would fit, so
  // the block stays at 1024 lanes and the launch is refused
  const LaunchPlan pl = plan(flows(32 * 2048, 32, false, 2048), "COMB_ENTRIES=2000 LCACHE_SETS=2048");
  CHECK(dyn_lds_for(CTX_XDP, false, 32, 2000, 2048, false, kBigBlock) == 159808);
  CHECK(pl.occupancy < 1 && pl.block == kBigBlock && pl.comb_entries == 2000 && pl.lcache == 2048 && pl.gctx);
}

int main() {
  table_entries();
  lookup_cache();
  ordered();
  grid();
  lds_fit();
  if (g_failed) return 1;
  printf("OK\n");
  return 0;
}
