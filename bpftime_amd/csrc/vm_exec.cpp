// bpftime_amd: ebpf_exec_batch as a sequence of stages -- check the batch,
// pick the image, fill the kernel's parameters, plan the launch (vm_plan.cpp),
// bind the per-stream buffers, run the map upkeep (vm_upkeep.cpp) and queue
// the kernels -- and ebpf_exec on top of it.
#include "vm_impl.hpp"
#include "vm_plan.hpp"

namespace bpftime_amd {
// experiment counters (BPFTIME_AMD_DBG 512), a device buffer made on first use
static std::mutex g_dbg_mu;
static uint64_t *g_dbg = nullptr;  // lookup-cache hit / miss lanes (gen_fast.py lcache_count)
uint64_t *dbg_counts() {
  std::lock_guard<std::mutex> g(g_dbg_mu);
  if (!g_dbg && (hipMalloc((void **)&g_dbg, 8 * kDbgCounts) != hipSuccess ||
                 hipMemset(g_dbg, 0, 8 * kDbgCounts) != hipSuccess))
    g_dbg = nullptr;
  return g_dbg;
}

namespace {
// what a batch's ctx kind and flags say
struct BatchFacts {
  uint32_t kind = CTX_RAW;  // the kernel's ctx kind
  bool uprobe = false, sys_exit = false, ordered = false;
  // the initial data offset inside each slot.  A descriptor names its frame's
  // first byte itself, so descriptor batches have none: ebpf_batch::head is not
  // used there (include/ebpf-vm.h)
  uint32_t head = 0;
};

// Every refusal that depends on the ebpf_batch alone ("": none), and the facts
std::string check_batch(const ebpf_batch *b, BatchFacts &f) {
  if (!b || b->ctx_kind > EBPF_CTX_UPROBE || (b->count && !b->data) || (b->count && !b->stride && !b->descs))
    return "invalid batch";
  // the uprobe ctx runs on the raw kernel: the unit is a pt_regs (r2 = 168),
  // and the recorded caller / clock and the override state apply as they do
  // to the syscall kinds (EBPF_CTX_UPROBE, include/ebpf-vm.h)
  const bool uprobe = f.uprobe = b->ctx_kind == EBPF_CTX_UPROBE;
  if (uprobe && (b->descs || (b->count && (b->stride < kPtRegsBytes || b->stride % 8 != 0 ||
                                            (uintptr_t)b->data % 8 != 0))))
    return "an uprobe batch needs 8-aligned units of at least " + std::to_string(kPtRegsBytes) +
           " bytes (struct pt_regs) at a stride that is a multiple of 8, and no descriptors";
  // the sys_exit ctx runs on the syscall kernel: only r2 (the ctx size) and
  // the window differ (EBPF_CTX_SYSCALL_EXIT, include/ebpf-vm.h)
  const bool sys_exit = f.sys_exit = b->ctx_kind == EBPF_CTX_SYSCALL_EXIT;
  const uint32_t kind = f.kind = sys_exit ? CTX_SYSCALL : uprobe ? CTX_RAW : b->ctx_kind;
  f.ordered = (b->flags & EBPF_BATCH_ORDERED) != 0;
  f.head = b->descs ? 0 : b->head;
  if (b->sys_state && ((kind != CTX_SYSCALL && !uprobe) || (b->sys_phase != 1 && b->sys_phase != 2)))
    return uprobe ? "sys_state needs sys_phase 1 (enter) or 2 (exit)"
                  : "sys_state needs a syscall batch with sys_phase 1 (enter) or 2 (exit)";
  if (b->descs && (kind == CTX_SYSCALL || !b->umem_bytes))
    return "descriptor batches need an XDP / raw ctx and umem_bytes";
  // the recorded caller / clock (include/ebpf-vm.h): syscall kinds only; an
  // offset 8-aligned with the u64 inside the unit (the kernel
  // reads it for any nonzero value, in both tiers), or an array with an
  // 8-aligned stride, not both
  const uint64_t extent = sys_exit && b->stride >= 96 ? b->stride - 64 : b->stride;
  struct R {
    const char *name;
    int32_t off;
    const void *arr;
    uint64_t stride;
  };
  for (const R &o : {R{"pid_tgid", b->pid_tgid_off, b->pid_tgid_arr, b->pid_tgid_stride},
                     R{"ktime", b->ktime_off, b->ktime_arr, b->ktime_stride}}) {
    if (!o.off && !o.arr) continue;
    std::string bad;
    if ((kind != CTX_SYSCALL && !uprobe) || b->descs)
      bad = uprobe ? "not with descriptors" : "a syscall batch only";
    else if (o.off && o.arr)
      bad = "an offset or an array, not both";
    else if (o.off && (o.off < 0 || o.off % 8 != 0 || (uint64_t)o.off + 8 > extent))
      bad = "the u64 inside the unit (8-aligned, off + 8 <= " + std::to_string(extent) + ")";
    else if (o.arr && (o.stride == 0 || o.stride % 8 != 0 || (uintptr_t)o.arr % 8 != 0))
      bad = "an 8-aligned array with a nonzero stride that is a multiple of 8";
    if (!bad.empty()) return std::string(o.name) + (o.arr ? "_arr" : "_off " + std::to_string(o.off)) + ": " + bad;
  }
  // the recorded call stacks (include/ebpf-vm.h): any ctx kind
  if (b->stack_arr) {
    if ((uintptr_t)b->stack_arr % 8 != 0) return "stack_arr: an 8-aligned array";
    if (b->stack_unit_stride == 0 || b->stack_unit_stride % 8 != 0)
      return "stack_unit_stride " + std::to_string(b->stack_unit_stride) + ": a nonzero multiple of 8";
    if (b->stack_frame_stride == 0 || b->stack_frame_stride % 8 != 0)
      return "stack_frame_stride " + std::to_string(b->stack_frame_stride) + ": a nonzero multiple of 8";
    if ((uintptr_t)b->stack_depths % 4 != 0) return "stack_depths: a 4-aligned array";
    if (b->stack_max_depth < 1 || b->stack_max_depth > kStMaxDepth)
      return "stack_max_depth " + std::to_string(b->stack_max_depth) + ": 1.." + std::to_string(kStMaxDepth);
  }
  return "";
}

// The image a batch launches (a tail-calling program's is relinked first when
// a prog array moved), checked against the maps its program names
struct Launchee {
  std::shared_ptr<Image> im;
  std::vector<int32_t> st_commit;  // the STACK_TRACE maps k_stack_commit visits behind the launch
  int32_t unwind_helper = -1;      // the unwind helper as the device knows helpers (bpftime ids)
};
bool pick_image(Mi355xVm &vm, const ebpf_batch *b, const BatchFacts &f, Launchee &l) {
  {
    std::lock_guard<std::mutex> g(vm.img_mu);
    if (vm.has_tail && vm.link_tail_image_locked() < 0) return false;
    l.im = vm.img;
  }
  if (!l.im) {
    vm.error = "no program loaded";
    return false;
  }
  const Image &im = *l.im;
  const FastForm &ff = f.kind == CTX_XDP ? im.fx : im.fr;
  // ARRAY_OF_MAPS: the inner maps the slots name, before anything is queued
  if (!inner_launch_check(ff, vm.error)) return false;
  if (!perf_launch_prepare(im.prog, vm.error)) return false;
  // STACK_TRACE maps: what a parallel batch may do to one
  {
    std::lock_guard<std::mutex> g(rt().mu);
    if (!st_launch_check(ff, f.ordered, b->stack_arr ? b->stack_max_depth : 0, vm.error, l.st_commit)) return false;
  }
  // (the registration that was given ubpf id unwind_idx)
  for (const auto &kv : vm.helper_id_map)
    if ((int)kv.second == vm.unwind_idx) l.unwind_helper = (int32_t)kv.first;
  if (l.unwind_helper == (int)kTailHelper && im.d_tail_entry) {
    vm.error = "an unwind index on bpf_tail_call is not supported on the device";
    return false;
  }
  return true;
}

// The straight copies from the batch, the runtime and the VM
void fill_params(Mi355xVm &vm, const ebpf_batch *b, const BatchFacts &f, const Launchee &l, KParams &p) {
  Runtime &r = rt();
  const Image &im = *l.im;
  const uint32_t kind = f.kind;
  p.prog = im.d_prog;
  p.needs_ctx = kind == CTX_XDP && im.fx.needs_ctx ? 1 : 0;
  p.fast_div = getenv("BPFTIME_AMD_NO_ASM_DIVERGENCE") ? 0 : 1;
  p.maps = r.d_maptab;
  p.data = (uint8_t *)b->data;
  p.lens = kind == CTX_SYSCALL || f.uprobe ? nullptr : b->lens;
  p.verdicts = b->verdicts;
  p.rets = b->rets;
  p.out_data_off = b->data_off_out;
  p.out_len = b->len_out;
  p.err_count = vm.d_err + (vm.err_slot.fetch_add(1) % Mi355xVm::kErrSlots);
  p.n = b->count;
  p.stride = b->stride;
  p.first_unit = b->first_unit;
  p.data_lo = (uint64_t)(uintptr_t)b->data;
  // (a sys_exit unit is 24 B inside its record: the window ends with the
  // last record's exit half, 32 B of a 96-B record)
  p.data_hi = p.data_lo + (b->descs     ? b->umem_bytes
                           : f.sys_exit ? (b->count - 1) * b->stride + (b->stride < 32 ? b->stride : 32)
                                        : b->count * b->stride);
  p.descs = (const uint64_t *)b->descs;
  p.umem_bytes = b->umem_bytes;
  p.sys_nr = (b->flags & EBPF_BATCH_SYS_NR) && kind == CTX_SYSCALL ? b->sys_nr : -1;
  p.sys_state = b->sys_state;
  p.sys_ret = b->sys_ret;
  p.sys_phase = b->sys_phase;
  p.pid_off = b->pid_tgid_off;
  if (b->pid_tgid_off) {
    p.pid_base = (const uint8_t *)b->data + b->pid_tgid_off;
    p.pid_stride = b->stride;
  } else if (b->pid_tgid_arr) {
    p.pid_base = (const uint8_t *)b->pid_tgid_arr;
    p.pid_stride = b->pid_tgid_stride;
  }
  if (b->ktime_off) {
    p.kt_base = (const uint8_t *)b->data + b->ktime_off;
    p.kt_stride = b->stride;
  } else if (b->ktime_arr) {
    p.kt_base = (const uint8_t *)b->ktime_arr;
    p.kt_stride = b->ktime_stride;
  }
  if (b->stack_arr)
    p.stacks = StackSrc{(const uint8_t *)b->stack_arr, b->stack_unit_stride, b->stack_frame_stride, b->stack_depths,
                        b->stack_fixed_depth, b->stack_max_depth};
  p.pid_tgid = ((uint64_t)(uint32_t)getpid() << 32) | (uint32_t)syscall(SYS_gettid);
  vm.task_into(p.task_uid_gid, p.task_comm);
  vm.attach_into(p.attach_func_ip, p.attach_cookie);
  p.trace_log = trace_log().d;  // (made at load when the program calls helper 6)
  p.trace_cap = trace_log().cap;
  p.arena_lo = (uint64_t)(uintptr_t)r.arena;
  p.arena_hi = p.arena_lo + r.arena_size;
  p.step_limit = vm.step_limit;
  // (syscall kinds: r2 = sizeof the ctx, syscall_trace_attach_impl.cpp:46)
  // (uprobe: sizeof(struct pt_regs), frida_attach_entry.hpp:54-55)
  p.fixed_len = f.uprobe ? kPtRegsBytes : kind != CTX_SYSCALL ? b->fixed_len : f.sys_exit ? 24 : 64;
  p.stack_size = im.prog.stack_size;
  p.stack_stride = lane_stride(im.prog.stack_size);
  p.ctx_stride = lane_stride(kXdpCtxBytes);
  p.ncpu = r.ncpu;
  p.unwind_idx = l.unwind_helper;
  p.ifindex = b->ingress_ifindex;
  p.rxq = b->rx_queue_index;
  p.head = f.head;
  p.checked = (b->flags & EBPF_BATCH_UNCHECKED) ? 0 : 1;
  if (im.d_tail_entry) {
    p.tail_entry = im.d_tail_entry;
    p.tail_slots = im.d_tail_slots;
    p.frame_words = im.frame_words;
    p.tail_ctx_mask = im.fx.tail_ctx_mask;
    p.tail_stack_mask = im.fx.tail_stack_mask;
  }
}

// which map types exist (they decide buffers, not programs)
struct MapKinds {
  bool prog_arrays = false, rings = false;
};
MapKinds map_kinds() {
  Runtime &r = rt();
  MapKinds k;
  for (uint32_t fd = 0; fd < kMaxFds; fd++)
    if (r.kind[fd] == HKind::MAP) {
      k.prog_arrays |= r.maps[fd].type == MT_PROG_ARRAY;
      k.rings |= r.maps[fd].type == MT_RINGBUF;
    }
  return k;
}

PlanIn plan_in(const ebpf_batch *b, const BatchFacts &f, const Image &im, bool rings) {
  const bool xdp = f.kind == CTX_XDP;
  const FastForm &ff = xdp ? im.fx : im.fr;
  PlanIn in;
  in.kind = f.kind;
  in.ordered = f.ordered;
  in.n = b->count;
  in.big_stack = im.prog.big_stack;
  in.stack_size = im.prog.stack_size;
  in.comb_entries = im.prog.comb_entries;
  in.comb_hint = ff.comb_hint;
  in.lcache_sets = ff.needs_lcache ? lcache_sets() : 0;
  in.needs_ctx = xdp && im.fx.needs_ctx;
  in.tail = im.d_tail_entry != nullptr;
  in.tail_max_live = im.fx.tail_max_live;
  in.tail_ctx_mask = im.fx.tail_ctx_mask;
  in.tail_stack_mask = im.fx.tail_stack_mask;
  in.rings = rings;
  in.stage_need = stage_need(ff, xdp ? f.head : 0);
  // (descriptor batches: the kernel checks each wave's frames)
  in.aligned = ((uint64_t)(uintptr_t)b->data % 16) == 0 &&
               (b->descs ? true : (b->stride % 16) == 0 && b->stride >= in.stage_need);
  in.ncpu = rt().ncpu;
  return in;
}

int device_cus() {
  static int cus = 0;
  if (!cus) {
    hipDeviceProp_t prop;
    int dev = 0;
    hipGetDevice(&dev);
    hipGetDeviceProperties(&prop, dev);
    cus = prop.multiProcessorCount;
  }
  return cus;
}

// The launch's device buffers, one set per stream: concurrent batches never
// share them
bool bind_buffers(Mi355xVm &vm, const LaunchPlan &pl, const Image &im, bool prog_arrays, hipStream_t s, KParams &p) {
  const uint32_t grid = pl.grid, block = pl.block;
  if (pl.greg) {
    p.gregs = (uint64_t *)vm.regs.get(s, (uint64_t)grid * 11 * block * 8);
    if (!p.gregs) {
      vm.error = "register copy allocation failed";
      return false;
    }
  }
  if (im.d_tail_entry) {
    // tail-call frames for the lanes of this launch ([depth][word][lane])
    const uint64_t fbytes = (uint64_t)grid * kBlock * kTailDepth * im.frame_words * 8;
    p.frames = (uint8_t *)vm.frames.get(s, fbytes);
    if (!p.frames) {
      vm.error = "tail-call frame allocation failed (" + std::to_string(fbytes >> 20) + " MiB)";
      return false;
    }
  }
  // a scratch word per lane while prog arrays exist (device map_lookup_elem
  // on one hands out a copy of the fd there, prog_array.cpp:113-143), after
  // them the blocks' ring-buffer staging areas while ring buffers exist
  // (dev_helpers.hpp RbStage; not in ORDERED batches: exact order), then the
  // lanes' global XDP ctx (gctx)
  if (prog_arrays || pl.rb_stage || pl.gctx) {
    const uint64_t words = (uint64_t)grid * block * 8, sbytes = pl.rb_stage ? (uint64_t)grid * kRbStageBytes : 0;
    uint8_t *base = (uint8_t *)vm.scratch.get(s, words + sbytes + (pl.gctx ? 48ull * grid * block : 0));
    if (!base) {
      vm.error = "lane scratch allocation failed";
      return false;
    }
    p.lane_scratch = (uint64_t *)base;
    p.rb_stage = pl.rb_stage ? base + words : nullptr;
    p.gctx = pl.gctx ? base + words + sbytes : nullptr;
  }
  if (pl.log_words) {
    p.flush_log = (uint64_t *)vm.logs.get(s, (uint64_t)grid * pl.log_words * 8);
    if (!p.flush_log) {
      vm.error = "flush log allocation failed";
      return false;
    }
  }
  if (pl.miss_cap) {
    // (the counts, then a u32 of records the merge refused: a log that
    // names an address outside the windows is never added)
    const uint64_t cbytes = ((uint64_t)grid * kMissParts * 4 + 4 + 255) & ~255ull;
    uint8_t *m = (uint8_t *)vm.misses.get(s, cbytes + (uint64_t)grid * kMissParts * pl.miss_cap * 16);
    if (!m) {
      vm.error = "miss log allocation failed";
      return false;
    }
    p.miss_counts = (uint32_t *)m;
    if (hipMemsetAsync(m + (uint64_t)grid * kMissParts * 4, 0, 4, s) != hipSuccess) {
      vm.error = "miss log reset failed";
      return false;
    }
    p.miss_log = (uint64_t *)(m + cbytes);
  }
  return true;
}

// bpftime_amd_vm_last_launch and the BPFTIME_AMD_VERBOSE line: the plan and
// the buffers it got
void report_launch(Mi355xVm &vm, const LaunchPlan &pl, const KParams &p) {
  bpftime_amd_launch_info li{};
  li.units = p.n;
  li.grid = pl.grid;
  li.block = pl.block;
  li.comb_entries = pl.comb_entries;
  li.lcache_sets = pl.lcache;
  li.stage = pl.stage;
  li.gregs = p.gregs ? 1 : 0;
  li.gctx = p.gctx ? 1 : 0;
  li.miss_cap = pl.miss_cap;
  li.tail_lds_depths = pl.tail_lds & 0xff;
  li.tail_lds_words = pl.tail_lds >> 8;
  li.occupancy = pl.occupancy;
  li.flush_log = p.flush_log ? 1 : 0;
  li.miss_log = p.miss_log ? 1 : 0;
  li.ordered = pl.ordered ? 1 : 0;
  if (getenv("BPFTIME_AMD_VERBOSE"))
    fprintf(stderr,
            "bpftime_amd: launch units %llu grid %u block %u comb %u lcache %u stage %u stack %u gregs %d gctx %d unwind %d "
            "miss cap %u tail lds %u x %u words occ %d\n",
            (unsigned long long)li.units, li.grid, li.block, li.comb_entries, li.lcache_sets, li.stage,
            (unsigned)p.stack_size, (int)li.gregs, (int)li.gctx, p.unwind_idx, li.miss_cap, li.tail_lds_depths,
            li.tail_lds_words, li.occupancy);
  std::lock_guard<std::mutex> g(vm.last_mu);
  vm.last = li;
}

// k_interp, then what merges or commits behind it, between the timing events
// of an EBPF_BATCH_TIMED batch (the host work before -- linking, buffers,
// index upkeep -- stays outside)
bool queue_kernels(Mi355xVm &vm, const ebpf_batch *b, const BatchFacts &f, const Launchee &l, const LaunchPlan &pl,
                   const KParams &p, hipStream_t s) {
  const bool timed = (b->flags & EBPF_BATCH_TIMED) != 0;
  if (timed) {
    if ((!vm.ev_t0 && hipEventCreate(&vm.ev_t0) != hipSuccess) ||
        (!vm.ev_t1 && hipEventCreate(&vm.ev_t1) != hipSuccess) || hipEventRecord(vm.ev_t0, s) != hipSuccess) {
      vm.error = "timing event failed";
      return false;
    }
  }
  const uint32_t grid = pl.grid;
  hipError_t e = bpftime_amd_launch_interp(&p, f.kind, l.im->prog.big_stack, grid, f.ordered ? 1 : 0, pl.block, s);
  // (BPFTIME_AMD_SYNC_EACH: synchronize after every launch, naming the one that failed)
  const bool sync_each = getenv("BPFTIME_AMD_SYNC_EACH") != nullptr;
  auto step = [&](const char *what, hipError_t le) {
    if (le == hipSuccess && sync_each) le = hipStreamSynchronize(s);
    if (le != hipSuccess && sync_each) fprintf(stderr, "bpftime_amd: %s: %s\n", what, hipGetErrorString(le));
    return le;
  };
  e = step("k_interp", e);
  if (e == hipSuccess && p.flush_log) e = step("k_comb_merge", bpftime_amd_launch_merge(p.flush_log, p.log_words, grid, s));
  if (e == hipSuccess && p.miss_log)
    e = step("k_miss_merge", bpftime_amd_launch_miss_merge(p.miss_log, p.miss_counts, p.miss_cap, grid, &p,
                                                           p.miss_counts + (uint64_t)grid * kMissParts, s));
  if (e == hipSuccess && p.miss_log && sync_each) {
    uint32_t bad = 0;
    hipMemcpy(&bad, p.miss_counts + (uint64_t)grid * kMissParts, 4, hipMemcpyDeviceToHost);
    if (bad) fprintf(stderr, "bpftime_amd: k_miss_merge: %u records outside the windows\n", bad);
  }
  // a parallel batch's bpf_get_stackid claims become stored stacks (without
  // a stack source no call claims anything)
  if (p.stacks.arr)
    for (const int32_t fd : l.st_commit) {
      if (e != hipSuccess) break;
      DMap dm;
      {
        std::lock_guard<std::mutex> g(rt().mu);
        dm = rt().maps[fd].d;
      }
      e = step("k_stack_commit", bpftime_amd_launch_stack_commit(&dm, &p.stacks, b->first_unit, b->count, s));
    }
  if (e == hipSuccess && timed) e = hipEventRecord(vm.ev_t1, s);
  if (e != hipSuccess) {
    vm.error = std::string("kernel launch failed: ") + hipGetErrorString(e);
    return false;
  }
  return true;
}
}  // namespace

int Mi355xVm::exec_batch(const ebpf_batch *b) {
  if (!loaded) {
    error = "no program loaded";
    return -1;
  }
  BatchFacts f;
  const std::string bad = check_batch(b, f);
  if (!bad.empty()) {
    error = bad;
    return -1;
  }
  hipStream_t s = (hipStream_t)b->stream;
  if (b->count == 0) return 0;
  Launchee l;
  if (!pick_image(*this, b, f, l)) return -1;
  Image &im = *l.im;
  const LoadOut &prog = im.prog;
  const bool xdp = f.kind == CTX_XDP;
  const FastForm &ff = xdp ? im.fx : im.fr;
  KParams p{};
  fill_params(*this, b, f, l, p);

  const MapKinds maps = map_kinds();
  const PlanIn in = plan_in(b, f, im, maps.rings);
  const LaunchPlan pl = plan_launch(
      in,
      [&in](size_t dyn, bool greg, uint32_t block) {
        return bpftime_amd_occupancy(in.kind, in.big_stack, dyn, greg, block, in.tail && !in.big_stack);
      },
      device_cus);
  p.fast = im.linked(pl.greg, xdp, xdp ? f.head : 0, pl.stage, f.ordered, l.unwind_helper, pl.lcache, b->pid_tgid_off);
  if (!p.fast) {
    error = "device upload failed";
    return -1;
  }
  if (pl.occupancy < 1) {
    error = lds_fit_error(f.kind, prog.big_stack, prog.stack_size, pl.comb_entries, pl.lcache, !pl.gctx, pl.greg, pl.block,
                          pl.image, pl.tail_lds);
    return -1;
  }
  pl.into(p);
  if (p.dbg & 512) p.dbg_counts = dbg_counts();
  {
    const hipError_t me = hipMemsetAsync(p.err_count, 0, 4, s);
    if (me != hipSuccess) {
      error = std::string("hipMemsetAsync failed: ") + hipGetErrorString(me) +
              " (an earlier operation on this stream or device may have failed)";
      return -1;
    }
  }

  LaunchUpkeep upkeep(f.ordered);
  upkeep.lcache = pl.lcache;
  if (!upkeep.add(prog, ff)) {
    error = upkeep.err;
    return -1;
  }
  // QUEUE / STACK maps: one kind of access per map in a parallel launch
  if (!qs_launch_check(ff, f.ordered, error, upkeep.qs_adds, upkeep.qs_takes)) return -1;
  if (!bind_buffers(*this, pl, im, maps.prog_arrays, s, p)) return -1;
  if (!upkeep.before(b->count, p.lru_seq)) {
    error = upkeep.err;
    return -1;
  }
  report_launch(*this, pl, p);
  if (!queue_kernels(*this, b, f, l, pl, p, s)) return -1;
  upkeep.after();
  if (!(b->flags & EBPF_BATCH_SYNC)) return 0;
  const int64_t failed = upkeep.finish(p.err_count, s, "batch sync failed: ");
  if (failed < 0) error = upkeep.err.empty() ? bpftime_amd_last_error() : upkeep.err;
  return (int)failed;
}

// ebpf_exec: one unit, copied to the device and back.
int Mi355xVm::exec_one(void *mem, size_t mem_len, uint64_t *ret) {
  if (!loaded) {
    error = "no program loaded";
    return -1;
  }
  struct XdpMd {
    uint64_t data, data_end;
    uint32_t data_meta, ingress_ifindex, rx_queue_index, egress_ifindex;
    uint64_t buffer_start, buffer_end;
  };
  uint8_t *host_base;
  size_t slot_bytes;
  uint32_t head = 0, len;
  XdpMd *x = nullptr;
  if (ctx_kind == CTX_XDP) {
    x = (XdpMd *)mem;
    uint64_t lo = x->buffer_start && x->buffer_start <= x->data ? x->buffer_start : x->data;
    uint64_t hi = x->buffer_end && x->buffer_end >= x->data_end ? x->buffer_end : x->data_end;
    host_base = (uint8_t *)(uintptr_t)lo;
    slot_bytes = hi - lo;
    head = (uint32_t)(x->data - lo);
    len = (uint32_t)(x->data_end - x->data);
  } else {
    host_base = (uint8_t *)mem;
    slot_bytes = mem_len;
    len = (uint32_t)mem_len;
  }
  std::lock_guard<std::mutex> sg(stage_mu);  // one ebpf_exec at a time per VM uses the staging buffer
  size_t need = ((slot_bytes + 255) & ~(size_t)255) + 64;
  if (need > stage_size) {
    if (d_stage) hipFree(d_stage);
    if (hipMalloc((void **)&d_stage, need) != hipSuccess) {
      d_stage = nullptr;
      stage_size = 0;
      error = "staging alloc failed";
      return -1;
    }
    stage_size = need;
  }
  uint8_t *d_slot = d_stage + 64;
  uint64_t *d_ret = (uint64_t *)d_stage;
  int32_t *d_off = (int32_t *)(d_stage + 8);
  uint32_t *d_len = (uint32_t *)(d_stage + 12);
  if (slot_bytes && hipMemcpy(d_slot, host_base, slot_bytes, hipMemcpyHostToDevice) != hipSuccess) return -1;
  ebpf_batch b{};
  b.ctx_kind = ctx_kind;
  b.flags = EBPF_BATCH_SYNC | EBPF_BATCH_ORDERED;
  b.count = 1;
  b.data = d_slot;
  b.stride = slot_bytes ? slot_bytes : 1;
  b.fixed_len = len;
  b.head = head;
  b.rets = d_ret;
  if (x) {
    b.data_off_out = d_off;
    b.len_out = d_len;
    b.ingress_ifindex = x->ingress_ifindex;
    b.rx_queue_index = x->rx_queue_index;
  }
  int failed = exec_batch(&b);
  if (failed < 0) return -1;
  uint8_t hdr[16];
  if (hipMemcpy(hdr, d_stage, 16, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  if (slot_bytes && hipMemcpy(host_base, d_slot, slot_bytes, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  if (failed) {
    error = "program execution failed on device";
    return -1;
  }
  uint64_t r0;
  memcpy(&r0, hdr, 8);
  if (x) {
    int32_t off;
    uint32_t l;
    memcpy(&off, hdr + 8, 4);
    memcpy(&l, hdr + 12, 4);
    x->data = (uint64_t)(uintptr_t)host_base + (uint64_t)(int64_t)off;
    x->data_end = x->data + l;
  }
  *ret = r0;
  return 0;
}

}  // namespace bpftime_amd
