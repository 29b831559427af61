// bpftime_amd: what other files ask a VM (runtime.hpp vm_*), and the
// thread-ordered dispatches: one launch of k_sys_seq / k_up_seq that runs
// every attached program's callbacks.
#include "vm_impl.hpp"

using namespace bpftime_amd;

namespace bpftime_amd {
int vm_prog_flags(const ::ebpf_vm *vm) {
  if (!vm || !vm->impl->loaded) return -1;
  auto im = vm->impl->image();
  if (!im) return -1;
  return (im->prog.sets_retval ? kProgSetsRetval : 0) | (im->fr.stores_unit ? kProgStoresCtx : 0) |
         (im->prog.reads_stacks ? kProgReadsStacks : 0);
}

int vm_map_effects(const ::ebpf_vm *vm, std::map<int32_t, uint8_t> &fx, uint8_t &any) {
  if (!vm || !vm->impl->loaded) return -1;
  std::shared_ptr<Image> im;
  {
    // a tail-calling program's effects are its linked image's: the targets
    // its prog arrays name now, appended to it (link_tail_image_locked), so
    // the loader's pass over the image is the union over them
    std::lock_guard<std::mutex> g(vm->impl->img_mu);
    if (vm->impl->has_tail && vm->impl->link_tail_image_locked() < 0) return -1;
    im = vm->impl->img;
  }
  if (!im) return -1;
  fx = im->fr.map_fx;
  any = im->fr.any_fx;
  return 0;
}

bool vm_has_tail(const ::ebpf_vm *vm) { return vm && vm->impl->loaded && vm->impl->has_tail; }

bool vm_touches_qs(const ::ebpf_vm *vm) {
  if (!vm || !vm->impl->loaded) return false;
  auto im = vm->impl->image();
  if (!im) return false;
  std::string e;
  bool adds = false, takes = false;
  qs_launch_check(im->fr, true, e, adds, takes);
  return adds || takes;
}

// the tier of this host thread's most recent thread-ordered dispatch (1 asm,
// 0 C++, -1 none yet): bpftime_amd_last_seq_tier
thread_local int g_last_seq_tier = -1;

namespace {
// What the thread-ordered launches (k_sys_seq, k_up_seq) share: per attached
// program its checks and link, the table of task identities, and the map
// upkeep (vm_upkeep.cpp LaunchUpkeep) around the one launch that runs them all
struct SeqLaunch : LaunchUpkeep {
  // the images stay referenced until the launch is queued (a relink by
  // another thread never frees what is read: vm_impl.hpp Image)
  std::vector<std::shared_ptr<Image>> keep;
  uint32_t ntasks = 0;

  using LaunchUpkeep::LaunchUpkeep;

  // constant-address loads (loader.cpp const_loads: array storage nothing in
  // THAT program writes) stay scalar-cache loads only while no attached
  // program writes or adds to an array map: one launch runs them all
  bool array_writes(const std::vector<const ::ebpf_vm *> &vms) {
    bool any = false;
    for (const ::ebpf_vm *v : vms) {
      auto im = v->impl->image();
      if (!im) continue;
      const uint8_t w = FX_WRITE | FX_INIT | FX_ADD;
      any = any || (im->fr.any_fx & w);
      for (const auto &kv : im->fr.map_fx)
        if ((kv.second & w) && kv.first >= 0 && kv.first < (int32_t)kMaxFds &&
            (r.maps[kv.first].type == MT_ARRAY || r.maps[kv.first].type == MT_PERCPU_ARRAY))
          any = true;
    }
    return any;
  }

  // One attached program: its image and ORDERED link, and the index of its
  // VM's identity in `tasks` (one table entry per distinct identity), and its
  // VM's step limit.  `rec`:
  // the asm tier's link, with the kernel's caller / clock offsets (pid 0: the
  // C++ tier's)
  bool attach(Mi355xVm *vm, bool no_kldx, RecOffs rec, SeqTask *tasks, const DInsn *&prog, const FInsn *&link,
              uint32_t &task, uint32_t &step_limit) {
    auto im = vm->image();
    if (!vm->loaded || !im) return fail("an attached program is not loaded");
    if (vm->has_tail) return fail("an attached program calls bpf_tail_call (program-major dispatch runs it)");
    link = im->linked(false, false, 0, 0, true, -1, 0, 0, no_kldx, rec);
    if (!link) return fail("device upload failed");
    prog = im->d_prog;
    SeqTask tk{};
    vm->task_into(tk.uid_gid, tk.comm);
    uint32_t ti = 0;
    while (ti < ntasks && memcmp(&tasks[ti], &tk, sizeof(tk)) != 0) ti++;
    if (ti == ntasks) {
      if (ntasks == kSeqMaxTasks)
        return fail("the attached programs' VMs have more than " + std::to_string(kSeqMaxTasks) +
                    " distinct task identities");
      tasks[ntasks++] = tk;
    }
    task = ti;
    {  // ARRAY_OF_MAPS: the inner maps its slots name (as exec_batch)
      std::string ie;
      if (!inner_launch_check(im->fr, ie)) return fail(ie);
      if (!perf_launch_prepare(im->prog, ie)) return fail(ie);
    }
    {  // QUEUE / STACK maps: lanes in thread order are not record order across threads
      std::string qe;
      bool touches_add = false, touches_take = false;
      qs_launch_check(im->fr, true, qe, touches_add, touches_take);
      if ((touches_add || touches_take) && !ordered)
        return fail("an attached program touches a QUEUE / STACK map: it does not commute and runs only in "
                    "EBPF_BATCH_ORDERED dispatches");
      qs_adds |= touches_add;
      qs_takes |= touches_take;
    }
    if (!add(im->prog, im->fr)) return false;
    // (each callback runs under its own VM's limit, as in the program-major
    // plan: the kernels count in 32 bits)
    step_limit = (uint32_t)std::min<uint64_t>(vm->step_limit, 0xffffffffull);
    keep.push_back(std::move(im));
    return true;
  }
};
}  // namespace

int64_t seq_dispatch(const std::vector<SeqAttach> &progs, const SysLayout &lay, uint64_t n, const uint32_t *perm,
                     const uint32_t *seg, uint64_t nseg, int64_t *out, uint32_t flags, uint32_t *err, hipStream_t s) {
  auto fail = [](const std::string &e) {
    if (!e.empty()) set_error("thread-ordered dispatch: " + e);
    return (int64_t)-1;
  };
  if (progs.size() > kSeqMaxProgs)
    return fail(std::to_string(progs.size()) + " programs attached (at most " + std::to_string(kSeqMaxProgs) + ")");
  SeqParams p{};
  SeqLaunch L((flags & EBPF_BATCH_ORDERED) != 0);
  // the asm tier runs the callbacks when every stack fits the LDS stacks and
  // the threads are at most kSeqAsmThreads: measured (profiles/
  // r06_seq_xover.txt, syscount's pair) 2-3.7x the C++ tier up to 8192
  // threads, even at 16384, and behind it from 32768 on, where the waves no
  // longer wait on their own latency chains and the map helpers' coherent
  // atomics set the rate.  BPFTIME_AMD_SEQ_ASM=1 / 0 forces a tier.
  const char *asm_env = getenv("BPFTIME_AMD_SEQ_ASM");
  bool fast = asm_env && asm_env[0] ? asm_env[0] != '0' : nseg <= kSeqAsmThreads;
  std::vector<const ::ebpf_vm *> vms;
  for (const SeqAttach &a : progs) {
    vms.push_back(a.vm);
    auto im = a.vm->impl->image();
    if (!im) continue;
    fast = fast && !im->prog.big_stack && im->prog.stack_size <= kLdsStackMax;
  }
  const bool no_kldx = L.array_writes(vms) && progs.size() > 1;
  for (const SeqAttach &a : progs) {
    SeqProg &q = p.progs[p.nprogs++];
    uint32_t task = 0;
    if (!L.attach(a.vm->impl, no_kldx, fast ? kSeqRecOffs : RecOffs{}, p.tasks, q.prog, q.fast, task, q.step_limit))
      return fail(L.err);
    q.task = (uint16_t)task;
    q.sys_nr = a.sys_nr;
    q.enter = a.enter ? 1 : 0;
    // its attach cookie (a link's; a syscall tracepoint has no func_ip)
    uint64_t ip;
    a.vm->impl->attach_into(ip, p.cookies[p.nprogs - 1]);
  }
  Runtime &r = L.r;
  p.lay = lay;
  p.n = n;
  p.perm = perm;
  p.seg = seg;
  p.nseg = nseg;
  p.out = out;
  p.maps = r.d_maptab;
  p.ncpu = r.ncpu;
  p.checked = (flags & EBPF_BATCH_UNCHECKED) ? 0 : 1;
  p.arena_lo = (uint64_t)(uintptr_t)r.arena;
  p.arena_hi = p.arena_lo + r.arena_size;
  p.pid_tgid = ((uint64_t)(uint32_t)getpid() << 32) | (uint32_t)syscall(SYS_gettid);
  p.err_count = err;
  p.trace_log = trace_log().d;
  p.trace_cap = trace_log().cap;
  p.exact = L.ordered ? 1 : 0;
  p.fast = fast ? 1 : 0;
  if (!L.before(n, p.lru_seq)) return fail(L.err);
  hipError_t e = hipMemsetAsync(err, 0, 4, s);
  if (e == hipSuccess) e = bpftime_amd_launch_sys_seq(&p, s);
  if (e != hipSuccess) return fail(std::string("kernel launch failed: ") + hipGetErrorString(e));
  g_last_seq_tier = fast ? 1 : 0;
  L.after();
  if (!(flags & EBPF_BATCH_SYNC)) return 0;
  const int64_t failed = L.finish(err, s, "sync failed: ");
  return failed < 0 ? fail(L.err) : failed;
}

int vm_task_identity(const ::ebpf_vm *vm, uint64_t out[9]) {
  if (!vm || !vm->impl->loaded) return -1;
  vm->impl->task_into(out[0], out + 1);
  return 0;
}

int64_t useq_dispatch(const std::vector<USeqAttach> &progs, const UpSeqParams &recs, uint32_t flags, uint32_t *err,
                      hipStream_t s) {
  auto fail = [](const std::string &e) {
    if (!e.empty()) set_error("thread-ordered dispatch: " + e);
    return (int64_t)-1;
  };
  if (progs.size() > kSeqMaxProgs)
    return fail(std::to_string(progs.size()) + " programs attached (at most " + std::to_string(kSeqMaxProgs) + ")");
  UpSeqParams p = recs;  // (the records, their grouping and the outputs: uprobe_dispatch.cpp)
  p.nprogs = 0;
  SeqLaunch L((flags & EBPF_BATCH_ORDERED) != 0);
  // the tier, by seq_dispatch's rule: the asm tier when every stack fits the
  // LDS stacks and the threads are at most kUpSeqAsmThreads (measured:
  // profiles/uprobe_asm_measurement.txt; an ORDERED dispatch is one thread and
  // so takes the asm tier too); BPFTIME_AMD_SEQ_ASM=1 / 0 forces a tier, and
  // a forced 1 still falls back when a program does not qualify
  const char *asm_env = getenv("BPFTIME_AMD_SEQ_ASM");
  bool fast = asm_env && asm_env[0] ? asm_env[0] != '0' : p.nseg <= kUpSeqAsmThreads;
  const bool fast_asked = fast;
  int fallback = -1;  // the first attached program that keeps the dispatch in the C++ tier
  std::vector<const ::ebpf_vm *> vms;
  for (const USeqAttach &a : progs) {
    vms.push_back(a.vm);
    auto im = a.vm->impl->image();
    if (!im) continue;
    if (fast && (im->prog.big_stack || im->prog.stack_size > kLdsStackMax)) {
      fast = false;
      fallback = (int)vms.size() - 1;
    }
  }
  const bool no_kldx = L.array_writes(vms) && progs.size() > 1;
  for (const USeqAttach &a : progs) {
    UpSeqProg &q = p.progs[p.nprogs++];
    uint32_t task = 0;
    if (!L.attach(a.vm->impl, no_kldx, fast ? kUpSeqRecOffs : RecOffs{}, p.tasks, q.prog, q.fast, task, q.step_limit))
      return fail(L.err);
    q.task = (uint16_t)task;
    q.func = a.func;
    q.phase = a.at_return ? 1 : 0;
    q.kind = a.kind;
    uint64_t ip;  // (attach() set it to what kind and func say: common.hpp UpSeqProg)
    a.vm->impl->attach_into(ip, q.cookie);
  }
  Runtime &r = L.r;
  p.maps = r.d_maptab;
  p.ncpu = r.ncpu;
  p.checked = (flags & EBPF_BATCH_UNCHECKED) ? 0 : 1;
  p.arena_lo = (uint64_t)(uintptr_t)r.arena;
  p.arena_hi = p.arena_lo + r.arena_size;
  p.pid_tgid = ((uint64_t)(uint32_t)getpid() << 32) | (uint32_t)syscall(SYS_gettid);
  p.err_count = err;
  p.trace_log = trace_log().d;
  p.trace_cap = trace_log().cap;
  p.exact = L.ordered ? 1 : 0;
  p.fast = fast ? 1 : 0;
  if (!L.before(p.n, p.lru_seq)) return fail(L.err);
  if (getenv("BPFTIME_AMD_VERBOSE")) {
    std::string why;
    if (fast_asked && !fast)
      why = " (program " + std::to_string(fallback) + " at func 0x" + [&] {
        char b[32];
        snprintf(b, sizeof b, "%llx", (unsigned long long)progs[fallback].func);
        return std::string(b);
      }() + " needs a stack of more than " + std::to_string(kLdsStackMax) + " B or the scratch-stack kernels)";
    fprintf(stderr, "bpftime_amd: launch uprobe replay %s items %llu threads %llu block %u programs %u tier %s%s lds %zu\n",
            p.events ? "events" : "calls", (unsigned long long)p.n, (unsigned long long)p.nseg, kUpSeqBlock, p.nprogs,
            fast ? "asm" : "c++", why.c_str(), seq_lds_bytes(kUpSeqBlock, fast));
  }
  hipError_t e = hipMemsetAsync(err, 0, 4, s);
  if (e == hipSuccess) e = bpftime_amd_launch_up_seq(&p, s);
  if (e != hipSuccess) return fail(std::string("kernel launch failed: ") + hipGetErrorString(e));
  g_last_seq_tier = fast ? 1 : 0;
  L.after();
  if (!(flags & EBPF_BATCH_SYNC)) return 0;
  const int64_t failed = L.finish(err, s, "sync failed: ");
  return failed < 0 ? fail(L.err) : failed;
}
}  // namespace bpftime_amd

extern "C" int bpftime_amd_last_seq_tier(void) { return bpftime_amd::g_last_seq_tier; }
