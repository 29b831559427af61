// bpftime_amd: uprobe / uretprobe / override dispatch over recorded function
// calls (include/bpftime_amd.h, "uprobe replay").
//
// The reference hooks a function with frida-gum and, per call, runs the
// attached programs on the calling thread (attach/frida_uprobe_attach_impl):
//  * a function whose first attachment is an override / replace is hooked by
//    replacement: only that program runs, and every later attach at the
//    function fails with -EEXIST (frida_uprobe_attach_impl.cpp:64-79);
//  * any other function is hooked as a listener
//    (frida_internal_attach_entry.cpp:128-165): its uprobes run at entry and
//    its uretprobes at return, in attach order (:221-239); an override
//    attached after them is kept in the list and never run;
//  * a uprobe / uretprobe callback sees the function's address through
//    bpf_get_func_ip, an override callback 0 (frida_attach_entry.hpp:25-40);
//    bpf_get_attach_cookie is the attachment's cookie or 0;
//  * the override handler (:243-277) runs the program on the entry registers
//    and, when it called bpf_override_return / bpf_set_retval, returns that
//    value in place of the call; a replace always returns the program's r0
//    (frida_uprobe_attach_impl.cpp:236-263).
// Here the calls are recorded and one of two plans runs them:
//  * program-major (the default): every attachment runs once over the records
//    of its function (uprobe_dispatch.hip gathers them), entry attachments in
//    attach order, then return attachments.  That equals the per-call order
//    when the programs commute; two that may not (the loader's map effects,
//    as the syscall dispatch reads them) are refused;
//  * thread-ordered (BPFTIME_AMD_DISPATCH_THREADS): the records grouped by
//    their recorded thread (group.hip), one lane per thread walking its calls
//    in record order, each call's entry callbacks and then its return
//    callbacks back to back (interp.hip k_up_seq; vm_seq.cpp useq_dispatch) --
//    the reference's schedule, whatever the programs share.  funclatency's
//    pair is the case (example/tracing/funclatency/funclatency.bpf.c: the
//    entry probe stores starts[tid], the return probe reads it).  The plan is
//    opt-in, never taken by itself: the refusal above is pinned behaviour.
//    With an event list (bpftime_amd_uprobe_dispatch_events) the lanes walk
//    recorded entries and returns, not whole calls: a nested or recursive
//    call's return runs after the entries recorded inside it, as frida's
//    on_enter / on_leave order them on the calling thread.
// Host-side bookkeeping only; the work is on the device.
#include <errno.h>
#include <stdlib.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/bpftime_amd.h"
#include "../../include/ebpf-vm.h"
#include "runtime.hpp"
#include "uprobe_dispatch.hpp"

extern "C" size_t bpftime_amd_group_scratch_bytes(uint64_t n);
extern "C" hipError_t bpftime_amd_group_threads(const void *pid, uint64_t stride, uint64_t n, void *scratch,
                                                uint32_t **perm, uint32_t **seg, uint64_t *nseg,
                                                hipStream_t stream);

using namespace bpftime_amd;

namespace {

struct Attach {
  int id;
  int prog_fd;
  uint64_t func;
  int kind;  // BPFTIME_AMD_UPROBE / _URETPROBE / _UPROBE_OVERRIDE / _UREPLACE
  int flags; // vm_prog_flags
  int link_fd;  // the link this attachment was bound from, or -1
  std::string name;
  std::shared_ptr<struct ebpf_vm> vm;  // (shared: a dispatch in flight keeps it through a detach)
};

bool overrides(int kind) { return kind == BPFTIME_AMD_UPROBE_OVERRIDE || kind == BPFTIME_AMD_UREPLACE; }

std::mutex g_mu;
std::vector<Attach> g_attach;  // in attach order
// how each function with attachments is hooked: true by replacement (its first
// attachment was an override / replace), false as a listener.  Kept until the
// function's last attachment goes, as the reference keeps its internal entry
std::map<uint64_t, bool> g_replaced;
int g_next_id = 1;

// Per-stream device scratch and the lock a dispatch holds from taking it until
// its last launch is queued (as the syscall dispatch's)
std::mutex g_buf_mu;
struct Buf {
  void *p = nullptr;
  uint64_t bytes = 0;
};
struct StreamBufs {
  Buf counts, rows;
  Buf group;  // the thread-ordered plan: its failure counter, then the thread grouping
  std::shared_ptr<std::mutex> mu = std::make_shared<std::mutex>();
};
std::map<hipStream_t, StreamBufs> g_bufs;

uint8_t *grow(Buf &b, uint64_t bytes, hipStream_t s) {
  if (b.bytes < bytes) {
    if (b.p && (hipStreamSynchronize(s) != hipSuccess || hipFree(b.p) != hipSuccess)) return nullptr;
    b.p = nullptr;
    b.bytes = 0;
    if (hipMalloc(&b.p, bytes) != hipSuccess) return nullptr;
    b.bytes = bytes;
  }
  return (uint8_t *)b.p;
}

int64_t fail(const std::string &what, int err) {
  set_error("uprobe dispatch: " + what);
  errno = err;
  return -1;
}

// The attachments a dispatch runs, program-major: those at entry (uprobes of
// listener functions, the override / replace of a replaced one) in attach
// order, then the uretprobes in attach order
void running(std::vector<Attach> &entry, std::vector<Attach> &leave) {
  std::lock_guard<std::mutex> g(g_mu);
  std::map<uint64_t, bool> seen;
  for (const Attach &a : g_attach) {
    const bool first = !seen[a.func];
    seen[a.func] = true;
    const bool replaced = g_replaced[a.func];
    if (replaced) {
      if (first && overrides(a.kind)) entry.push_back(a);  // (nothing else is attached there)
    } else if (a.kind == BPFTIME_AMD_UPROBE) {
      entry.push_back(a);
    } else if (a.kind == BPFTIME_AMD_URETPROBE) {
      leave.push_back(a);
    }  // (a late override: never run)
  }
}

// The first pair of attachments that may not commute, by the dispatches'
// shared analysis (runtime.hpp first_map_conflict).  Programs at different
// functions see disjoint records but still share their maps.
// 0 none, 1 found (*what names it), -1 a program is not loaded.
int first_conflict(const std::vector<Attach> &order, std::string *what) {
  std::vector<const struct ebpf_vm *> vms;
  for (const Attach &a : order) vms.push_back(a.vm.get());
  size_t i = 0, j = 0;
  int map = -1;
  const int c = first_map_conflict(vms, &i, &j, &map);
  if (c <= 0) return c;
  auto who = [&](size_t k) {
    return "'" + order[k].name + "' (prog fd " + std::to_string(order[k].prog_fd) + ", attachment " +
           std::to_string(order[k].id) + ")";
  };
  // (i == j: one program against itself, its calls of one thread in
  // parallel lanes -- runtime.hpp first_map_conflict)
  *what = (i == j ? "program " + who(i) + " may not commute with itself on "
                  : "programs " + who(i) + " and " + who(j) + " may not commute on ") +
          (map < 0 ? std::string("a map the loader cannot place") : "map fd " + std::to_string(map)) +
          ": program-major order would differ from the per-call order (detach one, or dispatch them apart); "
          "BPFTIME_AMD_DISPATCH_THREADS runs them in the per-call order";
  return 1;
}

// What the thread-ordered plan does not run, named (empty: nothing)
std::string threads_refusal(const std::vector<Attach> &order, uint32_t flags) {
  if (order.size() > kSeqMaxProgs)
    return std::to_string(order.size()) + " running attachments: the thread-ordered plan holds at most " +
           std::to_string(kSeqMaxProgs);
  std::vector<std::vector<uint64_t>> ids;
  for (const Attach &a : order) {
    if (a.flags & kProgReadsStacks)
      return "'" + a.name + "' calls bpf_get_stackid / bpf_get_stack: the STACK_TRACE commit order belongs to the "
             "program-major plan, the thread-ordered plan does not run it";
    // lanes in thread order are not record order across threads
    if (!(flags & EBPF_BATCH_ORDERED) && vm_touches_qs(a.vm.get()))
      return "'" + a.name + "' touches a QUEUE / STACK map: the thread-ordered plan runs it only with EBPF_BATCH_ORDERED";
    std::vector<uint64_t> id(9);
    if (vm_task_identity(a.vm.get(), id.data()) < 0) return "an attached program is not loaded";
    if (std::find(ids.begin(), ids.end(), id) == ids.end()) ids.push_back(id);
  }
  if (ids.size() > kSeqMaxTasks)
    return "the attached programs' VMs have " + std::to_string(ids.size()) +
           " distinct task identities: the thread-ordered plan holds at most " + std::to_string(kSeqMaxTasks);
  return "";
}

// The plan of a dispatch with these flags over the running attachments
// (entry, then return): 1 thread-ordered, 0 program-major, -1 a named error
int plan_for(const std::vector<Attach> &order, uint32_t flags) {
  const bool threads = (flags & BPFTIME_AMD_DISPATCH_THREADS) != 0;
  if (threads && (flags & BPFTIME_AMD_DISPATCH_PROGRAMS))
    return (int)fail("BPFTIME_AMD_DISPATCH_PROGRAMS and BPFTIME_AMD_DISPATCH_THREADS name different plans", EINVAL);
  if (threads) {
    const std::string why = threads_refusal(order, flags);
    return why.empty() ? 1 : (int)fail(why, EINVAL);
  }
  std::string what;
  const int c = first_conflict(order, &what);
  if (c < 0) return (int)fail("an attached program is not loaded", EINVAL);
  if (c) return (int)fail(what, EINVAL);
  return 0;
}

int attach(int prog_fd, uint64_t func, int kind, const uint64_t *cookie, int link_fd) {
  if (!bpftime_is_prog_fd(prog_fd) || (kind != BPFTIME_AMD_UPROBE && kind != BPFTIME_AMD_URETPROBE && !overrides(kind))) {
    set_error("uprobe attach: not a program fd, or an attach kind other than 6 / 7 / 1008 / 1009");
    errno = EINVAL;
    return -1;
  }
  {  // (before the program is instantiated: the common refusal costs no load)
    std::lock_guard<std::mutex> g(g_mu);
    auto it = g_replaced.find(func);
    if (it != g_replaced.end() && it->second) {
      set_error("uprobe attach: the function was already attached with replace or override, cannot attach anything else");
      errno = EEXIST;
      return -1;
    }
  }
  char *err = nullptr;
  struct ebpf_vm *vm = bpftime_amd_prog_instantiate(prog_fd, &err);
  if (!vm) {
    set_error(std::string("uprobe attach: ") + (err ? err : "load failed"));
    free(err);
    errno = EINVAL;
    return -1;
  }
  std::shared_ptr<struct ebpf_vm> owned(vm, ebpf_destroy);
  ebpf_set_ctx_kind(vm, EBPF_CTX_UPROBE);
  // (func_ip: 0 inside an override / replace callback)
  bpftime_amd_vm_set_attach(vm, overrides(kind) ? 0 : func, cookie ? *cookie : 0);
  const int flags = vm_prog_flags(vm);
  if (flags < 0) {
    set_error("uprobe attach: the program is not loaded");
    errno = EINVAL;
    return -1;
  }
  std::string name;
  {
    Runtime &r = rt();
    std::lock_guard<std::mutex> g(r.mu);
    name = r.progs[prog_fd].name;
  }
  std::lock_guard<std::mutex> g(g_mu);
  auto it = g_replaced.find(func);
  if (it != g_replaced.end() && it->second) {  // (another thread replaced it meanwhile)
    set_error("uprobe attach: the function was already attached with replace or override, cannot attach anything else");
    errno = EEXIST;
    return -1;
  }
  if (it == g_replaced.end()) g_replaced[func] = overrides(kind);
  g_attach.push_back(Attach{g_next_id, prog_fd, func, kind, flags, link_fd, name, std::move(owned)});
  return g_next_id++;
}

// ebpf_batch's rules for the stack fields (vm_exec.cpp exec_batch), checked
// here so that a dispatch is refused before its first launch
std::string stack_fields_bad(const struct bpftime_amd_call_records *r) {
  if (!r->stack_arr) return "";
  if ((uintptr_t)r->stack_arr % 8 != 0) return "stack_arr: an 8-aligned array";
  if (r->stack_unit_stride == 0 || r->stack_unit_stride % 8 != 0)
    return "stack_unit_stride " + std::to_string(r->stack_unit_stride) + ": a nonzero multiple of 8";
  if (r->stack_frame_stride == 0 || r->stack_frame_stride % 8 != 0)
    return "stack_frame_stride " + std::to_string(r->stack_frame_stride) + ": a nonzero multiple of 8";
  if ((uintptr_t)r->stack_depths % 4 != 0) return "stack_depths: a 4-aligned array";
  if (r->stack_max_depth < 1 || r->stack_max_depth > 127)
    return "stack_max_depth " + std::to_string(r->stack_max_depth) + ": 1..127";
  return "";
}

uint64_t up(uint64_t v) { return (v + 255) & ~255ull; }

// EBPF_BATCH_TIMED: the last such dispatch's kernel times, summed over its
// attachments (bpftime_amd_uprobe_last_ms)
std::mutex g_time_mu;
struct Times {
  float count_ms = 0, gather_ms = 0;  // (thread-ordered plan: the grouping, the replay kernel)
  uint64_t rows = 0;                  // (... and the records, or the events of an event list)
} g_times;

// a pair of events around launches on s (no-ops unless `on`)
struct Span {
  hipEvent_t a = nullptr, b = nullptr;
  bool on;
  hipStream_t s;
  Span(bool on_, hipStream_t s_) : on(on_), s(s_) {
    if (on && (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess)) on = false;
    if (on) hipEventRecord(a, s);
  }
  void end() {
    if (on) hipEventRecord(b, s);
  }
  float ms() {  // (after the stream was synchronized past end())
    float v = 0;
    if (on && hipEventSynchronize(b) == hipSuccess) hipEventElapsedTime(&v, a, b);
    return v;
  }
  ~Span() {
    if (a) hipEventDestroy(a);
    if (b) hipEventDestroy(b);
  }
};

// One attachment over the records: count, gather, run, scatter.  >= 0 failed
// callbacks (SYNC), -1 error.
int64_t run_one(const Attach &a, bool at_entry, const struct bpftime_amd_call_records *r, uint32_t *out_state,
                int64_t *out_rets, uint32_t flags, StreamBufs &sb, hipStream_t s) {
  const uint64_t n = r->count;
  UGather g{};
  g.regs = (const uint64_t *)(at_entry ? r->enter : r->leave);
  g.func = r->func;
  g.pid = r->pid_tgid;
  g.clock = (const uint64_t *)r->clock;
  g.target = a.func;
  g.n = n;
  g.phase = at_entry ? 0 : 1;
  g.chunks = (uint32_t)((n + 63) / 64);
  uint8_t *cb = grow(sb.counts, up(4ull * g.chunks) + 256, s);
  if (!cb) return fail("scratch allocation failed", ENOMEM);
  g.counts = (uint32_t *)cb;
  g.total = (uint32_t *)(cb + up(4ull * g.chunks));
  const bool timed = (flags & EBPF_BATCH_TIMED) != 0;
  Span t_count(timed, s);
  hipError_t e = bpftime_amd_launch_ug_count(&g, s);
  t_count.end();
  uint32_t m = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&m, g.total, 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return fail(std::string("match count: ") + hipGetErrorString(e), EIO);
  if (timed) {
    std::lock_guard<std::mutex> tg(g_time_mu);
    g_times.count_ms += t_count.ms();
  }
  if (m == 0) return 0;  // nothing of this function in the records: nothing to launch
  const bool ovr = overrides(a.kind), replace = a.kind == BPFTIME_AMD_UREPLACE;
  const bool stacks = r->stack_arr && (a.flags & kProgReadsStacks);
  const uint32_t D = r->stack_max_depth;
  // rows | override state, values | stack rows, depths
  const uint64_t rows_b = up((uint64_t)m * kRowBytes), st_b = ovr ? up(4ull * m) : 0, val_b = ovr ? up(8ull * m) : 0;
  const uint64_t sr_b = stacks ? up(8ull * m * D) : 0, sd_b = stacks ? up(4ull * m) : 0;
  uint8_t *rb = grow(sb.rows, rows_b + st_b + val_b + sr_b + sd_b, s);
  if (!rb) return fail("scratch allocation failed", ENOMEM);
  g.rows = (uint64_t *)rb;
  g.cap = m;
  uint32_t *st = (uint32_t *)(rb + rows_b);
  int64_t *vals = (int64_t *)(rb + rows_b + st_b);
  if (stacks) {
    g.stack_arr = (const uint8_t *)r->stack_arr;
    g.stack_unit_stride = r->stack_unit_stride;
    g.stack_frame_stride = r->stack_frame_stride;
    g.stack_depths = r->stack_depths;
    g.stack_fixed_depth = r->stack_fixed_depth;
    g.stack_max_depth = D;
    g.stack_rows = (uint64_t *)(rb + rows_b + st_b + val_b);
    g.stack_depths_out = (uint32_t *)(rb + rows_b + st_b + val_b + sr_b);
  }
  g.pid_default = 0;  // (without recorded callers the batch answers the dispatching thread's itself)
  Span t_gather(timed, s);
  e = bpftime_amd_launch_ug_gather(&g, s);
  t_gather.end();
  if (e == hipSuccess && ovr) e = hipMemsetAsync(st, 0, st_b + val_b, s);
  if (e != hipSuccess) return fail(std::string("gather: ") + hipGetErrorString(e), EIO);
  struct ebpf_batch b = {};
  b.ctx_kind = EBPF_CTX_UPROBE;
  b.flags = flags & (EBPF_BATCH_SYNC | EBPF_BATCH_UNCHECKED | EBPF_BATCH_ORDERED);
  b.count = m;
  b.data = rb;
  b.stride = kRowBytes;
  b.stream = s;
  if (r->pid_tgid) b.pid_tgid_off = kRowPidOff;
  if (r->clock) b.ktime_off = kRowClockOff;
  if (ovr) {
    // 58 / 187 record into the compact state; a plain uprobe / uretprobe has
    // none and the helpers fail its unit
    b.sys_state = st;
    b.sys_ret = vals;
    b.sys_phase = 1;
    if (replace) b.rets = (uint64_t *)vals;  // r0 is the value (a failed unit reports 0, bpftime_prog.cpp:250-257)
  }
  if (stacks) {
    b.stack_arr = g.stack_rows;
    b.stack_unit_stride = 8ull * D;
    b.stack_frame_stride = 8;
    b.stack_depths = g.stack_depths_out;
    b.stack_max_depth = D;
  }
  const int rc = ebpf_exec_batch(a.vm.get(), &b);
  if (rc < 0) return -1;
  if (timed) {
    std::lock_guard<std::mutex> tg(g_time_mu);
    g_times.gather_ms += t_gather.ms();
    g_times.rows += m;
  }
  if (ovr) {
    e = bpftime_amd_launch_ug_scatter(g.rows, m, n, st, vals, replace ? 1 : 0, out_state, out_rets, s);
    if (e == hipSuccess && (flags & EBPF_BATCH_SYNC)) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(std::string("scatter: ") + hipGetErrorString(e), EIO);
  }
  return rc;
}

// The thread-ordered plan: group the records by caller, one launch for every
// attachment (vm_seq.cpp useq_dispatch).  >= 0 failed callbacks (SYNC), -1 error.
// With `events` (n_events words (record << 1) | phase) the walked items are the
// events: they are grouped by their record's caller (uprobe_dispatch.hip
// k_ug_event_keys, which also counts the events naming no record; the count
// is read in the grouping's host wait) and the grouping's perm is rewritten to
// the event words.  One thread walks the caller's list itself.
int64_t dispatch_threads(const std::vector<Attach> &order, size_t nentry, const struct bpftime_amd_call_records *r,
                         const uint32_t *events, uint64_t n_events, uint32_t *out_state, int64_t *out_rets,
                         uint32_t flags, StreamBufs &sb, hipStream_t s) {
  const uint64_t n = events ? n_events : r->count;  // the walked items
  std::vector<USeqAttach> progs;
  for (size_t i = 0; i < order.size(); i++) {
    const int k = order[i].kind;
    progs.push_back({order[i].vm.get(), order[i].func, i >= nentry,
                     k == BPFTIME_AMD_UREPLACE ? kUpReplace : k == BPFTIME_AMD_UPROBE_OVERRIDE ? kUpOverride : kUpPlain});
  }
  // one thread: an ORDERED dispatch (the serial reference run) or records
  // without a recorded caller (every call is the dispatching thread's)
  const bool one = (flags & EBPF_BATCH_ORDERED) || !r->pid_tgid;
  const uint64_t gbytes = one ? 0 : bpftime_amd_group_scratch_bytes(n);
  if (!one && !gbytes) return fail("thread grouping of " + std::to_string(n) + " records", EINVAL);
  // the failure counter and the out-of-range count | the grouping | the events' keys
  const uint64_t keys_b = events && !one ? up(8 * n) : 0;
  uint8_t *buf = grow(sb.group, 256 + up(gbytes) + keys_b, s);
  if (!buf) return fail("scratch allocation failed", ENOMEM);
  const bool timed = (flags & EBPF_BATCH_TIMED) != 0;
  UpSeqParams p{};
  p.nseg = 1;
  Span t_group(timed, s);
  const void *keys = r->pid_tgid;
  uint32_t bad = 0;  // (events naming no record: read in the wait below)
  if (events) {
    uint32_t *bad_d = (uint32_t *)(buf + 128);
    keys = one ? nullptr : buf + 256 + up(gbytes);
    hipError_t e = bpftime_amd_launch_ug_event_keys(events, n, one ? nullptr : r->pid_tgid, r->count, (uint64_t *)keys,
                                                    bad_d, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, bad_d, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && one) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
      hipStreamSynchronize(s);  // (nothing is left writing `bad`)
      return fail(std::string("event key pass: ") + hipGetErrorString(e), EIO);
    }
  }
  if (!one) {
    const hipError_t e = bpftime_amd_group_threads(keys, 8, n, buf + 256, const_cast<uint32_t **>(&p.perm),
                                                   const_cast<uint32_t **>(&p.seg), &p.nseg, s);
    if (e != hipSuccess) {
      hipStreamSynchronize(s);
      return fail(std::string("thread grouping: ") + hipGetErrorString(e), EIO);
    }
  }
  if (events) {
    if (bad)
      return fail(std::to_string(bad) + " of the " + std::to_string(n) + " events name a record index >= count (" +
                      std::to_string(r->count) + "): nothing was run",
                  EINVAL);
    if (order.empty()) return 0;
    if (one) {
      p.perm = events;
    } else {
      const hipError_t e = bpftime_amd_launch_ug_event_words(const_cast<uint32_t *>(p.perm), events, n, s);
      if (e != hipSuccess) return fail(std::string("event words: ") + hipGetErrorString(e), EIO);
    }
    p.events = 1;
    p.nrec = r->count;
  }
  t_group.end();
  p.n = n;
  p.enter = (const uint64_t *)r->enter;
  p.leave = (const uint64_t *)r->leave;
  p.func = r->func;
  p.pid = r->pid_tgid;
  p.clock = (const uint64_t *)r->clock;
  p.out_state = out_state;
  p.out_rets = out_rets;
  Span t_run(timed, s);
  const int64_t rc = useq_dispatch(progs, p, flags, (uint32_t *)buf, s);
  t_run.end();
  if (rc >= 0 && timed && hipStreamSynchronize(s) == hipSuccess) {
    std::lock_guard<std::mutex> tg(g_time_mu);
    g_times.count_ms = t_group.ms();
    g_times.gather_ms = t_run.ms();
    g_times.rows = n;
  }
  return rc;
}

// What bpftime_amd_uprobe_dispatch and _dispatch_events (`events` non-null:
// its own refusals made, the flags naming the thread-ordered plan) share: the
// records' checks, the running attachments, the plan and the stream's buffers
int64_t dispatch(const struct bpftime_amd_call_records *r, const uint32_t *events, uint64_t n_events,
                 uint32_t *out_state, int64_t *out_rets, uint32_t flags, void *stream) {
  if (!r) return fail("no records", EINVAL);
  if (r->count && !r->func) return fail("no func array: the records need each call's function address", EINVAL);
  if (r->count > 0xffffffffull) return fail("more than 2^32 records", EINVAL);
  for (const void *a : {r->enter, r->leave, (const void *)r->func, (const void *)r->pid_tgid, r->clock})
    if ((uintptr_t)a % 8) return fail("the record arrays must be 8-aligned", EINVAL);
  std::vector<Attach> entry, leave;
  running(entry, leave);
  if (!entry.empty() && r->count && !r->enter)
    return fail("uprobe / override programs are attached: the records need the enter registers", EINVAL);
  if (!leave.empty() && r->count && !r->leave)
    return fail("uretprobe programs are attached: the records need the leave registers", EINVAL);
  const std::string sbad = stack_fields_bad(r);
  if (!sbad.empty()) return fail(sbad, EINVAL);
  bool any_ovr = false;
  for (const Attach &a : entry) any_ovr |= overrides(a.kind);
  if (any_ovr && (!out_state || !out_rets))
    return fail("override / replace programs are attached: out_state and out_rets are needed", EINVAL);
  std::vector<Attach> order = entry;
  order.insert(order.end(), leave.begin(), leave.end());
  const int plan = plan_for(order, flags);
  if (plan < 0) return -1;
  // (an event list is range-checked whatever is attached: dispatch_threads)
  if (!events && (r->count == 0 || order.empty())) return 0;
  hipStream_t s = (hipStream_t)stream;
  StreamBufs *sb;
  std::shared_ptr<std::mutex> mu;
  {
    std::lock_guard<std::mutex> g(g_buf_mu);
    sb = &g_bufs[s];  // (std::map: the node stays where it is)
    mu = sb->mu;
  }
  std::lock_guard<std::mutex> hold(*mu);
  if (flags & EBPF_BATCH_TIMED) {
    std::lock_guard<std::mutex> tg(g_time_mu);
    g_times = Times();
  }
  if (plan) return dispatch_threads(order, entry.size(), r, events, n_events, out_state, out_rets, flags, *sb, s);
  int64_t failed = 0;
  for (size_t i = 0; i < order.size(); i++) {
    const int64_t rc = run_one(order[i], i < entry.size(), r, out_state, out_rets, flags, *sb, s);
    if (rc < 0) return -1;
    failed += rc;
  }
  return failed;
}

}  // namespace

void bpftime_amd::uprobe_detach_all() {
  std::lock_guard<std::mutex> g(g_mu);
  g_attach.clear();
  g_replaced.clear();
}

extern "C" {

int bpftime_amd_uprobe_attach(int prog_fd, uint64_t func, int kind, const uint64_t *cookie) {
  return attach(prog_fd, func, kind, cookie, -1);
}

int bpftime_amd_uprobe_attach_link(int link_fd, uint64_t func) {
  Runtime &r = rt();
  int prog_fd, kind;
  bool has_cookie;
  uint64_t cookie;
  {
    std::lock_guard<std::mutex> g(r.mu);
    if (link_fd < 0 || link_fd >= (int)kMaxFds || r.kind[link_fd] != HKind::LINK || !r.links[link_fd].perf ||
        r.kind[r.links[link_fd].target] != HKind::PERF) {
      set_error("uprobe attach: fd " + std::to_string(link_fd) + " is no link to a perf event");
      errno = EINVAL;
      return -1;
    }
    const LinkRec &l = r.links[link_fd];
    if (l.uprobe_id) {
      set_error("uprobe attach: link " + std::to_string(link_fd) + " is already bound");
      errno = EEXIST;
      return -1;
    }
    kind = r.perfs[l.target].type;  // bpf_event_type: 6 uprobe, 7 uretprobe, 1008 override
    prog_fd = (int)l.prog_fd;
    has_cookie = l.has_cookie;
    cookie = l.cookie;
  }
  if (kind != BPFTIME_AMD_UPROBE && kind != BPFTIME_AMD_URETPROBE && kind != BPFTIME_AMD_UPROBE_OVERRIDE) {
    set_error("uprobe attach: the link's perf event is no uprobe, uretprobe or uprobe override");
    errno = EINVAL;
    return -1;
  }
  const int id = attach(prog_fd, func, kind, has_cookie ? &cookie : nullptr, link_fd);
  if (id < 0) return -1;
  std::lock_guard<std::mutex> g(r.mu);
  if (r.kind[link_fd] == HKind::LINK) r.links[link_fd].uprobe_id = id;
  return id;
}

int bpftime_amd_uprobe_link_bound(int link_fd) {
  Runtime &r = rt();
  std::lock_guard<std::mutex> g(r.mu);
  if (link_fd < 0 || link_fd >= (int)kMaxFds || r.kind[link_fd] != HKind::LINK) return -1;
  return r.links[link_fd].uprobe_id ? 1 : 0;
}

int bpftime_amd_uprobe_detach(int id) {
  int link_fd = -1;
  {
    std::lock_guard<std::mutex> g(g_mu);
    auto it = g_attach.begin();
    while (it != g_attach.end() && it->id != id) ++it;
    if (it == g_attach.end()) {
      errno = ENOENT;
      return -1;
    }
    const uint64_t func = it->func;
    link_fd = it->link_fd;
    g_attach.erase(it);
    bool left = false;
    for (const Attach &a : g_attach) left |= a.func == func;
    if (!left) g_replaced.erase(func);  // (the hook goes with its last attachment)
  }
  if (link_fd >= 0) {
    Runtime &r = rt();
    std::lock_guard<std::mutex> g(r.mu);
    if (r.kind[link_fd] == HKind::LINK && r.links[link_fd].uprobe_id == id) r.links[link_fd].uprobe_id = 0;
  }
  return 0;
}

int bpftime_amd_uprobe_last_ms(float *count_ms, float *gather_ms, uint64_t *rows) {
  std::lock_guard<std::mutex> tg(g_time_mu);
  if (count_ms) *count_ms = g_times.count_ms;
  if (gather_ms) *gather_ms = g_times.gather_ms;
  if (rows) *rows = g_times.rows;
  return 0;
}

int bpftime_amd_uprobe_dispatch_plan(uint32_t flags) {
  std::vector<Attach> order, leave;
  running(order, leave);
  order.insert(order.end(), leave.begin(), leave.end());
  return plan_for(order, flags);
}

int64_t bpftime_amd_uprobe_dispatch(const struct bpftime_amd_call_records *r, uint32_t *out_state, int64_t *out_rets,
                                    uint32_t flags, void *stream) {
  return dispatch(r, nullptr, 0, out_state, out_rets, flags, stream);
}

int64_t bpftime_amd_uprobe_dispatch_events(const struct bpftime_amd_call_records *r, const uint32_t *events,
                                           uint64_t n_events, uint32_t *out_state, int64_t *out_rets, uint32_t flags,
                                           void *stream) {
  if (!r) return fail("no records", EINVAL);
  if (!events || !n_events) return fail("no events: the event list needs at least one (record, phase) word", EINVAL);
  if ((uintptr_t)events % 4) return fail("the event list must be 4-aligned", EINVAL);
  if (r->count >= (1ull << 31))
    return fail("2^31 or more records: an event word holds a 31-bit record index", EINVAL);
  if (n_events > 0xffffffffull) return fail("more than 2^32 - 1 events", EINVAL);
  // the plan: thread-ordered only
  if (!(flags & BPFTIME_AMD_DISPATCH_THREADS))
    return fail("an event list runs under the thread-ordered plan only: BPFTIME_AMD_DISPATCH_THREADS is required",
                EINVAL);
  if (flags & BPFTIME_AMD_DISPATCH_PROGRAMS)
    return fail("BPFTIME_AMD_DISPATCH_PROGRAMS: an event list runs under the thread-ordered plan only "
                "(BPFTIME_AMD_DISPATCH_THREADS alone)",
                EINVAL);
  return dispatch(r, events, n_events, out_state, out_rets, flags, stream);
}

}  // extern "C"
