// bpftime_amd: the drop-in VM C ABI (include/ebpf-vm.h).
//
// Mirrors vm/vm-core/src/ebpf-vm.cpp:6-98 over a single backend class that
// plays the role of a bpftime::vm::compat::bpftime_vm_impl
// (vm/compat/include/bpftime_vm_compat.hpp:27-198) registered under the name
// "mi355x" (the reference registers "ubpf" the same way,
// vm/compat/ubpf-vm/compat_ubpf.cpp:253-257).
#include "vm_impl.hpp"

namespace bpftime_amd {
// bpf_trace_printk's record log (vm_impl.hpp TraceLog)
TraceLog &trace_log() {
  static TraceLog t;
  return t;
}
int trace_log_ensure() {
  TraceLog &t = trace_log();
  std::lock_guard<std::mutex> g(t.mu);
  if (t.d) return 0;
  uint64_t cap = kTraceDefaultRecords;
  if (const char *e = getenv("BPFTIME_AMD_TRACE_RECORDS")) {
    const uint64_t v = strtoull(e, nullptr, 0);
    if (v >= 1 && v <= (1ull << 26)) cap = v;
  }
  uint8_t *d = nullptr;
  if (hipMalloc((void **)&d, kTraceHdrBytes + cap * kTraceRecBytes) != hipSuccess) return -1;
  if (hipMemset(d, 0, kTraceHdrBytes) != hipSuccess) {
    hipFree(d);
    return -1;
  }
  t.d = d;
  t.cap = cap;
  t.consumed = 0;
  return 0;
}
}  // namespace bpftime_amd

using namespace bpftime_amd;

extern "C" {

struct ebpf_vm *ebpf_create(const char *vm_name) {
  if (!vm_name || strcmp(vm_name, "mi355x") != 0) return nullptr;
  ebpf_vm *vm = new ebpf_vm;
  vm->impl = new Mi355xVm();
  return vm;
}

void ebpf_destroy(struct ebpf_vm *vm) {
  if (!vm) return;
  delete vm->impl;
  delete vm;
}

const char *ebpf_get_vm_name(struct ebpf_vm *vm) { return vm->vm_name.c_str(); }

bool ebpf_toggle_bounds_check(struct ebpf_vm *vm, bool enable) {
  bool prev = vm->impl->bounds_check;
  vm->impl->bounds_check = enable;
  return prev;
}

void ebpf_set_error_print(struct ebpf_vm *vm, int (*error_printf)(FILE *, const char *, ...)) {
  vm->impl->error_print = error_printf;
}

int ebpf_register(struct ebpf_vm *vm, unsigned int index, const char *name, void *fn) {
  return vm->impl->register_external_function(index, name ? name : "", fn);
}

int ebpf_load(struct ebpf_vm *vm, const void *code, uint32_t code_len, char **errmsg) {
  int err = vm->impl->load_code(code, code_len);
  if (err < 0 && errmsg) *errmsg = strdup(vm->impl->error.c_str());
  return err;
}

void ebpf_unload_code(struct ebpf_vm *vm) { vm->impl->unload(); }

int ebpf_exec(const struct ebpf_vm *vm, void *mem, size_t mem_len, uint64_t *bpf_return_value) {
  return vm->impl->exec_one(mem, mem_len, bpf_return_value);
}

ebpf_jit_fn ebpf_compile(struct ebpf_vm *vm, char **errmsg) {
  vm->impl->error = "mi355x is a device interpreter: use ebpf_exec / ebpf_exec_batch";
  if (errmsg) *errmsg = strdup(vm->impl->error.c_str());
  return nullptr;
}

// compat_ubpf.cpp:239-241 -> ubpf_set_unwind_function_index: a call of
// helper idx that returns 0 ends the program with r0 = 0 (interp.hip R_CALL)
// (idx is a ubpf helper id, the id register_external_function gave it)
int ebpf_set_unwind_function_index(struct ebpf_vm *vm, unsigned int idx) {
  if (idx >= 64) return -1;  // ubpf's MAX_EXT_FUNCS
  vm->impl->unwind_idx = (int)idx;
  return 0;
}

int ebpf_set_pointer_secret(struct ebpf_vm *vm, uint64_t secret) {
  (void)vm;
  (void)secret;
  return -1;
}

void ebpf_set_lddw_helpers(struct ebpf_vm *vm, uint64_t (*map_by_fd)(uint32_t), uint64_t (*map_by_idx)(uint32_t),
                           uint64_t (*map_val)(uint64_t), uint64_t (*var_addr)(uint32_t),
                           uint64_t (*code_addr)(uint32_t)) {
  LddwHelpers &l = vm->impl->lddw;
  l.map_by_fd = map_by_fd ? map_by_fd : nullptr;
  l.map_by_idx = map_by_idx;
  l.map_val = map_val;
  l.var_addr = var_addr;
  l.code_addr = code_addr;
}

ebpf_jit_fn ebpf_load_aot_object(struct ebpf_vm *vm, const void *buf, size_t buf_len) {
  (void)buf;
  (void)buf_len;
  vm->impl->error = "AOT objects are not supported by the mi355x interpreter";
  return nullptr;
}

int ebpf_exec_batch(const struct ebpf_vm *vm, const struct ebpf_batch *batch) {
  if (!vm) return -1;
  return vm->impl->exec_batch(batch);
}

int ebpf_set_ctx_kind(struct ebpf_vm *vm, uint32_t ctx_kind) {
  if (ctx_kind > EBPF_CTX_UPROBE) return -1;
  vm->impl->ctx_kind = ctx_kind;
  return 0;
}

// ---- runtime glue ----------------------------------------------------------
int bpftime_amd_register_default_helpers(struct ebpf_vm *vm) {
  // kernel helper group + shm maps group subset (bpf_helper.cpp:1177-1401)
  static const struct {
    unsigned id;
    const char *name;
  } h[] = {{8, "bpf_get_smp_processor_id"}, {28, "bpf_csum_diff"},    {44, "bpf_xdp_adjust_head"},
           {65, "bpf_xdp_adjust_tail"},      {5, "bpf_ktime_get_ns"}, {7, "bpf_get_prandom_u32"},
           {131, "bpf_ringbuf_reserve"},     {132, "bpf_ringbuf_submit"}, {133, "bpf_ringbuf_discard"},
           {130, "bpf_ringbuf_output"},      {12, "bpf_tail_call"},
           {1, "bpf_map_lookup_elem"},       {2, "bpf_map_update_elem"}, {3, "bpf_map_delete_elem"},
           {58, "bpf_override_return"},      {187, "bpf_set_retval"},
           {14, "bpf_get_current_pid_tgid"},
           {87, "bpf_map_push_elem"},        {88, "bpf_map_pop_elem"},   {89, "bpf_map_peek_elem"},
           {4, "bpf_probe_read"},            {112, "bpf_probe_read_user"}, {113, "bpf_probe_read_kernel"},
           {45, "bpf_probe_read_str"},       {114, "bpf_probe_read_user_str"},
           {115, "bpf_probe_read_kernel_str"}, {182, "bpf_strncmp"},
           {15, "bpf_get_current_uid_gid"},  {16, "bpf_get_current_comm"},
           {36, "bpf_probe_write_user"},     {125, "bpf_ktime_get_boot_ns"},
           {160, "bpf_ktime_get_coarse_ns"}, {25, "bpf_perf_event_output"},
           {27, "bpf_get_stackid"},          {67, "bpf_get_stack"},
           {173, "bpf_get_func_ip"},         {174, "bpf_get_attach_cookie"}};
  int err = 0;
  for (auto &e : h) err |= ebpf_register(vm, e.id, e.name, nullptr);
  // ... and bpf_trace_printk once the host enabled it (bpftime_amd_enable_trace_printk)
  if (rt().trace_printk_on.load()) err |= ebpf_register(vm, 6, "bpf_trace_printk", nullptr);
  return err ? -1 : 0;
}

struct ebpf_vm *bpftime_amd_prog_instantiate(int prog_fd, char **errmsg) {
  Runtime &r = rt();
  if (prog_fd < 0 || prog_fd >= (int)kMaxFds || r.kind[prog_fd] != HKind::PROG) {
    if (errmsg) *errmsg = strdup("not a prog fd");
    return nullptr;
  }
  std::vector<uint8_t> insns = r.progs[prog_fd].insns;
  int type = r.progs[prog_fd].type;
  ebpf_vm *vm = ebpf_create("mi355x");
  bpftime_amd_register_default_helpers(vm);
  if (type == BPFTIME_AMD_PROG_TYPE_XDP) vm->impl->ctx_kind = CTX_XDP;
  if (type == BPFTIME_AMD_PROG_TYPE_TRACEPOINT) vm->impl->ctx_kind = CTX_SYSCALL;
  if (ebpf_load(vm, insns.data(), (uint32_t)insns.size(), errmsg) < 0) {
    ebpf_destroy(vm);
    return nullptr;
  }
  return vm;
}

int bpftime_amd_vm_info(const struct ebpf_vm *vm, uint32_t *stack_size, int *big_stack, uint32_t *fused_rmw,
                        uint32_t *n_insns) {
  if (!vm || !vm->impl->loaded) return -1;
  auto im = vm->impl->image();
  if (stack_size) *stack_size = im->prog.stack_size;
  if (big_stack) *big_stack = im->prog.big_stack;
  if (fused_rmw) *fused_rmw = im->prog.fused_rmw;
  if (n_insns) *n_insns = (uint32_t)im->prog.prog.size();
  return 0;
}

int bpftime_amd_vm_fast_info(const struct ebpf_vm *vm, uint32_t ctx_kind, uint32_t *specialized) {
  if (!vm || !vm->impl->loaded) return -1;
  auto im = vm->impl->image();
  if (specialized) *specialized = ctx_kind == CTX_XDP ? im->fx.specialized : im->fr.specialized;
  return 0;
}

const char *bpftime_amd_vm_fast_handler(const struct ebpf_vm *vm, uint32_t ctx_kind, uint32_t pc) {
  if (!vm || !vm->impl->loaded) return nullptr;
  auto im = vm->impl->image();
  const FastForm &f = ctx_kind == CTX_XDP ? im->fx : im->fr;
  if (pc >= f.fast.size() || f.fast[pc].hoff < 4) return nullptr;
  return fop_name((f.fast[pc].hoff - 4) / 4);
}

int bpftime_amd_vm_counter_info(const struct ebpf_vm *vm, uint32_t ctx_kind, uint32_t *deferred, uint32_t *direct) {
  if (!vm || !vm->impl->loaded) return -1;
  auto im = vm->impl->image();
  const FastForm &f = ctx_kind == CTX_XDP ? im->fx : im->fr;
  uint32_t nd = 0, nn = 0;
  for (size_t i = 0; i < f.add_site.size(); i++)
    if (f.add_site[i]) ((f.fast[i].w1 & FW_NODEFER) ? nn : nd)++;
  if (deferred) *deferred = nd;
  if (direct) *direct = nn;
  return 0;
}

int bpftime_amd_vm_last_launch(const struct ebpf_vm *vm, struct bpftime_amd_launch_info *out) {
  if (!vm || !out) return -1;
  std::lock_guard<std::mutex> g(vm->impl->last_mu);
  if (!vm->impl->last.block) return -1;
  *out = vm->impl->last;
  return 0;
}

void bpftime_amd_set_step_limit(struct ebpf_vm *vm, uint64_t limit) { vm->impl->step_limit = limit; }

int bpftime_amd_vm_set_task(struct ebpf_vm *vm, const char *comm, const uint64_t *uid_gid) {
  if (!vm) return -1;
  if (comm && strnlen(comm, 64) > 63) return -1;  // (the VM unchanged)
  std::lock_guard<std::mutex> g(vm->impl->task_mu);
  if (comm) {
    memset(vm->impl->task_comm, 0, sizeof(vm->impl->task_comm));
    strncpy(vm->impl->task_comm, comm, 63);
  }
  if (uid_gid) vm->impl->task_uid_gid = *uid_gid;
  return 0;
}

int bpftime_amd_vm_set_attach(struct ebpf_vm *vm, uint64_t func_ip, uint64_t cookie) {
  if (!vm) return -1;
  std::lock_guard<std::mutex> g(vm->impl->task_mu);
  vm->impl->attach_func_ip = func_ip;
  vm->impl->attach_cookie = cookie;
  return 0;
}

int bpftime_amd_vm_get_task(const struct ebpf_vm *vm, char *comm, uint64_t *uid_gid) {
  if (!vm) return -1;
  std::lock_guard<std::mutex> g(vm->impl->task_mu);
  if (comm) memcpy(comm, vm->impl->task_comm, 64);
  if (uid_gid) *uid_gid = vm->impl->task_uid_gid;
  return 0;
}

int bpftime_amd_enable_trace_printk(int on) {
  const bool was = rt().trace_printk_on.exchange(on != 0);
  return was ? 1 : 0;
}

int64_t bpftime_amd_trace_read(struct bpftime_amd_trace_line *lines, uint64_t max_lines, char *text,
                               uint64_t text_cap, uint64_t *lost) {
  TraceLog &t = trace_log();
  std::lock_guard<std::mutex> g(t.mu);
  if (!t.d) return -1;
  if (hipDeviceSynchronize() != hipSuccess) return -1;  // the batches still writing records first
  uint64_t hdr[2] = {0, 0};
  if (hipMemcpy(hdr, t.d, sizeof(hdr), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  const uint64_t stored = hdr[0] < t.cap ? hdr[0] : t.cap;
  if (lost) *lost += hdr[1];
  if (hdr[1] && hipMemset(t.d + 8, 0, 8) != hipSuccess) return -1;
  uint64_t want = stored > t.consumed ? stored - t.consumed : 0;
  if (!lines || !text) max_lines = 0;
  if (want > max_lines) want = max_lines;
  int64_t delivered = 0;
  uint64_t used = 0;
  std::vector<TraceRec> recs;
  const uint64_t kChunk = 4096;
  bool full = false;
  for (uint64_t at = 0; at < want && !full; at += kChunk) {
    const uint64_t k = std::min(kChunk, want - at);
    recs.resize(k);
    if (hipMemcpy(recs.data(), t.d + kTraceHdrBytes + (t.consumed + at) * kTraceRecBytes, k * kTraceRecBytes,
                  hipMemcpyDeviceToHost) != hipSuccess)
      return -1;
    for (uint64_t j = 0; j < k; j++) {
      char line[1024];
      const int len = trace_format(recs[j], line, sizeof(line));
      if (len < 0 || used + (uint64_t)len + 1 > text_cap) {  // only lines that fit whole
        full = true;
        break;
      }
      memcpy(text + used, line, (size_t)len + 1);
      lines[delivered].unit = recs[j].unit;
      lines[delivered].text_off = (uint32_t)used;
      lines[delivered].text_len = (uint32_t)len;
      used += (uint64_t)len + 1;
      delivered++;
    }
  }
  t.consumed += (uint64_t)delivered;
  if (t.consumed >= stored) {  // fully consumed: the tickets start over
    if (hipMemset(t.d, 0, 8) != hipSuccess) return -1;
    t.consumed = 0;
  }
  return delivered;
}

float bpftime_amd_last_batch_ms(struct ebpf_vm *vm) {
  Mi355xVm *v = vm ? vm->impl : nullptr;
  float ms = -1.f;
  if (!v || !v->ev_t0 || !v->ev_t1 || hipEventSynchronize(v->ev_t1) != hipSuccess ||
      hipEventElapsedTime(&ms, v->ev_t0, v->ev_t1) != hipSuccess)
    return -1.f;
  return ms;
}

const char *bpftime_amd_vm_error(const struct ebpf_vm *vm) { return vm->impl->error.c_str(); }

// ---- experiment counters (BPFTIME_AMD_DBG 512) ----------------------------
int bpftime_amd_dbg_counters(uint64_t *out, int n, int reset) {
  uint64_t *d = bpftime_amd::dbg_counts();
  if (!d || !out || n < 0) return -1;
  if (n > kDbgCounts) n = kDbgCounts;
  if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(out, d, 8 * n, hipMemcpyDeviceToHost) != hipSuccess)
    return -1;
  if (reset && hipMemset(d, 0, 8 * kDbgCounts) != hipSuccess) return -1;
  return n;
}

// ---- device utilities ------------------------------------------------------
int bpftime_amd_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}
int bpftime_amd_set_device(int dev) { return hipSetDevice(dev) == hipSuccess ? 0 : -1; }
int bpftime_amd_hip_runtime_version(void) {
  int v = 0;
  return hipRuntimeGetVersion(&v) == hipSuccess ? v : -1;
}
void *bpftime_amd_dev_alloc(uint64_t bytes) {
  void *p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
  return p;
}
void bpftime_amd_dev_free(void *p) {
  if (p) hipFree(p);
}
int bpftime_amd_memcpy_htod(void *dst, const void *src, uint64_t bytes) {
  return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
}
int bpftime_amd_memcpy_dtoh(void *dst, const void *src, uint64_t bytes) {
  return hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
int bpftime_amd_memcpy_htod_async(void *dst, const void *src, uint64_t bytes, void *stream) {
  return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream) == hipSuccess ? 0 : -1;
}
int bpftime_amd_memcpy_dtoh_async(void *dst, const void *src, uint64_t bytes, void *stream) {
  return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream) == hipSuccess ? 0 : -1;
}
void *bpftime_amd_stream_create(void) {
  hipStream_t s = nullptr;
  if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return nullptr;
  return (void *)s;
}
void bpftime_amd_stream_destroy(void *stream) {
  if (stream) hipStreamDestroy((hipStream_t)stream);
}
int bpftime_amd_stream_sync(void *stream) {
  return hipStreamSynchronize((hipStream_t)stream) == hipSuccess ? 0 : -1;
}
int bpftime_amd_memset(void *dst, int v, uint64_t bytes) { return hipMemset(dst, v, bytes) == hipSuccess ? 0 : -1; }
int bpftime_amd_sync(void) { return hipDeviceSynchronize() == hipSuccess ? 0 : -1; }
void *bpftime_amd_host_alloc(uint64_t bytes) {
  void *p = nullptr;
  if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
  return p;
}
void bpftime_amd_host_free(void *p) {
  if (p) hipHostFree(p);
}
void *bpftime_amd_event_create(void) {
  hipEvent_t e;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return (void *)e;
}
void bpftime_amd_event_destroy(void *ev) {
  if (ev) hipEventDestroy((hipEvent_t)ev);
}
int bpftime_amd_event_record(void *ev, void *stream) {
  return hipEventRecord((hipEvent_t)ev, (hipStream_t)stream) == hipSuccess ? 0 : -1;
}
int bpftime_amd_stream_wait_event(void *stream, void *ev) {
  return hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)ev, 0) == hipSuccess ? 0 : -1;
}
float bpftime_amd_event_elapsed_ms(void *start, void *stop) {
  float ms = -1;
  if (hipEventSynchronize((hipEvent_t)stop) != hipSuccess) return -1;
  if (hipEventElapsedTime(&ms, (hipEvent_t)start, (hipEvent_t)stop) != hipSuccess) return -1;
  return ms;
}

}  // extern "C"
