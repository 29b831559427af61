// bpftime_amd: the VM behind the C ABI (include/ebpf-vm.h), shared by the
// vm_*.cpp files: the trace log, a loaded program's device image, the
// per-stream buffers, the backend class and the launch checks and upkeep.
#pragma once
#include <errno.h>
#include <hip/hip_runtime_api.h>
#include <stdlib.h>
#include <string.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "../../include/bpftime_amd.h"
#include "loader.hpp"
#include "runtime.hpp"
#include "trace_fmt.hpp"

namespace bpftime_amd {
// bpf_trace_printk's record log (trace_fmt.hpp): one per process, device
// memory of the runtime's own, made when the first program that calls helper
// 6 is loaded.  BPFTIME_AMD_TRACE_RECORDS (read once, here) sets its records.
struct TraceLog {
  std::mutex mu;
  uint8_t *d = nullptr;
  uint64_t cap = 0;
  uint64_t consumed = 0;  // records the host has delivered since the log was last empty
};
TraceLog &trace_log();   // (vm_abi.cpp)
int trace_log_ensure();

extern "C" hipError_t bpftime_amd_launch_interp(const KParams *p, uint32_t kind, bool big_stack, uint32_t grid,
                                                uint32_t ordered, uint32_t block, hipStream_t stream);
extern "C" hipError_t bpftime_amd_launch_stack_commit(const DMap *m, const StackSrc *src, uint64_t first_unit,
                                                      uint64_t count, hipStream_t stream);
extern "C" int bpftime_amd_occupancy(uint32_t kind, bool big_stack, size_t dyn_lds, bool gregs, uint32_t block,
                                    bool image);
extern "C" size_t bpftime_amd_static_lds_image(uint32_t kind, bool big_stack, bool gregs, uint32_t block, bool image);
extern "C" hipError_t bpftime_amd_launch_merge(const uint64_t *log, uint32_t log_words, uint32_t nblocks,
                                                hipStream_t stream);
extern "C" hipError_t bpftime_amd_launch_miss_merge(const uint64_t *log, const uint32_t *counts, uint32_t cap,
                                                     uint32_t nblocks, const KParams *p, uint32_t *bad,
                                                     hipStream_t stream);
extern "C" hipError_t bpftime_amd_launch_fast_xlat(uint32_t kind, bool big_stack, bool greg, bool image,
                                                   uint32_t *d_out, hipStream_t stream);
extern "C" hipError_t bpftime_amd_launch_sys_seq(const SeqParams *p, hipStream_t stream);
extern "C" hipError_t bpftime_amd_launch_up_seq(const UpSeqParams *p, hipStream_t stream);

// A loaded program in device form.  Tail-call images (common.hpp
// kTailHelper) are rebuilt when a prog array changes; a batch holds a
// reference to the image it launches, so a relink by another thread never
// frees what an exec_batch in flight is reading (hipFree waits for the
// device, so launches already queued are safe too).
struct Image {
  LoadOut prog;
  DInsn *d_prog = nullptr;
  // threaded-code forms: XDP entry (r1 = ctx) and raw/syscall entry (r1 = the
  // unit's slot) differ in the loader's pointer kinds
  FastForm fx, fr;
  int32_t *d_tail_entry = nullptr;  // prog fd -> entry pc (tail-call images)
  // the asm tier's one-load form of the same: [kMaxFds] offsets of each
  // reachable PROG_ARRAY's slots (-1: not in the image), then per slot the
  // entry pc of the program it held at link time (-1: none / not linked)
  int32_t *d_tail_slots = nullptr;
  uint32_t frame_words = 0;         // tail-call frame: header + ctx + the image's stack bytes, / 8
  uint64_t gen = 0;                 // rt().prog_gen it was linked at
  // linked FInsn arrays per launch configuration (entry form, ORDERED,
  // staged bytes, batch head): a few per program, built on first use
  std::mutex link_mu;
  std::map<std::pair<uint64_t, uint32_t>, FInsn *> links;

  ~Image() {
    if (d_prog) hipFree(d_prog);
    if (d_tail_entry) hipFree(d_tail_entry);
    if (d_tail_slots) hipFree(d_tail_slots);
    for (auto &kv : links) hipFree(kv.second);
  }
  // greg: the asm variant of the launch (k_interp G), whose handler offsets
  // the form is translated to
  const FInsn *linked(bool greg, bool xdp, uint32_t head, uint32_t stage, bool ordered, int32_t unwind_idx,
                      uint32_t lc_sets, int32_t pid_off, bool no_kldx = false, RecOffs rec = {});
  // device copy of the decoded program + both threaded forms
  int upload(LoadOut &&out, std::string &err);
};

// device buffers kept per stream: a batch's launches use them in stream
// order, batches on other streams have their own
struct StreamBufs {
  struct Buf {
    void *p = nullptr;
    uint64_t bytes = 0;
  };
  std::mutex mu;
  std::map<hipStream_t, Buf> bufs;
  ~StreamBufs() {
    for (auto &kv : bufs)
      if (kv.second.p) hipFree(kv.second.p);
  }
  void *get(hipStream_t s, uint64_t bytes) {
    std::lock_guard<std::mutex> g(mu);
    Buf &b = bufs[s];
    if (b.bytes < bytes) {
      // the stream may still run a batch that uses the old buffer
      if (b.p && (hipStreamSynchronize(s) != hipSuccess || hipFree(b.p) != hipSuccess)) return nullptr;
      b.p = nullptr;
      b.bytes = 0;
      if (hipMalloc(&b.p, bytes) != hipSuccess) return nullptr;
      b.bytes = bytes;
    }
    return b.p;
  }
};

class Mi355xVm {
 public:
  std::string error;
  // compat_ubpf.hpp:42-44 (bpftime id -> ubpf-style id)
  std::map<size_t, size_t> helper_id_map;
  std::map<size_t, std::string> helper_names;
  size_t next_helper_id = 1;
  LddwHelpers lddw;
  bool bounds_check = true;
  int (*error_print)(FILE *, const char *, ...) = nullptr;
  int unwind_idx = -1;
  uint32_t ctx_kind = CTX_RAW;
  uint64_t step_limit = 1ull << 22;
  // task identity (bpf_get_current_uid_gid / bpf_get_current_comm): the
  // reference's answers for the launching process until
  // bpftime_amd_vm_set_task; comm is zero from its NUL to the end
  uint64_t task_uid_gid = 0;
  char task_comm[64] = {};
  std::mutex task_mu;
  // the attachment this VM runs for (bpf_get_func_ip / bpf_get_attach_cookie):
  // bpftime_amd_vm_set_attach; both 0 by default (guarded by task_mu)
  uint64_t attach_func_ip = 0;
  uint64_t attach_cookie = 0;

  bool loaded = false;
  std::mutex img_mu;                 // guards img (replaced by tail-call relinks)
  std::shared_ptr<Image> img;
  std::shared_ptr<Image> image() {
    std::lock_guard<std::mutex> g(img_mu);
    return img;
  }
  // failed-unit counters, one per in-flight batch: concurrent batches on
  // different streams must not share (and re-zero) one counter
  static constexpr uint32_t kErrSlots = 64;
  uint32_t *d_err = nullptr;
  std::atomic<uint32_t> err_slot{0};
  // staging for ebpf_exec
  std::mutex stage_mu;
  uint8_t *d_stage = nullptr;
  size_t stage_size = 0;
  // bpf_tail_call: the loaded code, relinked with the prog arrays' targets
  // when rt().prog_gen moves
  std::vector<RawInsn> raw;
  bool has_tail = false;
  uint32_t base_stack = 0;  // the loaded program's own stack need (kStackSize + 1: unknown)
  std::string link_note;    // targets left out of the last image, and why
  // block-end flush logs (common.hpp kMergeGroup) and tail-call frames
  StreamBufs logs, frames, scratch, regs, misses;
  // the kernels of the last EBPF_BATCH_TIMED batch
  hipEvent_t ev_t0 = nullptr, ev_t1 = nullptr;
  // the plan of the last launch (bpftime_amd_vm_last_launch; block 0: none yet)
  std::mutex last_mu;
  bpftime_amd_launch_info last{};

  Mi355xVm() {
    // bpftime_prog.cpp:126-127 defaults, pointed at the device registry
    lddw.map_by_fd = bpftime_amd_map_ptr_by_fd;
    lddw.map_val = bpftime_amd_map_val;
    const char *sl = getenv("BPFTIME_AMD_STEP_LIMIT");
    if (sl) step_limit = strtoull(sl, nullptr, 0);
    // bpf_helper.cpp:350-355: the gid in both halves; :364-385: the basename
    // of /proc/self/exe
    task_uid_gid = ((uint64_t)getgid() << 32) | (uint64_t)getgid();
    char exe[4096];
    const ssize_t k = readlink("/proc/self/exe", exe, sizeof(exe) - 1);
    if (k > 0) {
      exe[k] = 0;
      const char *base = strrchr(exe, '/');
      strncpy(task_comm, base ? base + 1 : exe, sizeof(task_comm) - 1);
    }
  }
  void attach_into(uint64_t &func_ip, uint64_t &cookie) {
    std::lock_guard<std::mutex> g(task_mu);
    func_ip = attach_func_ip;
    cookie = attach_cookie;
  }
  void task_into(uint64_t &uid_gid, uint64_t comm[8]) {
    std::lock_guard<std::mutex> g(task_mu);
    uid_gid = task_uid_gid;
    memcpy(comm, task_comm, 64);
  }
  ~Mi355xVm() {
    if (ev_t0) hipEventDestroy(ev_t0);
    if (ev_t1) hipEventDestroy(ev_t1);
    unload();
    if (d_err) hipFree(d_err);
    if (d_stage) hipFree(d_stage);
  }
  void unload() {
    std::lock_guard<std::mutex> g(img_mu);
    img.reset();
    loaded = false;
    raw.clear();
    has_tail = false;
  }
  int register_external_function(size_t index, const std::string &name, void *fn) {
    // compat_ubpf.cpp:50-59: allocate the next id; ubpf caps helpers at 64
    size_t next_id = next_helper_id++;
    if (next_id >= 64) {
      error = "too many helpers (ubpf supports 64)";
      return -1;
    }
    helper_id_map[index] = next_id;
    helper_names[index] = name;
    (void)fn;
    return 0;
  }
  int load_code(const void *code, size_t code_len);  // (vm_image.cpp)
  int link_tail_image_locked();
  int exec_batch(const ebpf_batch *b);  // (vm_exec.cpp)
  int exec_one(void *mem, size_t mem_len, uint64_t *ret);
};

// ---- launch checks and upkeep (vm_upkeep.cpp) ---------------------------------
bool qs_launch_check(const FastForm &f, bool ordered, std::string &error, bool &adds, bool &takes);
bool st_launch_check(const FastForm &f, bool ordered, uint32_t max_depth, std::string &error,
                     std::vector<int32_t> &commit);
bool inner_launch_check(const FastForm &f, std::string &error);
bool perf_launch_prepare(const LoadOut &prog, std::string &error);
std::string lds_fit_error(uint32_t kind, bool big_stack, uint32_t stack_size, uint32_t comb_entries,
                          uint32_t lcache, bool ctx_lds, bool greg, uint32_t block, bool image, uint32_t tail_lds);

// The fences and the map upkeep around one launch, whichever kernel it is
// (k_interp, k_sys_seq, k_up_seq): what keeps concurrent launches on
// different streams correct.  Made for the launch's mode, fed each program
// form the launch runs (exec_batch: one), then before() -- the launch is
// queued -- after(), and for EBPF_BATCH_SYNC finish().  The LPM launch lock is
// held from before() to after(), and released when the object dies on an
// error return in between.
struct LaunchUpkeep {
  Runtime &r = rt();
  const bool ordered;
  bool may_delete = false, names_lpm = false, qs_adds = false, qs_takes = false, touches_lpm = false;
  uint32_t lcache = 0;  // the launch's lookup-cache sets (only exec_batch launches hold one)
  std::vector<int> lpm_w;
  uint32_t lpm_updates = 0;
  std::unique_lock<std::mutex> lpm_lk;
  std::string err;  // why the last call returned false / -1

  explicit LaunchUpkeep(bool ordered_) : ordered(ordered_), lpm_lk(rt().lpm_launch_mu, std::defer_lock) {}
  bool fail(const std::string &e) {
    err = e;
    return false;
  }
  bool add(const LoadOut &prog, const FastForm &f);
  bool before(uint64_t n, uint64_t &lru_seq);
  void after();
  int64_t finish(uint32_t *counter, hipStream_t s, const char *what);
};

uint64_t *dbg_counts();  // (vm_exec.cpp)
constexpr int kDbgCounts = 4;
extern thread_local int g_last_seq_tier;  // (vm_seq.cpp)
}  // namespace bpftime_amd

// ebpf-vm.cpp's struct ebpf_vm {vm_name; vm_instance} (bpftime_vm_compat.hpp:260-263)
struct ebpf_vm {
  std::string vm_name;
  bpftime_amd::Mi355xVm *impl;
};
