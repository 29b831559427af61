// bpftime_amd: the prog, link and perf-event records (runtime.hpp).
#include <errno.h>

#include "../../include/bpftime_amd.h"
#include "perf_ring.hpp"
#include "runtime.hpp"

#include <string.h>

using namespace bpftime_amd;

extern "C" {

// ---- prog / link records ---------------------------------------------------
int bpftime_progs_create(int fd, const void *insns, size_t insn_cnt, const char *prog_name, int prog_type) {
  Runtime &r = rt();
  std::lock_guard<std::mutex> g(r.mu);
  fd = alloc_fd(fd);
  if (fd < 0) return -1;
  ProgRec p;
  p.name = prog_name ? prog_name : "";
  p.insns.assign((const uint8_t *)insns, (const uint8_t *)insns + insn_cnt * 8);
  p.type = prog_type;
  r.progs[fd] = std::move(p);
  r.kind[fd] = HKind::PROG;
  r.prog_gen++;
  return fd;
}

static int link_perf(int fd, int prog_fd, int perf_fd, int bad_errno, const uint64_t *cookie = nullptr);

// bpftime_shm_internal.cpp:566-607: only prog_fd is validated; the target of
// an XDP link is an ifindex.
int bpftime_link_create(int fd, struct bpf_link_create_args *args) {
  Runtime &r = rt();
  if (args && args->attach_type == BPFTIME_AMD_BPF_PERF_EVENT) {
    // :578-600: a perf-event link's target must be a perf event (libbpf
    // probes with target_fd -1 and expects EBADF); it attaches like
    // BPF_PROG_ATTACH (both fds checked under the runtime lock, link_perf)
    // (the cookie: perf_event.bpf_cookie, the first word of the union --
    // link_handler.hpp:25-31; the other attach types' unions hold none)
    return link_perf(fd, (int)args->prog_fd, (int)args->target_fd, EBADF, &args->attach_union[0]);
  }
  std::lock_guard<std::mutex> g(r.mu);
  if (!args) {
    errno = EINVAL;
    return -1;
  }
  if (args->prog_fd >= kMaxFds || r.kind[args->prog_fd] != HKind::PROG) {
    errno = EBADF;
    return -1;
  }
  fd = alloc_fd(fd);
  if (fd < 0) return -1;
  LinkRec l;
  l.prog_fd = args->prog_fd;
  l.target = args->target_fd;
  l.attach_type = args->attach_type;
  l.flags = args->flags;
  r.links[fd] = l;
  r.kind[fd] = HKind::LINK;
  return fd;
}

int bpftime_amd_xdp_links(int *link_fds, int *prog_fds, uint32_t *ifindexes, int max) {
  Runtime &r = rt();
  std::lock_guard<std::mutex> g(r.mu);
  int n = 0;
  for (uint32_t i = 0; i < kMaxFds; i++) {
    if (r.kind[i] != HKind::LINK || r.links[i].attach_type != BPFTIME_AMD_BPF_XDP) continue;
    if (n < max) {
      if (link_fds) link_fds[n] = (int)i;
      if (prog_fds) prog_fds[n] = (int)r.links[i].prog_fd;
      if (ifindexes) ifindexes[n] = r.links[i].target;
    }
    n++;
  }
  return n;
}

// ---- perf events + BPF_PROG_ATTACH (bpftime_shm.cpp:227-253,
// bpftime_shm_internal.cpp:212-315) ------------------------------------------
static int perf_create(int fd, const PerfRec &p) {
  Runtime &r = rt();
  std::lock_guard<std::mutex> g(r.mu);
  fd = alloc_fd(fd);
  if (fd < 0) return -1;
  r.perfs[fd] = p;
  r.kind[fd] = HKind::PERF;
  r.perf_dirty = true;  // (the device's perf table, runtime.cpp push_perfs)
  return fd;
}

int bpftime_amd_perf_event_syscall(int fd, int64_t sys_nr) {
  if (sys_nr < -1) {
    errno = EINVAL;
    return -1;
  }
  PerfRec p;
  p.sys_nr = sys_nr;
  return perf_create(fd, p);
}

// add_tracepoint (:254-264): the id is resolved when a program attaches
int bpftime_tracepoint_create(int fd, int pid, int32_t tp_id) {
  PerfRec p;
  p.pid = pid;
  p.tracepoint_id = tp_id;
  return perf_create(fd, p);
}

// add_uprobe / add_uprobe_override (:212-252): records only, nothing on this
// path probes a process
int bpftime_uprobe_create(int fd, int pid, const char *name, uint64_t offset, bool retprobe, size_t ref_ctr_off) {
  PerfRec p;
  p.type = retprobe ? 7 : 6;
  p.pid = pid;
  p.module = name ? name : "";
  p.offset = offset;
  p.ref_ctr_off = ref_ctr_off;
  return perf_create(fd, p);
}

int bpftime_amd_perf_event_record(int fd, const struct bpftime_amd_perf_event *e) {
  if (!e) {
    errno = EINVAL;
    return -1;
  }
  PerfRec p;
  p.type = e->type;
  p.pid = e->pid;
  p.enabled = e->enabled != 0;
  p.tracepoint_id = e->tracepoint_id;
  p.sys_nr = e->sys_nr;
  p.offset = e->offset;
  p.ref_ctr_off = e->ref_ctr_off;
  p.module = e->module_name ? e->module_name : "";
  p.cpu = e->cpu;
  p.sample_type = e->sample_type;
  p.config = e->config;
  return perf_create(fd, p);
}

int bpftime_amd_perf_event_get(int fd, struct bpftime_amd_perf_event *e) {
  Runtime &r = rt();
  std::lock_guard<std::mutex> g(r.mu);
  if (fd < 0 || fd >= (int)kMaxFds || r.kind[fd] != HKind::PERF || !e) {
    errno = ENOENT;
    return -1;
  }
  const PerfRec &p = r.perfs[fd];
  e->type = p.type;
  e->pid = p.pid;
  e->enabled = p.enabled;
  e->tracepoint_id = p.tracepoint_id;
  e->sys_nr = p.sys_nr;
  e->offset = p.offset;
  e->ref_ctr_off = p.ref_ctr_off;
  e->module_name = p.module.c_str();  // valid until the record changes
  e->cpu = p.cpu;
  e->sample_type = p.sample_type;
  e->config = p.config;
  return 0;
}

// ---- the ring of a software perf event --------------------------------------
// software_perf_event_buffer (perf_event_handler.cpp:235-450): a header page
// and mmap_size() data bytes, sized when the consumer mmaps the perf fd
// (ensure_mmap_buffer, :264-293); before that every output is dropped.  Here
// the ring lives in the device arena (common.hpp DPerf): the positions on a
// line each, then the data bytes.  It is made once: the reference grows the
// buffer on a larger mmap, the arena only ever hands out fresh bytes, so a
// second size is refused.
static PerfRec *soft_perf(Runtime &r, int fd) {
  if (fd < 0 || fd >= (int)kMaxFds || r.kind[fd] != HKind::PERF || r.perfs[fd].type != 1) {
    errno = EINVAL;
    return nullptr;
  }
  return &r.perfs[fd];
}

int bpftime_amd_perf_event_mmap(int perf_fd, uint64_t data_bytes) {
  Runtime &r = rt();
  std::lock_guard<std::mutex> g(r.mu);
  PerfRec *p = soft_perf(r, perf_fd);
  if (!p) {
    set_error("fd " + std::to_string(perf_fd) + " is not a software perf event");
    return -1;
  }
  if (data_bytes < 64 || (data_bytes & (data_bytes - 1))) {
    errno = EINVAL;
    set_error("Data size of a perf event buffer must be power of 2 (at least 64)");
    return -1;
  }
  if (p->ring) {
    if (p->ring_bytes == data_bytes) return 0;
    errno = EINVAL;
    set_error("perf event " + std::to_string(perf_fd) + " has a ring of " + std::to_string(p->ring_bytes) +
              " bytes: a ring cannot be resized");
    return -1;
  }
  if (r.ensure_device() < 0) return -1;
  const uint64_t base = r.arena_alloc(kPerfRingHdr + data_bytes);
  if (!base) {
    errno = ENOMEM;
    set_error("map arena exhausted (BPFTIME_AMD_ARENA_MB)");
    return -1;
  }
  if (hipMemset((void *)base, 0, kPerfRingHdr + data_bytes) != hipSuccess) return -1;
  p->ring = base;
  p->ring_bytes = data_bytes;
  r.perf_dirty = true;
  return 0;
}

int bpftime_amd_perf_event_ring_state(int perf_fd, uint64_t *head, uint64_t *tail, uint64_t *data_bytes) {
  Runtime &r = rt();
  uint64_t ring, bytes;
  {
    std::lock_guard<std::mutex> g(r.mu);
    PerfRec *p = soft_perf(r, perf_fd);
    if (!p) return -1;
    ring = p->ring;
    bytes = p->ring_bytes;
  }
  uint64_t h = 0, t = 0;
  if (ring) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpy(&h, (void *)ring, 8, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&t, (void *)(ring + kPerfTailOff), 8, hipMemcpyDeviceToHost) != hipSuccess)
      return -1;
  }
  if (head) *head = h;
  if (tail) *tail = t;
  if (data_bytes) *data_bytes = bytes;
  return 0;
}

// The consumer: the producers of queued batches finish first, as
// bpftime_amd_ringbuf_fetch has it; the walk is perf_ring.hpp's.
int64_t bpftime_amd_perf_event_fetch(int perf_fd, void *out, uint64_t cap, uint64_t *used) {
  Runtime &r = rt();
  if (used) *used = 0;
  uint64_t ring, bytes;
  {
    std::lock_guard<std::mutex> g(r.mu);
    PerfRec *p = soft_perf(r, perf_fd);
    if (!p) return -1;
    ring = p->ring;
    bytes = p->ring_bytes;
  }
  if (!ring) return 0;
  if (!out && cap) {
    errno = EINVAL;
    return -1;
  }
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  uint64_t head, tail;
  if (hipMemcpy(&head, (void *)ring, 8, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(&tail, (void *)(ring + kPerfTailOff), 8, hipMemcpyDeviceToHost) != hipSuccess)
    return -1;
  if (head == tail) return 0;
  std::vector<uint8_t> data(bytes);
  if (hipMemcpy(data.data(), (void *)(ring + kPerfRingHdr), bytes, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  uint64_t u = 0;
  const int64_t n = perf_ring_walk(data.data(), bytes, head, &tail, (uint8_t *)out, cap, &u);
  if (hipMemcpy((void *)(ring + kPerfTailOff), &tail, 8, hipMemcpyHostToDevice) != hipSuccess) return -1;
  if (used) *used = u;
  return n;
}

static int perf_enable(int fd, bool on) {  // :317-337
  Runtime &r = rt();
  std::lock_guard<std::mutex> g(r.mu);
  if (fd < 0 || fd >= (int)kMaxFds || r.kind[fd] != HKind::PERF) {
    errno = ENOENT;
    return -1;
  }
  r.perfs[fd].enabled = on;
  return 0;
}
int bpftime_perf_event_enable(int fd) { return perf_enable(fd, true); }
int bpftime_perf_event_disable(int fd) { return perf_enable(fd, false); }

// What a link to perf event p drives: 1 + the sys_enter dispatch slot for a
// syscall enter tracepoint (the global one: sys_nr -1), 0 for a record that
// runs nothing on this path (sys_exit tracepoints: the replay holds enter
// records only; uprobes, software events), -1 for a tracepoint id that does
// not resolve (the reference's attach fails there too,
// syscall_trace_attach_private_data.cpp:51-62); *enter: the sys_enter (1) or
// sys_exit (0) tracepoint
static int perf_drives(const PerfRec &p, int64_t *nr, int *enter) {
  if (p.type != 2) return 0;
  *enter = 1;
  *nr = p.sys_nr;
  if (p.tracepoint_id >= 0 && bpftime_amd_tracepoint_resolve(p.tracepoint_id, nr, enter) < 0) return -1;
  return 1;
}

// A link from prog_fd to perf_fd at `fd` (-1: a fresh one).  A link to a
// sys_enter or sys_exit tracepoint attaches the program to the syscall
// dispatch (it is instantiated: a program the device cannot load fails the
// link); any other perf target, and a tracepoint id that does not resolve
// here, gives a link record that runs nothing: the reference's
// add_bpf_link / add_bpf_prog_attach_target (bpftime_shm_internal.cpp:293-315,
// :566-607) check only the handler kinds and resolve the id when its agent
// attaches.  bad_errno: what a non-perf perf_fd or non-program prog_fd sets
// (ENOENT for BPF_PROG_ATTACH, EBADF for BPF_LINK_CREATE).  cookie: the link's
// attach cookie (null: none), handed to the syscall attachment it drives.
static int link_perf(int fd, int prog_fd, int perf_fd, int bad_errno, const uint64_t *cookie) {
  Runtime &r = rt();
  int64_t nr = -1;
  int drives, enter = 1;
  {
    std::lock_guard<std::mutex> g(r.mu);
    if (perf_fd < 0 || perf_fd >= (int)kMaxFds || r.kind[perf_fd] != HKind::PERF) {  // "Fd is not a perf fd"
      errno = bad_errno;
      return -1;
    }
    if (prog_fd < 0 || prog_fd >= (int)kMaxFds || r.kind[prog_fd] != HKind::PROG) {
      errno = bad_errno;
      return -1;
    }
    if (fd >= 0 && (fd >= (int)kMaxFds || r.kind[fd] != HKind::NONE)) {
      errno = EBADF;
      return -1;
    }
    drives = perf_drives(r.perfs[perf_fd], &nr, &enter);
  }
  int id = 0;
  if (drives > 0) {
    id = bpftime_amd_syscall_attach_ex(prog_fd, nr, enter);  // instantiates the program (outside the lock)
    if (id < 0) return -1;
    if (cookie) syscall_attach_set_cookie(id, *cookie);
  }
  std::lock_guard<std::mutex> g(r.mu);
  fd = alloc_fd(fd);
  if (fd < 0) {
    if (id) bpftime_amd_syscall_detach(id);
    return -1;
  }
  LinkRec l;
  l.prog_fd = (uint32_t)prog_fd;
  l.target = (uint32_t)perf_fd;
  l.attach_type = BPFTIME_AMD_BPF_PERF_EVENT;
  l.perf = true;
  l.attach_id = id;
  l.has_cookie = cookie != nullptr;
  l.cookie = cookie ? *cookie : 0;
  r.links[fd] = l;
  r.kind[fd] = HKind::LINK;
  return fd;
}

int bpftime_attach_perf_to_bpf(int perf_fd, int bpf_fd) { return link_perf(-1, bpf_fd, perf_fd, ENOENT); }

int bpftime_attach_perf_to_bpf_with_cookie(int perf_fd, int bpf_fd, uint64_t cookie) {
  return link_perf(-1, bpf_fd, perf_fd, ENOENT, &cookie);
}

int bpftime_amd_link_perf(int fd, int prog_fd, int perf_fd) { return link_perf(fd, prog_fd, perf_fd, ENOENT); }

int bpftime_amd_link_attached(int fd) {
  Runtime &r = rt();
  std::lock_guard<std::mutex> g(r.mu);
  if (fd < 0 || fd >= (int)kMaxFds || r.kind[fd] != HKind::LINK) return -1;
  return r.links[fd].attach_id ? 1 : 0;
}

}  // extern "C"
