// bpftime_amd: the process-wide runtime (runtime.hpp) -- the device arena and
// map table, fd allocation and the kind predicates, close and reset.
#include <errno.h>
#include <stdlib.h>

#include "../../include/bpftime_amd.h"
#include "map_ops.hpp"

namespace bpftime_amd {

Runtime &rt() {
  static Runtime *r = new Runtime();
  return *r;
}

void set_error(const std::string &e) { rt().last_error = e; }

int Runtime::ensure_device() {
  if (d_maptab) return 0;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) {
    set_error("no HIP device");
    return -1;
  }
  device = dev;
  const char *mb = getenv("BPFTIME_AMD_ARENA_MB");
  arena_size = (uint64_t)(mb ? atoll(mb) : 1024) << 20;  // (288 GB of HBM: two 64-MiB staged rings and more fit)
  if (hipMalloc((void **)&arena, arena_size) != hipSuccess) {
    set_error("hipMalloc(arena) failed");
    arena = nullptr;
    return -1;
  }
  if (hipMemset(arena, 0, arena_size) != hipSuccess) return -1;
  // (the map table, then the perf table: common.hpp DPerf)
  if (hipMalloc((void **)&d_maptab, (sizeof(DMap) + sizeof(DPerf)) * kMaxFds) != hipSuccess) {
    set_error("hipMalloc(map table) failed");
    return -1;
  }
  if (hipMemset(d_maptab, 0, (sizeof(DMap) + sizeof(DPerf)) * kMaxFds) != hipSuccess) return -1;
  perf_dirty = true;  // (perf records may be older than the device)
  arena_used = 0;
  return 0;
}

uint64_t Runtime::arena_alloc(uint64_t bytes) {
  uint64_t off = (arena_used + 255) & ~255ull;
  if (off + bytes > arena_size) return 0;
  arena_used = off + bytes;
  return (uint64_t)(uintptr_t)arena + off;
}

int Runtime::push_map(int fd) {
  return hipMemcpy(d_maptab + fd, &maps[fd].d, sizeof(DMap), hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
}

// The whole perf table from the records: 32 KiB, only when a record changed
// since the last upload.  Launches that may still run read only the entries
// of rings they write, which a ring's lifetime keeps unchanged.
int Runtime::push_perfs() {
  if (!perf_dirty) return 0;
  if (ensure_device() < 0) return -1;
  std::vector<DPerf> t(kMaxFds, DPerf{});
  for (uint32_t fd = 0; fd < kMaxFds; fd++) {
    if (kind[fd] != HKind::PERF || perfs[fd].type != 1) continue;
    t[fd].soft = 1;
    t[fd].ring = perfs[fd].ring;
    t[fd].data_bytes = perfs[fd].ring_bytes;
  }
  if (hipMemcpy((void *)(d_maptab + kMaxFds), t.data(), sizeof(DPerf) * kMaxFds, hipMemcpyHostToDevice) != hipSuccess)
    return -1;
  perf_dirty = false;
  return 0;
}

int alloc_fd(int fd) {
  Runtime &r = rt();
  if (fd < 0) {
    for (fd = 3; fd < (int)kMaxFds && r.kind[fd] != HKind::NONE; fd++) {
    }
  }
  if (fd < 0 || fd >= (int)kMaxFds || r.kind[fd] != HKind::NONE) {
    errno = EBADF;
    return -1;
  }
  return fd;
}

}  // namespace bpftime_amd

using namespace bpftime_amd;

extern "C" {

const char *bpftime_amd_last_error(void) { return rt().last_error.c_str(); }

void bpftime_amd_set_ncpu(uint32_t ncpu) { rt().ncpu = ncpu ? ncpu : 1; }
uint32_t bpftime_amd_get_ncpu(void) { return rt().ncpu; }

int bpftime_find_minimal_unused_fd(void) {
  std::lock_guard<std::mutex> g(rt().mu);
  return alloc_fd(-1);
}

int bpftime_is_map_fd(int fd) { return fd >= 0 && fd < (int)kMaxFds && rt().kind[fd] == HKind::MAP; }
int bpftime_is_prog_fd(int fd) { return fd >= 0 && fd < (int)kMaxFds && rt().kind[fd] == HKind::PROG; }
int bpftime_is_perf_event_fd(int fd) { return fd >= 0 && fd < (int)kMaxFds && rt().kind[fd] == HKind::PERF; }

void bpftime_close(int fd) {
  Runtime &r = rt();
  int detach = 0, udetach = 0;
  {
    std::lock_guard<std::mutex> g(r.mu);
    if (fd < 0 || fd >= (int)kMaxFds) return;
    r.prog_gen++;
    if (r.kind[fd] == HKind::MAP) {
      drop_host_view(r, fd);
      lpm_drop_flat(r.maps[fd]);
      r.lru_maps.erase(fd);
      r.lpm_dev_dirty.erase(fd);
      if (r.maps[fd].lpm) r.lpm_maps--;
      r.maps[fd] = MapRec();
      r.push_map(fd);
    } else if (r.kind[fd] == HKind::PROG) {
      r.progs[fd] = ProgRec();
    } else if (r.kind[fd] == HKind::LINK) {
      detach = r.links[fd].attach_id;
      udetach = r.links[fd].uprobe_id;
      r.links[fd] = LinkRec();
    } else if (r.kind[fd] == HKind::PERF) {
      // (its ring goes with the record; the arena's bytes come back at reset)
      r.perfs[fd] = PerfRec();
      r.perf_dirty = true;
    }
    r.kind[fd] = HKind::NONE;
  }
  if (detach) bpftime_amd_syscall_detach(detach);  // a perf link: its syscall attachment
  if (udetach) bpftime_amd_uprobe_detach(udetach);  // ... or its bound uprobe attachment
}

void bpftime_amd_reset(void) {
  Runtime &r = rt();
  std::lock_guard<std::mutex> g(r.mu);
  std::vector<int> detach;
  for (uint32_t i = 0; i < kMaxFds; i++) {
    if (r.kind[i] == HKind::MAP) {
      drop_host_view(r, (int)i);
      lpm_drop_flat(r.maps[i]);
    }
    if (r.kind[i] == HKind::LINK && r.links[i].attach_id) detach.push_back(r.links[i].attach_id);
    r.kind[i] = HKind::NONE;
    r.maps[i] = MapRec();
    r.lru_maps.erase((int)i);
    r.lpm_dev_dirty.erase((int)i);
    r.progs[i] = ProgRec();
    r.links[i] = LinkRec();
    r.perfs[i] = PerfRec();
  }
  r.lpm_maps = 0;
  (void)detach;
  syscall_detach_all();  // the link-made attachments and the direct ones
  uprobe_detach_all();
  if (r.d_maptab) hipMemset(r.d_maptab, 0, (sizeof(DMap) + sizeof(DPerf)) * kMaxFds);
  if (r.dump_buf) hipFree(r.dump_buf);  // (bpftime_amd_map_dump's calls are synchronous: nothing uses it)
  r.dump_buf = nullptr;
  r.dump_bytes = 0;
  r.perf_dirty = false;  // (no perf record is left, and the table says so)
  r.arena_used = 0;
  r.trace_printk_on = false;
  r.prog_gen++;  // tail-call images linked before the reset relink
}

}  // extern "C"
