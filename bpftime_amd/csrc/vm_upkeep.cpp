// bpftime_amd: what a launch checks about the maps its program names, and the
// fences and map upkeep around it (LaunchUpkeep): one protocol for exec_batch
// and the thread-ordered dispatches.
#include "vm_impl.hpp"

namespace bpftime_amd {
// QUEUE / STACK maps in a launch of the program form `f` (loader.cpp
// qs_call_sites).  The device's parallel push / pop / peek are correct only
// while one map sees one kind of access during a launch (dev_helpers.hpp
// qs_group): each map must be add-only (helpers 87 / 2 with flags proven 0),
// remove-only (88 / 3) or peek-only (89 / 1).  Anything else -- mixed kinds on
// one map, a push with flags that are not proven 0, helpers 87 / 88 / 89 on a
// map register the loader cannot resolve while any QUEUE / STACK map exists --
// runs only in EBPF_BATCH_ORDERED batches (one lane, the reference's
// sequence).  `adds` / `takes`: the launch may add to such a map / remove from
// or peek one (Runtime::qs_adder_inflight).  An ORDERED launch that touches
// such a map counts as both, whatever its call sites do: its one lane moves
// `head` / `tail` with a read and an unconditional exchange, not with the
// parallel paths' compare-and-swap, so it must overlap no other launch that
// touches a QUEUE / STACK -- not even one of its own kind.
bool qs_launch_check(const FastForm &f, bool ordered, std::string &error, bool &adds, bool &takes) {
  adds = takes = false;
  if (f.qs_sites.empty()) return true;
  Runtime &r = rt();
  static const char *const kRule =
      ": in a parallel batch each QUEUE / STACK map must be add-only (push / update with flags 0), remove-only "
      "(pop / delete) or peek-only (peek / lookup); this program runs only in EBPF_BATCH_ORDERED batches";
  auto name = [](uint32_t h) {
    switch (h) {
      case 1: return "bpf_map_lookup_elem";
      case 2: return "bpf_map_update_elem";
      case 3: return "bpf_map_delete_elem";
      case 87: return "bpf_map_push_elem";
      case 88: return "bpf_map_pop_elem";
    }
    return "bpf_map_peek_elem";
  };
  auto is_qs = [&](int32_t fd) {
    return fd >= 0 && fd < (int32_t)kMaxFds && r.kind[fd] == HKind::MAP && qs_type(r.maps[fd].type);
  };
  bool any_qs = false;
  for (uint32_t fd = 0; fd < kMaxFds && !any_qs; fd++) any_qs = is_qs((int32_t)fd);
  if (!any_qs) return true;
  std::map<int32_t, std::pair<uint32_t, uint32_t>> modes;  // fd -> {kinds seen, the first site's helper}
  for (const FastForm::QsSite &q : f.qs_sites) {
    const uint32_t kind = (q.helper == 87 || q.helper == 2) ? 1u : (q.helper == 88 || q.helper == 3) ? 2u : 4u;
    if (q.fd < 0) {
      adds = takes = true;
      if (ordered) continue;
      error = std::string(name(q.helper)) + " on a map fd the loader cannot resolve (a QUEUE / STACK map exists)" +
              kRule;
      return false;
    }
    if (!is_qs(q.fd)) continue;
    if (ordered) {
      adds = takes = true;
      continue;
    }
    (kind == 1 ? adds : takes) = true;
    const std::string at = std::string(name(q.helper)) + " on " +
                           (r.maps[q.fd].type == MT_STACK ? "STACK" : "QUEUE") + " map fd " + std::to_string(q.fd);
    if (kind == 1 && !q.flags0) {
      error = at + " with flags not proven 0" + kRule;
      return false;
    }
    auto it = modes.find(q.fd);
    if (it == modes.end()) {
      modes[q.fd] = {kind, q.helper};
    } else if (it->second.first != kind) {
      error = at + " beside " + name(it->second.second) + " on the same map" + kRule;
      return false;
    }
  }
  return true;
}

// QUEUE / STACK launches on different streams: one that removes from or peeks
// a map never overlaps one that adds to a map, and an ORDERED one (both, see
// above) overlaps no other -- whichever comes second waits for the device
// first (the lookup cache's rule, Runtime::lcache_inflight)
static bool qs_launch_fence(bool adds, bool takes) {
  Runtime &r = rt();
  if ((takes && r.qs_adder_inflight.load()) || (adds && r.qs_taker_inflight.load())) {
    if (hipDeviceSynchronize() != hipSuccess) return false;
    r.qs_adder_inflight = false;
    r.qs_taker_inflight = false;
  }
  return true;
}

// STACK_TRACE maps in a launch of the program form `f` (loader.cpp
// qs_call_sites, FastForm::st_sites).  Every batch: a map the program names must
// hold the batch's deepest stack (value_size / 8 >= stack_max_depth).  A
// parallel batch leaves the map as the reference's serial run would only
// while a filled slot never changes (dev_helpers.hpp helper_stackid,
// stack_commit.hip): BPF_F_REUSE_STACKID makes the stored stack depend on the
// order of the calls, and a program-side lookup or delete would see or undo a
// fill that is not stored yet.  Such programs run only in EBPF_BATCH_ORDERED
// batches.  `commit`: the maps a parallel launch's bpf_get_stackid may claim
// slots of, which k_stack_commit visits afterwards.
bool st_launch_check(const FastForm &f, bool ordered, uint32_t max_depth, std::string &error,
                            std::vector<int32_t> &commit) {
  commit.clear();
  if (f.st_sites.empty()) return true;
  Runtime &r = rt();
  static const char *const kRule =
      ": in a parallel batch a STACK_TRACE map only takes bpf_get_stackid calls whose flags are a proven constant "
      "without BPF_F_REUSE_STACKID; this program runs only in EBPF_BATCH_ORDERED batches";
  for (const FastForm::StSite &q : f.st_sites) {
    if (q.fd < 0 || q.fd >= (int32_t)kMaxFds || r.kind[q.fd] != HKind::MAP || r.maps[q.fd].type != MT_STACK_TRACE)
      continue;  // closed since the load: the device answers -EINVAL / NULL
    const MapRec &m = r.maps[q.fd];
    if (m.value_size / 8 < max_depth) {
      error = "STACK_TRACE map fd " + std::to_string(q.fd) + " holds " + std::to_string(m.value_size / 8) +
              " frames per stack (value_size / 8) < stack_max_depth " + std::to_string(max_depth);
      return false;
    }
    if (ordered) continue;
    const std::string at = " on STACK_TRACE map fd " + std::to_string(q.fd);
    if (q.helper == 1 || q.helper == 3) {
      error = std::string(q.helper == 1 ? "bpf_map_lookup_elem" : "bpf_map_delete_elem") + at + kRule;
      return false;
    }
    if (q.helper == 27 && !q.flags_ok) {
      error = "bpf_get_stackid" + at + " with flags not proven free of BPF_F_REUSE_STACKID" + kRule;
      return false;
    }
    if (q.helper == 27 && std::find(commit.begin(), commit.end(), q.fd) == commit.end()) commit.push_back(q.fd);
  }
  return true;
}

// ARRAY_OF_MAPS: the maps a launch of the program form `f` reaches without
// naming them in an lddw -- whatever the slots of the outer maps it names
// (loader.cpp, FastForm::outer_maps) hold.  The walk reads the host mirror of
// the slots (MapRec::inner_slots), never device memory; a host write of a slot
// waits for the device first (map_arrmaps.cpp), so the mirror is what the
// kernel will read.  It runs before any kernel is launched.
//
// Inner ARRAY, PERCPU_ARRAY, HASH and PERCPU_HASH maps are accepted in every
// batch mode.  Everything a launch prepares for them is prepared for every
// such map of the runtime, named or not: the hash lookup indexes (Runtime::
// prepare_ix rebuilds every stale one and, for a program that calls
// map_delete_elem -- LoadOut::may_delete is a property of the program, not of
// a map -- invalidates them all), the element counts and index inserts (the
// device's own, dev_helpers.hpp hash_find), the host views (host_views_push /
// _pull) and the deleter / lookup-cache fences (keyed on the program).  The
// other types have per-launch work keyed on the maps a program names (LPM
// launch lock, replica upload and flat table; QUEUE / STACK access kinds and
// fences; ring staging; prog-array linking; the Bloom and LRU helpers'
// call-site routing), which an unnamed map would miss: a slot that holds one
// refuses the launch.  A slot that names no live map (0, garbage, a closed
// fd) is fine: the device answers NULL / -1 for it.
bool inner_launch_check(const FastForm &f, std::string &error) {
  if (f.outer_maps.empty()) return true;
  Runtime &r = rt();
  std::lock_guard<std::mutex> g(r.mu);
  for (const int32_t ofd : f.outer_maps) {
    if (ofd < 0 || ofd >= (int32_t)kMaxFds || r.kind[ofd] != HKind::MAP || r.maps[ofd].type != MT_ARRAY_OF_MAPS)
      continue;  // closed since the load: the device answers NULL
    const std::vector<int32_t> &slots = r.maps[ofd].inner_slots;
    for (size_t i = 0; i < slots.size(); i++) {
      const int32_t ifd = slots[i];
      if (ifd < 0 || ifd >= (int32_t)kMaxFds || r.kind[ifd] != HKind::MAP) continue;
      const uint32_t t = r.maps[ifd].type;
      if (t == MT_ARRAY || t == MT_PERCPU_ARRAY || t == MT_HASH || t == MT_PERCPU_HASH) continue;
      error = "ARRAY_OF_MAPS map fd " + std::to_string(ofd) + " slot " + std::to_string(i) + " holds map fd " +
              std::to_string(ifd) + " of type " + std::to_string(t) +
              ": inner maps must be ARRAY, PERCPU_ARRAY, HASH or PERCPU_HASH";
      return false;
    }
  }
  return true;
}

// bpf_perf_event_output: the device's perf table (common.hpp DPerf) as the
// records stand now -- which fds are software perf events, and their rings --
// before a launch of a program that calls the helper is queued.  Under the
// runtime lock; nothing is uploaded when no record changed since the last
// upload.  The slots of the perf arrays are the device's own copy, which a
// host write changes only after the device has finished (map_perfarr.cpp).
bool perf_launch_prepare(const LoadOut &prog, std::string &error) {
  if (!prog.perf_output) return true;
  Runtime &r = rt();
  std::lock_guard<std::mutex> g(r.mu);
  if (r.push_perfs() < 0) {
    error = "perf table upload failed";
    return false;
  }
  return true;
}

// The message of a launch whose block does not fit the CU's LDS: the parts
// of its dynamic LDS (common.hpp dyn_lds_for) and the kernel's static LDS
std::string lds_fit_error(uint32_t kind, bool big_stack, uint32_t stack_size, uint32_t comb_entries,
                          uint32_t lcache, bool ctx_lds, bool greg, uint32_t block, bool image, uint32_t tail_lds) {
  const size_t lanes = (size_t)block * ((kind == CTX_XDP && ctx_lds ? lane_stride(kXdpCtxBytes) : 0) +
                                        (big_stack ? 0 : lane_stride(stack_size)) +
                                        tail_lds_lane_bytes(tail_lds));
  const size_t dyn = dyn_lds_for(kind, big_stack, stack_size, comb_entries, lcache, ctx_lds, block, tail_lds);
  const size_t stat = bpftime_amd_static_lds_image(kind, big_stack, greg, block, image);
  return "launch does not fit the CU's LDS: " + std::to_string(dyn + stat) + " bytes per " +
         std::to_string(block) + "-lane block (lanes' ctx, stacks and tail-call frames " + std::to_string(lanes) +
         ", lookup cache " + std::to_string(lcache) + " sets " + std::to_string(lcache_bytes(lcache)) +
         ", launch constants " + std::to_string(kTenvBytes) + ", combining table " + std::to_string(comb_entries) +
         " entries " + std::to_string(comb_bytes(comb_entries)) + ", static " + std::to_string(stat) + ") > " +
         std::to_string(kCuLds) + " (check BPFTIME_AMD_COMB_ENTRIES / BPFTIME_AMD_LCACHE_SETS)";
}

// One program form of the launch.  Program-side LPM trie updates / deletes:
// the device changes a trie only in ORDERED batches (one lane, the
// reference's order: dev_helpers.hpp lpm_update), the host takes the replica
// back afterwards (lpm_pull)
bool LaunchUpkeep::add(const LoadOut &prog, const FastForm &f) {
  may_delete |= prog.may_delete;
  names_lpm |= f.names_lpm;
  for (const auto &w : f.lpm_writes) {
    if (!ordered)
      return fail(std::string(w.first == 2 ? "bpf_map_update_elem" : "bpf_map_delete_elem") +
                  " on LPM_TRIE map fd " + std::to_string(w.second) +
                  ": program-side LPM trie writes run only in EBPF_BATCH_ORDERED batches");
    lpm_updates += w.first == 2;
    if (std::find(lpm_w.begin(), lpm_w.end(), w.second) == lpm_w.end()) lpm_w.push_back(w.second);
  }
  return true;
}

// The map upkeep before the launch is queued, for the union of its programs
bool LaunchUpkeep::before(uint64_t n, uint64_t &lru_seq) {
  if (!qs_launch_fence(qs_adds, qs_takes)) return fail("device synchronize failed");
  // the lookup cache trusts a found slot for the whole launch: no deletion
  // may run beside it (Runtime::lcache_inflight)
  if ((lcache && r.deleter_inflight.load()) || (may_delete && r.lcache_inflight.load())) {
    if (hipDeviceSynchronize() != hipSuccess) return fail("device synchronize failed");
    r.lcache_inflight = false;
    r.deleter_inflight = false;
  }
  // LPM tries: a launch of a program that writes one (ORDERED) never
  // overlaps another launch that may touch one, on any stream -- whichever
  // comes second waits for the device -- and the launch and its marking of
  // the tries as device-written happen under one lock, so a concurrent
  // launch's preparation sees them
  // (only launches of programs that name a trie: others need
  // neither the lock nor the in-flight marks, and a writer waits for them)
  touches_lpm = r.lpm_maps.load() > 0 && names_lpm;
  if (touches_lpm) {
    lpm_lk.lock();
    if ((!lpm_w.empty() && r.lpm_inflight.load()) || r.lpm_writer_inflight.load()) {
      if (hipDeviceSynchronize() != hipSuccess) return fail("device synchronize failed");
      r.lpm_inflight = false;
      r.lpm_writer_inflight = false;
    }
  }
  if (r.prepare_ix(may_delete, n, lpm_w, lpm_updates, names_lpm) < 0) {
    // (an LPM trie's report names itself; else the index rebuild failed)
    const std::string le = bpftime_amd_last_error() ? bpftime_amd_last_error() : "";
    return fail(le.rfind("LPM_TRIE", 0) == 0 ? le : "hash lookup index rebuild failed");
  }
  lru_seq = r.prepare_lru();
  if (!lru_seq) return fail("LRU table upkeep failed");
  if (r.host_views_push() < 0) return fail("host view upload failed");  // host writes to mmap'd array maps first
  return true;
}

// (the launch is queued)
void LaunchUpkeep::after() {
  if (lcache) r.lcache_inflight = true;
  if (may_delete) r.deleter_inflight = true;
  if (qs_adds) r.qs_adder_inflight = true;
  if (qs_takes) r.qs_taker_inflight = true;
  if (!lpm_w.empty()) {
    std::lock_guard<std::mutex> g(r.mu);
    for (const int fd : lpm_w) r.lpm_dev_dirty.insert(fd);
    r.lpm_writer_inflight = true;
  }
  if (touches_lpm) {
    r.lpm_inflight = true;
    lpm_lk.unlock();
  }
}

// EBPF_BATCH_SYNC: the failed units (`counter`: the launch's device u32), the
// host views and written tries pulled; -1 with `err` (`what` sync failed: ...;
// empty: the pull set the runtime's error itself).  A program-side LPM update
// that ran out of the device node pool fails the launch here (map_lpm.cpp
// lpm_pull; asynchronous launches report it at the trie's next use)
int64_t LaunchUpkeep::finish(uint32_t *counter, hipStream_t s, const char *what) {
  uint32_t failed = 0;
  hipError_t e = hipMemcpyAsync(&failed, counter, 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess || r.host_views_pull() < 0) {
    fail(std::string(what) + (e != hipSuccess ? hipGetErrorString(e) : "host view pull"));
    return -1;
  }
  for (const int fd : lpm_w) {
    std::lock_guard<std::mutex> g(r.mu);
    if (lpm_pull(fd) < 0) {
      err.clear();
      return -1;
    }
  }
  return failed;
}

}  // namespace bpftime_amd
