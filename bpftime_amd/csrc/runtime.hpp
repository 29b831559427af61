// bpftime_amd: process-wide runtime state (device map registry, prog/link
// records).  Mirrors the role of bpftime's handler_manager in shared memory
// (runtime/src/handler/handler_manager.hpp:84-133) for one GPU per process.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "common.hpp"

struct ebpf_vm;  // include/ebpf-vm.h

namespace bpftime_amd {

struct MapRec {
  std::string name;
  uint32_t type = 0, key_size = 0, value_size = 0, max_entries = 0;
  uint64_t flags = 0;
  DMap d{};
  uint64_t bytes = 0;  // storage bytes at d.data
  uint64_t ix_addr = 0;    // hash lookup index storage (common.hpp ix_pos), 0 = none
  bool ix_valid = false;   // d.ix = ix_addr while the index holds exactly the reachable keys
  std::shared_ptr<struct LpmTrie> lpm;  // LPM_TRIE: the authoritative host trie (lpm_trie.hpp)
  // LPM_TRIE: the device flat table of a 4-byte-key trie (LpmTrie::flat;
  // DMap.ix), 0 = none; freed when the map goes (map_lpm.cpp lpm_drop_flat)
  void *lpm_flat = nullptr;
  uint64_t lpm_flat_bytes = 0;
  // LPM_TRIE: an ORDERED batch's device update ran out of the node pool;
  // every host op on the trie and every launch naming a trie reports it
  // (ENOMEM) until bpftime_amd_map_ack_error
  bool lpm_pool_out = false;
  // ARRAY_OF_MAPS: the host's copy of the slots (map_arrmaps.cpp keeps it equal
  // to the arena's).  The launch walk (vm_upkeep.cpp inner_launch_check) reads the
  // inner fds here, never from device memory
  // (PERF_EVENT_ARRAY: the same mirror of its perf event fds, map_perfarr.cpp)
  std::vector<int32_t> inner_slots;
  // BPF_MAP_CREATE attributes as given (BPF_OBJ_GET_INFO_BY_FD reports them)
  uint32_t ifindex = 0, btf_vmlinux_value_type_id = 0, btf_id = 0, btf_key_type_id = 0, btf_value_type_id = 0;
  uint64_t map_extra = 0;
  uint32_t kernel_bpf_map_id = 0;
  // host view of an ARRAY map (bpftime_get_array_map_raw_data, the mmap a
  // libbpf loader makes of .bss / .data): page-aligned host bytes kept
  // coherent with the device copy at batch boundaries (map_array.cpp)
  uint8_t *host_view = nullptr;
  uint64_t host_view_bytes = 0;
  std::vector<uint8_t> host_shadow;  // the bytes last exchanged with the device
};

// A perf event record (bpf_perf_event_handler, runtime/src/handler/
// perf_event_handler.hpp:161-215): what a link's target_fd names.  Only a
// syscall sys_enter / sys_exit tracepoint drives anything here (the syscall
// replay dispatch); the other kinds are kept as records, so state that holds
// them imports, exports and links unchanged.
struct PerfRec {
  int type = 2;                // bpf_event_type (bpftime_shm.hpp:48-64); 2 = PERF_TYPE_TRACEPOINT
  int pid = -1;
  bool enabled = false;        // perf_event_enable / _disable (a flag only, as in the reference)
  int32_t tracepoint_id = -1;  // tracepoint: the kernel id (tracepoints.cpp), or -1 when made from
  int64_t sys_nr = -1;         // ... a syscall number (bpftime_amd_perf_event_syscall; -1: every syscall)
  uint64_t offset = 0, ref_ctr_off = 0;  // uprobe / uretprobe / uprobe override
  std::string module;
  int cpu = 0;                 // software perf event
  int32_t sample_type = 0;
  int64_t config = 0;
  // software perf event: its device ring (common.hpp DPerf), 0 until
  // bpftime_amd_perf_event_mmap gives it one (handles.cpp)
  uint64_t ring = 0, ring_bytes = 0;
};

struct ProgRec {
  std::string name;
  std::vector<uint8_t> insns;  // raw 8-byte ebpf_inst records
  int type = 0;
};

struct LinkRec {
  uint32_t prog_fd = 0, target = 0, attach_type = 0, flags = 0;
  bool perf = false;  // target is a perf event record (handles.cpp link_perf)
  int attach_id = 0;  // a perf link to a sys_enter / sys_exit tracepoint: its syscall attachment (syscall_dispatch.cpp)
  // bpf_link_handler::attach_cookie (link_handler.hpp:20): what
  // bpf_get_attach_cookie answers while the program runs for this link
  bool has_cookie = false;
  uint64_t cookie = 0;
  int uprobe_id = 0;  // a perf link to a uprobe event bound to a function: its attachment (uprobe_dispatch.cpp)
};

enum class HKind : uint8_t { NONE, MAP, PROG, LINK, PERF };

struct Runtime {
  std::mutex mu;
  std::vector<HKind> kind = std::vector<HKind>(kMaxFds, HKind::NONE);
  std::vector<MapRec> maps = std::vector<MapRec>(kMaxFds);
  std::vector<ProgRec> progs = std::vector<ProgRec>(kMaxFds);
  std::vector<LinkRec> links = std::vector<LinkRec>(kMaxFds);
  std::vector<PerfRec> perfs = std::vector<PerfRec>(kMaxFds);
  std::set<int> host_views;     // ARRAY maps with a host view
  // before a launch: host writes to host views reach the device; after a
  // synchronous batch (or bpftime_amd_map_msync): device bytes reach them
  int host_views_push();
  int host_views_pull();
  int device = -1;
  DMap *d_maptab = nullptr;     // device table indexed by fd
  uint8_t *arena = nullptr;     // device map arena
  uint64_t arena_size = 0, arena_used = 0;
  uint32_t ncpu = 64;
  std::string last_error;
  uint64_t prog_gen = 1;        // bumped when a prog, a prog array or its contents change
  // bpf_trace_printk (6) on the device: off until bpftime_amd_enable_trace_printk(1)
  // (and again after bpftime_amd_reset).  While off the helper is no default
  // helper and a program that calls it is refused at load as before: a host
  // that never asked for the record log does not get one.
  std::atomic<bool> trace_printk_on{false};

  int ensure_device();          // lazily picks the current device, allocates arena + table
  uint64_t arena_alloc(uint64_t bytes);
  int push_map(int fd);         // upload DMap entry for fd
  // The device's perf table (common.hpp DPerf) lives behind the map table.
  // perf_dirty: a perf record was made, given a ring, closed or reset since
  // the table was uploaded; a launch of a program that calls
  // bpf_perf_event_output uploads it first (push_perfs; the caller holds mu)
  bool perf_dirty = false;
  int push_perfs();
  std::set<int> ix_stale;       // hash maps whose lookup index needs a rebuild
  std::set<int> lpm_stale;      // LPM tries whose device replica needs an upload
  std::set<int> lpm_flat_pending;  // IPv4 LPM tries whose flat table is not built (DMap.ix = 0: walk)
  // LPM tries an ORDERED batch of a program that writes them may have
  // changed on the device: the replica is authoritative until the host pulls
  // it back (map_lpm.cpp lpm_pull) before its next operation on the trie
  std::set<int> lpm_dev_dirty;
  // before a launch: a program that can delete invalidates every hash
  // lookup index; any other rebuilds the stale ones.  `lpm_written`: the LPM
  // tries the launch's program may update / delete (ORDERED batches only):
  // their lookups walk the replica (no flat table) while they change
  // `lpm`: the program names an LPM trie (loader.cpp lpm_write_sites); a
  // launch of one that does not leaves the tries as they are (their next
  // user uploads them, under the LPM launch lock)
  int prepare_ix(bool may_delete, uint64_t units, const std::vector<int> &lpm_written = {},
                 uint32_t lpm_update_sites = 0, bool lpm = true);
  // launches that may still run: one whose hash lookups use the block LDS
  // lookup cache (a found slot is trusted for the rest of the launch), one of
  // a program that can delete.  A cached launch never overlaps a deletion
  // (a program's, on any stream, or the host's): whichever comes second
  // waits for the device first (vm_upkeep.cpp LaunchUpkeep, map_hash.cpp hash_erase)
  std::atomic<bool> lcache_inflight{false}, deleter_inflight{false};
  // LPM tries (vm_upkeep.cpp LaunchUpkeep): launches of a runtime holding any are
  // prepared and launched under lpm_launch_mu; a launch that may write a
  // trie (ORDERED) waits for every launch that may still touch one, and any
  // launch after a writer waits for it
  std::mutex lpm_launch_mu;
  std::atomic<int> lpm_maps{0};
  std::atomic<bool> lpm_inflight{false}, lpm_writer_inflight{false};
  // QUEUE / STACK maps (vm_upkeep.cpp qs_launch_check): launches that may still
  // run and add to one / remove from or peek one.  A launch that removes from
  // or peeks a map never overlaps one that adds to a map, on any stream:
  // whichever comes second waits for the device first.  An ORDERED launch
  // that touches such a map sets and honours both flags (its lane moves the
  // ends without compare-and-swap), so it overlaps no other such launch
  std::atomic<bool> qs_adder_inflight{false}, qs_taker_inflight{false};
  std::set<int> lru_maps;                // LRU_HASH maps
  std::atomic<uint64_t> lru_seq{1};      // LRU stamp sequence: launches and host-side ops (common.hpp)
  uint32_t lru_launches = 0;             // launches since the last tombstone check
  // before a launch: renumbers the LRU stamps before the sequence runs out,
  // compacts tombstone-heavy LRU tables now and then; returns the launch's
  // stamp sequence (0 on failure)
  uint64_t prepare_lru();
  // bpftime_amd_map_dump's scratch and staging (map_dump.cpp): one device
  // buffer, replaced by a larger one when a call needs more, used under mu,
  // freed by bpftime_amd_reset
  void *dump_buf = nullptr;
  uint64_t dump_bytes = 0;
};

// hash lookup index upkeep for host-side writes (map_hash.cpp)
void ix_invalidate(int fd);
// the device replica of an LPM trie an ORDERED batch wrote, back into the
// host trie (no-op unless the trie is in lpm_dev_dirty)
int lpm_pull(int fd);

Runtime &rt();
void set_error(const std::string &e);
// `fd` when it is free, the lowest free fd for -1; else -1 and EBADF
// (runtime.cpp; the caller holds the runtime lock)
__attribute__((visibility("hidden"))) int alloc_fd(int fd);

// What the syscall dispatch needs to know of a loaded VM's program
// (vm_seq.cpp): bit 0 it calls bpf_override_return / bpf_set_retval (58 /
// 187), bit 1 it may store into the memory r1 points to (its unit: the
// dispatch then runs it on a copy of the records), bit 2 it calls
// bpf_get_stackid / bpf_get_stack (27 / 67).  -1: no program loaded.
constexpr int kProgSetsRetval = 1, kProgStoresCtx = 2, kProgReadsStacks = 4;
int vm_prog_flags(const ::ebpf_vm *vm);
// Drops every syscall attachment (bpftime_amd_reset; syscall_dispatch.cpp).
void syscall_detach_all();
// The cookie of syscall attachment `id` (a cookie link's; handles.cpp): what
// bpf_get_attach_cookie answers in its callbacks.  -1: no such attachment.
int syscall_attach_set_cookie(int id, uint64_t cookie);
// Drops every uprobe attachment (bpftime_amd_reset; uprobe_dispatch.cpp).
void uprobe_detach_all();
// A loaded program's map effects (loader.hpp FastForm::map_fx, the syscall /
// raw entry form): per map fd FX_* bits and the bits that may reach any map.
// A program that calls bpf_tail_call answers for its linked image: itself and
// every target its prog arrays name at the time of the call (a launch relinks
// when a prog array changed since: a plan made from these effects holds only
// while no host thread updates the prog arrays before the dispatch's last
// launch, DESIGN.md §5 "Tail calls").  -1: no program loaded, or the image
// did not link.
int vm_map_effects(const ::ebpf_vm *vm, std::map<int32_t, uint8_t> &fx, uint8_t &any);
// Whether the loaded program calls bpf_tail_call: only the program-major
// plans run it (the thread-ordered kernels hold no tail-call frames).
bool vm_has_tail(const ::ebpf_vm *vm);
// The commute analysis of the dispatches (syscall_dispatch.cpp).  Two of the
// loaded programs may not commute when both reach one map and one writes it
// (a store, a fetching / non-add atomic, update / delete / ring calls) or adds
// to it while the other loads from its values; counter adds commute with
// counter adds (and with lookups: an add changes no key's presence), reads
// with reads.  One program may not commute with ITSELF -- the
// program-major plans run all of one thread's records in parallel lanes --
// when it writes a map other than by a bpf_map_update_elem whose flags are
// the constant BPF_NOEXIST and whose value is constant, or both adds to a map and loads from its values;
// lookup + NOEXIST init + counter add stays order-free.  Effects the loader
// cannot place reach every map.  1 with the first such pair (first == second:
// the program against itself) and the map's fd (-1: unplaced effects) in the
// non-null outs, 0 none, -1 a program is not loaded.
int first_map_conflict(const std::vector<const ::ebpf_vm *> &vms, size_t *first, size_t *second, int *map);
// Whether a loaded program may reach a QUEUE / STACK map (loader.cpp
// qs_call_sites): such a program does not commute with itself across
// records, so the syscall dispatch runs it only in ORDERED dispatches.
bool vm_touches_qs(const ::ebpf_vm *vm);
// The thread-ordered syscall dispatch's launch (interp.hip k_sys_seq):
// `progs` in the reference's order (syscall_dispatch.cpp), over n device
// records laid out as `lay`; thread t's records perm[seg[t] .. seg[t + 1])
// (null perm / seg: one thread over every record in record order).  `err`: a
// device u32 (failed callbacks).  Returns the failed-callback count with
// EBPF_BATCH_SYNC, else 0; -1 on errors (set_error).
struct SeqAttach {
  const ::ebpf_vm *vm;
  int64_t sys_nr;
  bool enter;
};
int64_t seq_dispatch(const std::vector<SeqAttach> &progs, const SysLayout &lay, uint64_t n, const uint32_t *perm,
                     const uint32_t *seg, uint64_t nseg, int64_t *out, uint32_t flags, uint32_t *err, hipStream_t s);
// A loaded VM's task identity as the thread-ordered launches compare it:
// uid_gid, then the 64 bytes of comm.  -1: no program loaded.
int vm_task_identity(const ::ebpf_vm *vm, uint64_t out[9]);
// The thread-ordered uprobe replay's launch (interp.hip k_up_seq): `progs` as
// uprobe_dispatch.cpp's running() orders them (entry attachments, then return
// ones); `recs` carries the records, their grouping (perm / seg / nseg as
// above) and out_state / out_rets, the rest is filled here.  `err` and the
// return value as seq_dispatch's.
struct USeqAttach {
  const ::ebpf_vm *vm;
  uint64_t func;
  bool at_return;
  uint8_t kind;  // common.hpp kUpPlain / kUpOverride / kUpReplace
};
int64_t useq_dispatch(const std::vector<USeqAttach> &progs, const UpSeqParams &recs, uint32_t flags, uint32_t *err,
                      hipStream_t s);

}  // namespace bpftime_amd
