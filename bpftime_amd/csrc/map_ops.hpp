// bpftime_amd: what the host side of the maps shares -- the per-type
// operations table the generic front ends (maps.cpp) dispatch through, and
// the helpers the family files (map_*.cpp) have in common.
#pragma once
#include <errno.h>
#include <string.h>

#include <vector>

#include "runtime.hpp"

namespace bpftime_amd {
#pragma GCC visibility push(hidden)  // internal to the library

// One record per map type; no entry is null (a type without an operation
// answers in its own entry).  Every operation sets errno when it fails.
struct MapOps {
  // geometry and byte counts of a new map (m.d, m.bytes, m.lpm)
  int (*create)(Runtime &, MapRec &);
  // the value, valid until the thread's next lookup on any map
  const void *(*lookup)(MapRec &, int fd, const void *key);
  long (*update)(MapRec &, int fd, const void *key, const void *value, uint64_t flags);
  long (*erase)(MapRec &, int fd, const void *key);
  int (*next_key)(MapRec &, int fd, const void *key, void *next_key);
  // the syscall side moves every CPU's value (map_handler.cpp:69-84)
  bool percpu;
  // what bpftime_maps_create puts behind the slots: a 128-B counter line;
  // + a u64 stamp per bucket (the map joins Runtime::lru_maps); a second
  // copy of the slots, both INVALID_ENTRY (-1); a hash lookup index
  bool counter_line, lru_stamps, prog_shadow, lookup_index;
  // bpf_map_push / pop / peek_elem (map_handler.cpp:1378-1468): QUEUE, STACK
  // and BLOOM_FILTER; every other type's entries answer -ENOTSUP (map_no_*)
  long (*push_elem)(MapRec &, const void *value, uint64_t flags);
  long (*pop_elem)(MapRec &, void *value);
  long (*peek_elem)(MapRec &, void *value);
};
long map_no_push(MapRec &, const void *, uint64_t);
long map_no_pop(MapRec &, void *);
long map_no_peek(MapRec &, void *);
const MapOps *map_ops(uint32_t type);  // nullptr: no such map type
extern const MapOps kArrayOps, kPercpuArrayOps, kHashOps, kPercpuHashOps, kLruHashOps, kLpmTrieOps, kProgArrayOps,
    kRingbufOps, kBloomFilterOps, kQueueOps, kStackOps, kArrayOfMapsOps, kPerfEventArrayOps, kStackTraceOps;

// the one lookup buffer of a thread, shared by every map type
extern thread_local std::vector<uint8_t> tl_lookup_buf;

inline uint64_t user_value_size(const MapRec &m) {
  return map_ops(m.type)->percpu ? (uint64_t)m.value_size * m.d.ncpu : m.value_size;
}

// bpftime_hash_map.hpp:14-38
inline uint64_t next_prime(uint64_t n) {
  auto is_prime = [](uint64_t v) {
    if (v <= 1) return false;
    if (v <= 3) return true;
    if (v % 2 == 0 || v % 3 == 0) return false;
    for (uint64_t i = 5; i * i <= v; i += 6)
      if (v % i == 0 || v % (i + 2) == 0) return false;
    return true;
  };
  while (!is_prime(n)) ++n;
  return n;
}

inline uint64_t hash_bytes(const void *key, uint32_t n) {
  uint64_t h = 0;
  for (uint32_t i = 0; i < n; i++) h = h * 31 + ((const uint8_t *)key)[i];
  return h;
}

inline MapRec *map_of(int fd) {
  Runtime &r = rt();
  if (fd < 0 || fd >= (int)kMaxFds || r.kind[fd] != HKind::MAP) {
    errno = ENOENT;
    return nullptr;
  }
  return &r.maps[fd];
}

// --- device slot helpers (hash maps) ---
inline bool read_slot(const MapRec &m, uint64_t idx, std::vector<uint8_t> &buf) {
  buf.resize(m.d.slot_size);
  return hipMemcpy(buf.data(), (void *)(m.d.data + idx * m.d.slot_size), m.d.slot_size,
                   hipMemcpyDeviceToHost) == hipSuccess;
}
inline bool write_slot(const MapRec &m, uint64_t idx, const std::vector<uint8_t> &buf) {
  return hipMemcpy((void *)(m.d.data + idx * m.d.slot_size), buf.data(), m.d.slot_size,
                   hipMemcpyHostToDevice) == hipSuccess;
}
// the u64 at `off` in the counter line (0: the element count)
inline uint64_t read_word(const MapRec &m, uint64_t off) {
  uint64_t c = 0;
  hipMemcpy(&c, (void *)(m.d.count_addr + off), 8, hipMemcpyDeviceToHost);
  return c;
}
inline void write_word(const MapRec &m, uint64_t off, uint64_t c) {
  hipMemcpy((void *)(m.d.count_addr + off), &c, 8, hipMemcpyHostToDevice);
}
inline uint64_t read_count(const MapRec &m) { return read_word(m, 0); }
inline void write_count(const MapRec &m, uint64_t c) { write_word(m, 0, c); }

// map_hash.cpp: the slot layout of the hash families (LRU_HASH shares it),
// next_prime(want_buckets) buckets of state word, key at 8, value_bytes
// 8-aligned behind it
int hash_geometry(MapRec &m, uint64_t want_buckets, uint64_t value_bytes);
// probe like bpftime_hash_map::elem_lookup; returns bucket or -1
int64_t host_hash_find(const MapRec &m, const void *key, std::vector<uint8_t> &slot, int64_t *first_empty);

// map_queue.cpp: a QUEUE / STACK map's element count (tail - head)
uint64_t qs_count(const MapRec &m);

// map_arrmaps.cpp: an ARRAY_OF_MAPS (or PERF_EVENT_ARRAY) map's host mirror
// (MapRec::inner_slots) read back from the arena, after a restore wrote the slots
int arrmaps_pull(MapRec &m);

// map_perfarr.cpp: a new PERF_EVENT_ARRAY map's slots in the arena set to -1
int perfarr_init(MapRec &m);

// map_stacktrace.cpp: a new STACK_TRACE map's claim words in the arena set to "none"
int stacktrace_init(MapRec &m);

// map_lpm.cpp: the LPM half of Runtime::prepare_ix (its arguments; the caller
// holds the runtime lock)
int lpm_prepare_launch(Runtime &r, uint64_t units, const std::vector<int> &lpm_written, uint32_t lpm_update_sites,
                       bool lpm);

// what close and reset free of a map: an ARRAY map's host view
// (map_array.cpp), an LPM trie's device flat table (map_lpm.cpp)
void drop_host_view(Runtime &r, int fd);
void lpm_drop_flat(MapRec &m);

#pragma GCC visibility pop

}  // namespace bpftime_amd
