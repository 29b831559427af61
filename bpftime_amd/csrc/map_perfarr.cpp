// bpftime_amd: PERF_EVENT_ARRAY maps (runtime/src/bpf_map/userspace/
// perf_event_array_map.cpp).  An array of int32 perf event fds, -1 = empty: a
// program's bpf_perf_event_output reads the slot of its CPU and writes a
// record to that software perf event's ring (dev_helpers.hpp
// helper_perf_output).  The slots are untyped, as in the reference: any int may
// be stored, and what a slot names is looked at when a program emits.
//
// The slots in the arena are the copy the device reads.  MapRec::inner_slots
// mirrors them on the host: host lookups and the shm JSON export read the
// mirror, never device memory; every host write goes to both, after the device
// has finished what it was running.
#include "../../include/bpftime_amd.h"
#include "map_ops.hpp"

namespace bpftime_amd {

static int perfarr_create(Runtime &, MapRec &m) {
  if (m.key_size != 4 || m.value_size != 4) {  // :20-25 (the reference throws)
    errno = EINVAL;
    set_error("Key size and value size of perf_event_array must be 4");
    return -1;
  }
  m.bytes = 4ull * m.max_entries;
  m.inner_slots.assign(m.max_entries, -1);  // "Default value of fd map is -1" (:17-18)
  return 0;
}

// bpftime_maps_create zeroes the storage; the slots start at -1
int perfarr_init(MapRec &m) {
  if (!m.bytes) return 0;
  return hipMemset((void *)m.d.data, 0xff, m.bytes) == hipSuccess ? 0 : -1;
}

static bool perfarr_key(const MapRec &m, const void *key, int32_t *k) {
  memcpy(k, key, 4);
  if (*k < 0 || (uint64_t)*k >= m.max_entries) {
    errno = EINVAL;
    return false;
  }
  return true;
}

static int perfarr_store(MapRec &m, int32_t k, int32_t v) {
  // launches that may be reading the slots finish first (any stream)
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpy((void *)(m.d.data + 4ull * (uint32_t)k), &v, 4, hipMemcpyHostToDevice) != hipSuccess) return -1;
  m.inner_slots[(uint32_t)k] = v;
  return 0;
}

static const void *perfarr_lookup(MapRec &m, int, const void *key) {  // :28-36
  int32_t k;
  if (!perfarr_key(m, key, &k)) return nullptr;
  return &m.inner_slots[(uint32_t)k];
}

static long perfarr_update(MapRec &m, int, const void *key, const void *value, uint64_t) {  // :38-49, flags unread
  int32_t k, v;
  if (!perfarr_key(m, key, &k)) return -1;
  memcpy(&v, value, 4);
  return perfarr_store(m, k, v);
}

static long perfarr_erase(MapRec &m, int, const void *key) {  // :51-60
  int32_t k;
  if (!perfarr_key(m, key, &k)) return -1;
  return perfarr_store(m, k, -1);
}

static int perfarr_next_key(MapRec &m, int, const void *key, void *next_key) {  // :62-81
  int32_t k = 0;
  if (!key) {
    memcpy(next_key, &k, 4);
    return 0;
  }
  memcpy(&k, key, 4);
  if ((uint64_t)((int64_t)k + 1) == m.max_entries) {  // the last key (before the range check, as there)
    errno = ENOENT;
    return -1;
  }
  if (k < 0 || (uint64_t)k >= m.max_entries) {
    errno = EINVAL;
    return -1;
  }
  k++;
  memcpy(next_key, &k, 4);
  return 0;
}

const MapOps kPerfEventArrayOps = {
    perfarr_create, perfarr_lookup, perfarr_update, perfarr_erase, perfarr_next_key,
    /*percpu=*/false, /*counter_line=*/false, /*lru_stamps=*/false, /*prog_shadow=*/false, /*lookup_index=*/false,
    map_no_push, map_no_pop, map_no_peek};

}  // namespace bpftime_amd
