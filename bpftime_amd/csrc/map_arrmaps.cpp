// bpftime_amd: ARRAY_OF_MAPS maps (runtime/src/bpf_map/userspace/
// map_in_maps.hpp over array_map.cpp, and the ARRAY_OF_MAPS cases of
// map_handler.cpp: lookup :214-218, update :365-373, next key :519-523, delete
// :680-688, create :934-940).  An array of int32 map fds: a program's lookup
// yields the slot's fd as the inner map's "pointer" (map_in_maps.hpp:25-30),
// which it hands to the next map helper as r1.  bpf_map_attr has no
// inner_map_fd and the reference ignores one (bpftime_shm_internal.cpp:889),
// so the slots are untyped: any int may be stored, and what a slot names is
// looked at only when a program is launched (vm_upkeep.cpp inner_launch_check).
//
// The slots in the arena are the only copy the device reads.  MapRec::
// inner_slots mirrors them on the host for the launch walk; every host write
// goes to both, after the device has finished what it was running: a launch
// that names the map never overlaps a change of its slots, so the walk's view
// of them is the kernel's.
#include "../../include/bpftime_amd.h"
#include "map_ops.hpp"

namespace bpftime_amd {

static int arrmaps_create(Runtime &, MapRec &m) {
  // map_handler.cpp:934-940: array_map_of_maps_impl(memory, max_entries), an
  // array_map_impl(memory, sizeof(int), max_entries) -- the attr's value_size
  // does not size it
  m.d.value_size = 4;
  m.bytes = 4ull * m.max_entries;
  m.inner_slots.assign(m.max_entries, 0);
  return 0;
}

// NOT the reference's elem_lookup (map_in_maps.hpp:25-30), which dereferences
// array_map_impl::elem_lookup's nullptr for an out-of-range key and returns
// the map id itself as the pointer its syscall path then reads the value
// through.  Here: a 4-byte copy of the slot (zero-padded to the attr's
// value_size, which BPF_MAP_LOOKUP_ELEM copies out), NULL / ENOENT out of range.
static const void *arrmaps_lookup(MapRec &m, int, const void *key) {
  uint32_t k;
  memcpy(&k, key, 4);
  if (k >= m.max_entries) {
    errno = ENOENT;
    return nullptr;
  }
  std::vector<uint8_t> &buf = tl_lookup_buf;
  buf.assign(m.value_size > 4 ? m.value_size : 4, 0);
  memcpy(buf.data(), &m.inner_slots[k], 4);
  return buf.data();
}

// array_map.cpp:37-55 on a 4-byte value (from_syscall: map_handler.cpp:365-373);
// the value is not checked against the fd table
static long arrmaps_update(MapRec &m, int, const void *key, const void *value, uint64_t flags) {
  const uint64_t b = flags & 0xffffffffull;
  if (b != 0 && b != 1 && b != 2) {  // map_common_def.hpp:83-94
    errno = EINVAL;
    return -1;
  }
  uint32_t k;
  memcpy(&k, key, 4);
  if (k < m.max_entries && flags == 1) {
    errno = EEXIST;
    return -1;
  }
  if (k >= m.max_entries) {
    errno = E2BIG;
    return -1;
  }
  int32_t v;
  memcpy(&v, value, 4);
  // launches that may be reading the slots finish first (any stream)
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpy((void *)(m.d.data + 4ull * k), &v, 4, hipMemcpyHostToDevice) != hipSuccess) return -1;
  m.inner_slots[k] = v;
  return 0;
}

static long arrmaps_erase(MapRec &, int, const void *) {
  errno = EINVAL;  // array_map.cpp:57-63 (map_handler.cpp:680-688)
  return -1;
}

static int arrmaps_next_key(MapRec &m, int, const void *key, void *next_key) {  // array_map.cpp:65-81
  uint32_t k = 0;
  if (key) memcpy(&k, key, 4);
  if (!key || k >= m.max_entries) {
    uint32_t z = 0;
    memcpy(next_key, &z, 4);
    return 0;
  }
  if (k == m.max_entries - 1) {
    errno = ENOENT;
    return -1;
  }
  k++;
  memcpy(next_key, &k, 4);
  return 0;
}

const MapOps kArrayOfMapsOps = {
    arrmaps_create, arrmaps_lookup, arrmaps_update, arrmaps_erase, arrmaps_next_key,
    /*percpu=*/false, /*counter_line=*/false, /*lru_stamps=*/false, /*prog_shadow=*/false, /*lookup_index=*/false,
    map_no_push, map_no_pop, map_no_peek};

// after bpftime_amd_map_restore wrote the slots: the mirror follows the arena
int arrmaps_pull(MapRec &m) {
  m.inner_slots.assign(m.max_entries, 0);
  if (!m.max_entries) return 0;
  return hipMemcpy(m.inner_slots.data(), (void *)m.d.data, 4ull * m.max_entries, hipMemcpyDeviceToHost) == hipSuccess
             ? 0
             : -1;
}

}  // namespace bpftime_amd
