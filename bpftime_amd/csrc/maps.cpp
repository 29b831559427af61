// bpftime_amd: device-resident maps -- the generic host-side operations.
//
// Map semantics (syscall side, from_syscall = true) follow
// runtime/src/handler/map_handler.cpp:109-330 over
//   array_map.cpp:19-81, fix_hash_map.cpp:16-84 + bpftime_hash_map.hpp,
//   per_cpu_array_map.cpp:97-145, per_cpu_hash_map.cpp:141-216,
//   map_in_maps.hpp (map_arrmaps.cpp), perf_event_array_map.cpp (map_perfarr.cpp),
//   stack_trace_map.cpp (map_stacktrace.cpp),
// with storage in one device arena (HBM) whose layout is described by the
// DMap records the interpreter reads (csrc/common.hpp).  Host-side ops copy
// the touched slots over PCIe: they are control-plane operations and must not
// race a running batch (the reference's syscall path likewise takes the map
// lock, map_handler.hpp:45-62).
//
// Each map type's operations live in its family file (map_*.cpp) behind one
// MapOps record (map_ops.hpp); the front ends here only dispatch.
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/bpftime_amd.h"
#include "lpm_trie.hpp"
#include "map_ops.hpp"

namespace bpftime_amd {

thread_local std::vector<uint8_t> tl_lookup_buf;

const MapOps *map_ops(uint32_t type) {
  switch (type) {
    case MT_ARRAY: return &kArrayOps;
    case MT_PERCPU_ARRAY: return &kPercpuArrayOps;
    case MT_HASH: return &kHashOps;
    case MT_PERCPU_HASH: return &kPercpuHashOps;
    case MT_LRU_HASH: return &kLruHashOps;
    case MT_LPM_TRIE: return &kLpmTrieOps;
    case MT_PROG_ARRAY: return &kProgArrayOps;
    case MT_RINGBUF: return &kRingbufOps;
    case MT_BLOOM_FILTER: return &kBloomFilterOps;
    case MT_QUEUE: return &kQueueOps;
    case MT_STACK: return &kStackOps;
    case MT_ARRAY_OF_MAPS: return &kArrayOfMapsOps;
    case MT_PERF_EVENT_ARRAY: return &kPerfEventArrayOps;
    case MT_STACK_TRACE: return &kStackTraceOps;
  }
  return nullptr;
}

// map_handler.cpp:1404-1407, :1431-1434, :1463-1466: a map type without the
// operation
long map_no_push(MapRec &, const void *, uint64_t) { return -ENOTSUP; }
long map_no_pop(MapRec &, void *) { return -ENOTSUP; }
long map_no_peek(MapRec &, void *) { return -ENOTSUP; }

}  // namespace bpftime_amd

using namespace bpftime_amd;

extern "C" {

int bpftime_maps_create(int fd, const char *name, struct bpf_map_attr attr) {
  Runtime &r = rt();
  std::lock_guard<std::mutex> g(r.mu);
  if (r.ensure_device() < 0) return -1;
  fd = alloc_fd(fd);
  if (fd < 0) return -1;
  MapRec m;
  m.name = name ? name : "";
  m.type = (uint32_t)attr.type;
  m.key_size = attr.key_size;
  m.value_size = attr.value_size;
  m.max_entries = attr.max_ents;
  m.flags = attr.flags;
  m.ifindex = attr.ifindex;
  m.btf_vmlinux_value_type_id = attr.btf_vmlinux_value_type_id;
  m.btf_id = attr.btf_id;
  m.btf_key_type_id = attr.btf_key_type_id;
  m.btf_value_type_id = attr.btf_value_type_id;
  m.kernel_bpf_map_id = attr.kernel_bpf_map_id;
  m.map_extra = attr.map_extra;
  DMap &d = m.d;
  d.type = m.type;
  d.key_size = m.key_size;
  d.value_size = m.value_size;
  d.max_entries = m.max_entries;
  d.ncpu = r.ncpu;
  const MapOps *ops = map_ops(m.type);
  if (!ops) {
    errno = EINVAL;
    set_error("unsupported map type " + std::to_string(m.type));
    return -1;
  }
  if (ops->create(r, m) < 0) return -1;
  // hash maps: a 128-B counter line; LRU maps: + a u64 stamp per bucket
  uint64_t extra = ops->counter_line ? 128 + (ops->lru_stamps ? 8ull * d.nbuckets : 0) : 0;
  // PROG_ARRAY: a second copy of the slots after them, where device-side
  // map_lookup_elem hands out the looked-up fd (the reference returns a
  // thread-local copy, prog_array.cpp:113-143: a write through the pointer
  // must not change the array)
  const uint64_t shadow = ops->prog_shadow ? m.bytes : 0;
  uint64_t base = r.arena_alloc(m.bytes + extra + shadow + 8);
  if (!base) {
    errno = ENOMEM;
    set_error("map arena exhausted (BPFTIME_AMD_ARENA_MB)");
    return -1;
  }
  d.data = base;
  d.count_addr = extra ? base + ((m.bytes + 127) & ~127ull) : 0;
  if (hipMemset((void *)base, 0, m.bytes + extra + shadow + 8) != hipSuccess) return -1;
  if (ops->prog_shadow) {  // every slot INVALID_ENTRY (-1)
    if (hipMemset((void *)base, 0xff, 2 * m.bytes) != hipSuccess) return -1;
    r.prog_gen++;
  }
  if (m.type == MT_PERF_EVENT_ARRAY && perfarr_init(m) < 0) return -1;  // every slot -1
  if (m.type == MT_STACK_TRACE && stacktrace_init(m) < 0) return -1;    // every slot unclaimed
  if (m.lpm) {  // empty replica: root = -1, no nodes or entries, the pool's capacity
    const uint32_t hdr[4] = {~0u, 0, 0, m.lpm->cap};
    if (hipMemcpy((void *)base, hdr, 16, hipMemcpyHostToDevice) != hipSuccess) return -1;
  }
  if (ops->lookup_index && !getenv("BPFTIME_AMD_NO_HASH_INDEX")) {
    // lookup index (common.hpp ix_pos): a power of two >= 2 x buckets, so
    // it is at most half full; an empty table's index is empty and valid.
    // After it the bucket bitmap (common.hpp ix_bitmap), the bits past the
    // last bucket set
    // (keyed indexes, common.hpp ix_key_stride: the keys beside the
    // entries; config 3's 65,536 flows take 262,144 positions, 5 MiB with
    // their keys, of which a lookup touches one key line as the reference
    // probe touches one bucket line)
    const uint32_t ks = ix_key_stride(m.key_size);
    uint64_t isz = 64;
    while (isz < 2 * (uint64_t)d.nbuckets) isz <<= 1;
    const uint64_t words = ix_bitmap_words(d.nbuckets);
    uint64_t ix = isz <= (1ull << 32) ? r.arena_alloc((4 + ks) * isz + 8 * words) : 0;
    const uint64_t pad = d.nbuckets % 64 ? ~0ull << (d.nbuckets % 64) : 0;
    if (ix && hipMemset((void *)ix, 0, (4 + ks) * isz + 8 * words) == hipSuccess &&
        hipMemcpy((void *)(ix_bitmap(ix, (uint32_t)(isz - 1), m.key_size) + 8 * (words - 1)), &pad, 8,
                  hipMemcpyHostToDevice) == hipSuccess) {
      m.ix_addr = ix;
      m.ix_valid = true;
      d.ix = ix;
      d.ix_mask = (uint32_t)(isz - 1);
    }
  }
  r.maps[fd] = m;
  r.kind[fd] = HKind::MAP;
  if (ops->lru_stamps) r.lru_maps.insert(fd);
  if (m.lpm) r.lpm_maps++;
  if (r.push_map(fd) < 0) return -1;
  return fd;
}

uint32_t bpftime_map_value_size_from_syscall(int fd) {
  MapRec *m = map_of(fd);
  return m ? (uint32_t)user_value_size(*m) : 0;  // map_handler.cpp:69-84
}

const void *bpftime_map_lookup_elem(int fd, const void *key) {
  MapRec *m = map_of(fd);
  return m ? map_ops(m->type)->lookup(*m, fd, key) : nullptr;
}

long bpftime_map_update_elem(int fd, const void *key, const void *value, uint64_t flags) {
  MapRec *m = map_of(fd);
  return m ? map_ops(m->type)->update(*m, fd, key, value, flags) : -1;
}

long bpftime_map_delete_elem(int fd, const void *key) {
  MapRec *m = map_of(fd);
  return m ? map_ops(m->type)->erase(*m, fd, key) : -1;
}

int bpftime_map_get_next_key(int fd, const void *key, void *next_key) {
  MapRec *m = map_of(fd);
  return m ? map_ops(m->type)->next_key(*m, fd, key, next_key) : -1;
}

// bpftime_shm.cpp:168-200 over map_handler.cpp:1378-1468
long bpftime_map_push_elem(int fd, const void *value, uint64_t flags) {
  MapRec *m = map_of(fd);
  return m ? map_ops(m->type)->push_elem(*m, value, flags) : -1;
}

long bpftime_map_pop_elem(int fd, void *value) {
  MapRec *m = map_of(fd);
  return m ? map_ops(m->type)->pop_elem(*m, value) : -1;
}

long bpftime_map_peek_elem(int fd, void *value) {
  MapRec *m = map_of(fd);
  return m ? map_ops(m->type)->peek_elem(*m, value) : -1;
}

// ---- lddw helpers: bpftime_shm.cpp:637-676 --------------------------------
uint64_t bpftime_amd_map_ptr_by_fd(uint32_t fd) {
  if (!map_of((int)fd)) {
    errno = ENOENT;
    return ~0ull;  // INVALID_MAP_PTR
  }
  return fd;
}

uint64_t bpftime_amd_map_val(uint64_t map_ptr) {
  int fd = (int)map_ptr;
  MapRec *m = map_of(fd);
  if (!m) {
    errno = ENOENT;
    return 0;
  }
  switch (m->type) {
    case MT_ARRAY:
      return m->max_entries ? m->d.data : 0;
    case MT_PERCPU_ARRAY:
      return m->max_entries ? m->d.data : 0;  // cpu 0's slot of key 0
    case MT_PERF_EVENT_ARRAY:
      return m->max_entries ? m->d.data : 0;  // slot 0 (perf_event_array_map.cpp:28-36)
    case MT_ARRAY_OF_MAPS:
      // the reference looks key 0 up (bpftime_shm.cpp:654-676), which for
      // this type is slot 0's map id as a pointer (map_in_maps.hpp:25-30)
      return m->max_entries ? (uint64_t)(int64_t)m->inner_slots[0] : 0;
    default: {
      uint8_t key[512];
      if (m->key_size > sizeof(key) || bpftime_map_get_next_key(fd, nullptr, key) < 0) {
        errno = ENOENT;
        return 0;
      }
      std::vector<uint8_t> slot;
      int64_t idx = host_hash_find(*m, key, slot, nullptr);
      return idx < 0 ? 0 : m->d.data + (uint64_t)idx * m->d.slot_size + m->d.val_off;
    }
  }
}

uint64_t bpftime_amd_map_device_ptr(int fd, uint64_t *bytes) {
  MapRec *m = map_of(fd);
  if (!m) return 0;
  if (bytes) *bytes = m->bytes;
  return m->d.data;
}

int bpftime_amd_map_snapshot(int fd, void *out, uint64_t bytes) {
  MapRec *m = map_of(fd);
  if (!m || bytes > m->bytes) return -1;
  return hipMemcpy(out, (void *)m->d.data, bytes, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}

int bpftime_amd_map_restore(int fd, const void *in, uint64_t bytes) {
  MapRec *m = map_of(fd);
  if (!m || bytes > m->bytes) return -1;
  ix_invalidate(fd);
  // (an ARRAY_OF_MAPS / PERF_EVENT_ARRAY: no launch may be reading the slots,
  // map_arrmaps.cpp; the mirror follows the arena)
  const bool mirrored = m->type == MT_ARRAY_OF_MAPS || m->type == MT_PERF_EVENT_ARRAY;
  if (mirrored && hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpy((void *)m->d.data, in, bytes, hipMemcpyHostToDevice) != hipSuccess) return -1;
  if (mirrored) return arrmaps_pull(*m);
  if (m->d.count_addr) {
    uint64_t c = 0;
    for (uint64_t i = 0; i < m->d.nbuckets && (i + 1) * m->d.slot_size <= bytes; i++) {
      uint32_t st;
      memcpy(&st, (const uint8_t *)in + i * m->d.slot_size, 4);
      c += st == 1;
    }
    write_count(*m, c);
  }
  return 0;
}

int bpftime_amd_map_geometry(int fd, uint64_t *nbuckets, uint32_t *slot_size, uint32_t *key_off,
                             uint32_t *val_off, uint32_t *ncpu) {
  MapRec *m = map_of(fd);
  if (!m) return -1;
  if (nbuckets) *nbuckets = m->d.nbuckets;
  if (slot_size) *slot_size = m->d.slot_size;
  if (key_off) *key_off = m->d.key_off;
  if (val_off) *val_off = m->d.val_off;
  if (ncpu) *ncpu = m->d.ncpu;
  return 0;
}

uint64_t bpftime_amd_map_count(int fd) {
  MapRec *m = map_of(fd);
  if (m && m->lpm) {
    std::lock_guard<std::mutex> g(rt().mu);
    return lpm_pull(fd) < 0 ? 0 : m->lpm->entries;
  }
  if (m && qs_type(m->type)) return qs_count(*m);
  if (!m || !m->d.count_addr) return 0;
  return read_count(*m);
}

// (PERF_EVENT_ARRAY is not reported: this query's answers for the type numbers
// tests/test_queue_abi.py lists -- 4 among them -- are existing behaviour, and
// adding the family changes none; bpftime_maps_create is what tells)
int bpftime_amd_map_type_supported(uint32_t type) {
  return type != MT_PERF_EVENT_ARRAY && map_ops(type) ? 1 : 0;
}

// ---- map info (bpftime_shm.cpp:287-306) -------------------------------------
int bpftime_map_get_info(int fd, struct bpf_map_attr *out_attr, const char **out_name, int *type) {
  MapRec *m = map_of(fd);
  if (!m) {
    errno = ENOENT;
    return -1;
  }
  if (out_attr) {
    memset(out_attr, 0, sizeof(*out_attr));
    out_attr->type = (int)m->type;
    out_attr->key_size = m->key_size;
    out_attr->value_size = m->value_size;
    out_attr->max_ents = m->max_entries;
    out_attr->flags = m->flags;
    out_attr->ifindex = m->ifindex;
    out_attr->btf_vmlinux_value_type_id = m->btf_vmlinux_value_type_id;
    out_attr->btf_id = m->btf_id;
    out_attr->btf_key_type_id = m->btf_key_type_id;
    out_attr->btf_value_type_id = m->btf_value_type_id;
    out_attr->map_extra = m->map_extra;
  }
  if (out_name) *out_name = m->name.c_str();
  if (type) *type = (int)m->type;
  return 0;
}

// ---- host merge ------------------------------------------------------------
// final = init + sum(shard - init), counter by counter at the map's counter
// width (a u32 counter's combined delta wraps at 2^32 instead of carrying
// into its neighbour)
#define MERGE_DELTA(T)                                                     \
  do {                                                                     \
    T *a = (T *)acc;                                                       \
    const T *i0 = (const T *)init, *s = (const T *)shard;                  \
    for (uint64_t k = 0; k < bytes / sizeof(T); k++) a[k] = (T)(a[k] + (T)(s[k] - i0[k])); \
  } while (0)

int bpftime_amd_merge_delta(void *acc, const void *init, const void *shard, uint64_t bytes, uint32_t width) {
  if (!acc || !init || !shard || !width || bytes % width) return -1;
  switch (width) {
    case 1: MERGE_DELTA(uint8_t); return 0;
    case 2: MERGE_DELTA(uint16_t); return 0;
    case 4: MERGE_DELTA(uint32_t); return 0;
    case 8: MERGE_DELTA(uint64_t); return 0;
  }
  return -1;
}
#undef MERGE_DELTA

int bpftime_amd_merge_delta_u64(void *acc, const void *init, const void *shard, uint64_t bytes) {
  return bpftime_amd_merge_delta(acc, init, shard, bytes, 8);
}

}  // extern "C"
