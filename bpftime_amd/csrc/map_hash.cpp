// bpftime_amd: HASH and PERCPU_HASH maps (fix_hash_map.cpp:16-84 over
// bpftime_hash_map.hpp, per_cpu_hash_map.cpp:141-216) and the hash lookup
// index the device reads (common.hpp ix_pos).
#include <stdlib.h>

#include <set>
#include <string>

#include "map_ops.hpp"

namespace bpftime_amd {

int hash_geometry(MapRec &m, uint64_t want_buckets, uint64_t value_bytes) {
  if (m.key_size == 0 || m.value_size == 0 || m.max_entries == 0) {
    errno = EINVAL;
    set_error("hash map needs key/value size and max_entries");
    return -1;
  }
  DMap &d = m.d;
  d.nbuckets = next_prime(want_buckets);
  d.key_off = 8;
  d.val_off = 8 + ((m.key_size + 7) & ~7u);
  // Slots never straddle a 128-B cache line: a power of two up to one
  // line, whole lines beyond.  A lane that loads a FILLED state then
  // reads the key from the same line snapshot (dev_helpers.hpp hash_find).
  uint64_t raw = d.val_off + ((value_bytes + 7) & ~7ull);
  uint64_t ss = 16;
  if (raw > 128)
    ss = (raw + 127) & ~127ull;
  else
    while (ss < raw) ss <<= 1;
  d.slot_size = (uint32_t)ss;
  m.bytes = d.nbuckets * d.slot_size;
  return 0;
}

static int hash_create(Runtime &, MapRec &m) { return hash_geometry(m, m.max_entries, user_value_size(m)); }

int64_t host_hash_find(const MapRec &m, const void *key, std::vector<uint8_t> &slot, int64_t *first_empty) {
  const uint64_t nb = m.d.nbuckets;
  uint64_t idx = hash_bytes(key, m.key_size) % nb, start = idx;
  if (first_empty) *first_empty = -1;
  do {
    if (!read_slot(m, idx, slot)) return -1;
    uint32_t st;
    memcpy(&st, slot.data(), 4);
    if (st == 0) {
      if (first_empty) *first_empty = (int64_t)idx;
      return -1;
    }
    if (memcmp(slot.data() + m.d.key_off, key, m.key_size) == 0) return (int64_t)idx;
    idx = (idx + 1) % nb;
  } while (idx != start);
  return -1;
}

static const void *hash_lookup(MapRec &m, int, const void *key) {
  std::vector<uint8_t> slot;
  int64_t idx = host_hash_find(m, key, slot, nullptr);
  if (idx < 0) {
    errno = ENOENT;
    return nullptr;
  }
  tl_lookup_buf.assign(slot.begin() + m.d.val_off, slot.begin() + m.d.val_off + user_value_size(m));
  return tl_lookup_buf.data();
}

// a new element in the empty bucket the probe found
static void hash_insert(MapRec &m, int64_t empty, const void *key, const void *value, uint64_t count) {
  std::vector<uint8_t> s(m.d.slot_size, 0);
  uint32_t st = 1;
  memcpy(s.data(), &st, 4);
  memcpy(s.data() + m.d.key_off, key, m.key_size);
  memcpy(s.data() + m.d.val_off, value, user_value_size(m));
  write_slot(m, (uint64_t)empty, s);
  write_count(m, count + 1);
}

// fix_hash_map.cpp:34-39 -> bpftime_hash_map::elem_update; returns 0
static long hash_update(MapRec &m, int fd, const void *key, const void *value, uint64_t) {
  ix_invalidate(fd);
  std::vector<uint8_t> slot;
  int64_t empty;
  int64_t idx = host_hash_find(m, key, slot, &empty);
  if (idx >= 0) {
    memcpy(slot.data() + m.d.val_off, value, m.value_size);
    write_slot(m, (uint64_t)idx, slot);
  } else if (empty >= 0) {
    uint64_t c = read_count(m);
    if (c < m.max_entries) hash_insert(m, empty, key, value, c);
  }
  return 0;
}

// per_cpu_hash_map.cpp:157-183 (userspace view: ncpu * value_size)
static long percpu_hash_update(MapRec &m, int fd, const void *key, const void *value, uint64_t flags) {
  const uint64_t b = flags & 0xffffffffull;
  if (b != 0 && b != 1 && b != 2) {  // map_common_def.hpp:83-94
    errno = EINVAL;
    return -1;
  }
  ix_invalidate(fd);
  std::vector<uint8_t> slot;
  int64_t empty;
  int64_t idx = host_hash_find(m, key, slot, &empty);
  if (flags == 1 && idx >= 0) {
    errno = EEXIST;
    return -1;
  }
  if (flags == 2 && idx < 0) {
    errno = ENOENT;
    return -1;
  }
  if (idx >= 0) {
    memcpy(slot.data() + m.d.val_off, value, user_value_size(m));
    write_slot(m, (uint64_t)idx, slot);
    return 0;
  }
  uint64_t c = read_count(m);
  if (c >= m.max_entries || empty < 0) {
    errno = E2BIG;
    return -1;
  }
  hash_insert(m, empty, key, value, c);
  return 0;
}

// a missing key: fix_hash_map.cpp:41-45 returns 0 regardless, the per-CPU
// map ENOENT
template <bool kMissingIsError>
static long hash_erase(MapRec &m, int fd, const void *key) {
  // no launch that trusts its lookup cache may still run (runtime.hpp)
  if (rt().lcache_inflight.load()) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    rt().lcache_inflight = false;
    rt().deleter_inflight = false;
  }
  std::vector<uint8_t> slot;
  int64_t idx = host_hash_find(m, key, slot, nullptr);
  if (idx < 0) {
    if (kMissingIsError) {
      errno = ENOENT;
      return -1;
    }
    return 0;
  }
  ix_invalidate(fd);
  uint32_t st = 0;
  memcpy(slot.data(), &st, 4);
  write_slot(m, (uint64_t)idx, slot);
  write_count(m, read_count(m) - 1);
  return 0;
}

static int hash_next_key(MapRec &m, int, const void *key, void *next_key) {  // fix_hash_map.cpp:47-84: bucket index order
  if (!next_key) {
    errno = EINVAL;
    return -1;
  }
  std::vector<uint8_t> all(m.bytes);
  if (hipMemcpy(all.data(), (void *)m.d.data, m.bytes, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  uint64_t from = 0;
  if (key) {
    std::vector<uint8_t> slot;
    int64_t idx = host_hash_find(m, key, slot, nullptr);
    if (idx >= 0) from = (uint64_t)idx + 1;
  }
  for (uint64_t i = from; i < m.d.nbuckets; i++) {
    const uint8_t *s = all.data() + i * m.d.slot_size;
    uint32_t st;
    memcpy(&st, s, 4);
    if (st == 1) {
      memcpy(next_key, s + m.d.key_off, m.key_size);
      return 0;
    }
  }
  errno = ENOENT;
  return -1;
}

const MapOps kHashOps = {
    hash_create, hash_lookup, hash_update, hash_erase<false>, hash_next_key,
    /*percpu=*/false, /*counter_line=*/true, /*lru_stamps=*/false, /*prog_shadow=*/false, /*lookup_index=*/true,
    map_no_push, map_no_pop, map_no_peek};
const MapOps kPercpuHashOps = {
    hash_create, hash_lookup, percpu_hash_update, hash_erase<true>, hash_next_key,
    /*percpu=*/true, /*counter_line=*/true, /*lru_stamps=*/false, /*prog_shadow=*/false, /*lookup_index=*/true,
    map_no_push, map_no_pop, map_no_peek};

// ---- the lookup index -------------------------------------------------------
void ix_invalidate(int fd) {
  Runtime &r = rt();
  MapRec &m = r.maps[fd];
  if (!m.ix_addr || !m.ix_valid) return;
  m.ix_valid = false;
  m.d.ix = 0;
  r.push_map(fd);
  r.ix_stale.insert(fd);
}

// Rebuild from the table: index exactly the keys the reference probe
// (bpftime_hash_map.hpp:127-151: from hash % nb, linear, stop at an empty
// bucket) reaches, i.e. a filled bucket whose key's home bucket lies in the
// same run of filled buckets at or before it, first occurrence of a key
// only.  One pass over the runs, starting after an empty bucket; a table
// without an empty bucket keeps no index.
static int ix_rebuild(int fd) {
  Runtime &r = rt();
  MapRec &m = r.maps[fd];
  if (hipDeviceSynchronize() != hipSuccess) return -1;  // no batch still writing the table
  const uint64_t nb = m.d.nbuckets, ss = m.d.slot_size;
  std::vector<uint8_t> t(m.bytes);
  if (hipMemcpy(t.data(), (void *)m.d.data, m.bytes, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  auto state = [&](uint64_t i) {
    uint32_t st;
    memcpy(&st, t.data() + i * ss, 4);
    return st;
  };
  uint64_t e0 = nb;
  for (uint64_t i = 0; i < nb; i++)
    if (state(i) != 1) {
      e0 = i;
      break;
    }
  r.ix_stale.erase(fd);
  if (e0 == nb) return 0;  // full table: no index (lookups take the reference probe)
  const uint64_t isz = (uint64_t)m.d.ix_mask + 1, words = ix_bitmap_words(nb);
  const uint32_t ks = ix_key_stride(m.key_size);  // key bytes per position (keyed indexes)
  // the index (entries, keys), then the bucket bitmap (common.hpp ix_bitmap): one upload
  std::vector<uint32_t> ix(isz * (4 + ks) / 4 + 2 * words, 0);
  uint64_t *bits = (uint64_t *)(ix.data() + isz * (4 + ks) / 4);
  for (uint64_t i = 0; i < nb; i++)
    if (state(i) != 0) bits[i >> 6] |= 1ull << (i & 63);
  if (nb % 64) bits[words - 1] |= ~0ull << (nb % 64);
  std::set<std::string> run_keys;
  uint64_t run_start = 1;  // distance from e0 of the current run's first bucket
  for (uint64_t k = 1; k < nb; k++) {
    const uint64_t i = (e0 + k) % nb;
    if (state(i) != 1) {
      run_keys.clear();
      run_start = k + 1;
      continue;
    }
    const uint8_t *key = t.data() + i * ss + m.d.key_off;
    const uint64_t h = hash_bytes(key, m.key_size);
    const uint64_t home = (h % nb + nb - e0) % nb;  // distance from e0
    if (home < run_start || home > k) continue;       // orphaned by a deletion
    if (!run_keys.insert(std::string((const char *)key, m.key_size)).second) continue;  // shadowed
    uint32_t p = ix_pos(h, m.d.ix_mask);
    while (ix[p]) p = (p + 1) & m.d.ix_mask;
    ix[p] = (uint32_t)i + 1;
    if (ks) memcpy((uint8_t *)ix.data() + 4 * isz + (uint64_t)p * ks, key, m.key_size);
  }
  if (hipMemcpy((void *)m.ix_addr, ix.data(), 4 * ix.size(), hipMemcpyHostToDevice) != hipSuccess) return -1;
  m.ix_valid = true;
  m.d.ix = m.ix_addr;
  return r.push_map(fd);
}

int Runtime::prepare_ix(bool may_delete, uint64_t units, const std::vector<int> &lpm_written,
                        uint32_t lpm_update_sites, bool lpm) {
  std::lock_guard<std::mutex> g(mu);
  // the LPM tries first, then the hash indexes: the order the single function had
  if (lpm_prepare_launch(*this, units, lpm_written, lpm_update_sites, lpm) < 0) return -1;
  if (may_delete) {
    for (int fd = 0; fd < (int)kMaxFds; fd++)
      if (kind[fd] == HKind::MAP && maps[fd].ix_valid) ix_invalidate(fd);
    return 0;
  }
  while (!ix_stale.empty()) {
    const int fd = *ix_stale.begin();
    if (kind[fd] != HKind::MAP || !maps[fd].ix_addr) {
      ix_stale.erase(fd);
      continue;
    }
    if (ix_rebuild(fd) < 0) return -1;
  }
  return 0;
}

}  // namespace bpftime_amd
