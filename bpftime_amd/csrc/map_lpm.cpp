// bpftime_amd: LPM_TRIE maps.  The host keeps the authoritative trie
// (lpm_trie.hpp); this is its device replica -- upload, pull-back after an
// ORDERED batch wrote it, pool growth, the flat table of IPv4 tries -- and
// the host-side operations.  Those take the runtime lock: a launch on another
// thread inserts into lpm_dev_dirty and allocates from the arena under it.
#include <stdlib.h>

#include <algorithm>

#include "../../include/bpftime_amd.h"
#include "lpm_trie.hpp"
#include "map_ops.hpp"

namespace bpftime_amd {

static int lpm_create(Runtime &, MapRec &m) {
  // lpm_trie_map.cpp:43-81: key = u32 prefixlen + 1..256 data bytes
  if (m.key_size < 5 || m.key_size > 260 || m.value_size == 0 || m.max_entries == 0) {
    errno = EINVAL;
    set_error("LPM trie needs key_size 5..260, value_size > 0, max_entries > 0");
    return -1;
  }
  auto t = std::make_shared<LpmTrie>();
  t->dsz = m.key_size - 4;
  t->vsz = m.value_size;
  t->max_entries = m.max_entries;
  t->cap = (uint32_t)std::min<uint64_t>(2ull * m.max_entries + 8, 1u << 26);
  m.lpm = t;
  DMap &d = m.d;
  d.key_off = 16;
  d.val_off = 16 + ((t->dsz + 7) & ~7u);
  d.slot_size = d.val_off + ((m.value_size + 7) & ~7u);
  m.bytes = 16 + (uint64_t)t->cap * d.slot_size;
  return 0;
}

static void lpm_touch(int fd) { rt().lpm_stale.insert(fd); }

void lpm_drop_flat(MapRec &m) {
  if (m.lpm_flat) (void)hipFree(m.lpm_flat);
  m.lpm_flat = nullptr;
  m.lpm_flat_bytes = 0;
}

// A bigger node pool for the replica: logical deletions never free a node
// (lpm_trie_map.cpp:490-541), so a trie that keeps learning new prefixes
// outgrows any fixed pool; the reference's allocator just grows.  The
// replica moves to a new arena block (values stay inside the arena, which
// the device's access checks and counter tags rely on; the old block is
// not reused) and is uploaded whole before the next launch.
static int lpm_grow(int fd, uint64_t want_nodes) {
  Runtime &r = rt();
  MapRec &m = r.maps[fd];
  if (lpm_pull(fd) < 0) return -1;
  LpmTrie &t = *m.lpm;
  if (want_nodes <= t.cap) return 0;
  uint64_t cap = t.cap ? t.cap : 8;
  while (cap < want_nodes) cap *= 2;
  if (cap > (1ull << 26)) cap = 1ull << 26;
  if (cap <= t.cap) {
    errno = ENOMEM;
    return -1;
  }
  const uint64_t bytes = 16 + cap * m.d.slot_size;
  if (hipDeviceSynchronize() != hipSuccess) return -1;  // no batch still reading the old replica
  const uint64_t base = r.arena_alloc(bytes);
  if (!base) {
    errno = ENOMEM;
    set_error("map arena exhausted growing an LPM trie (BPFTIME_AMD_ARENA_MB)");
    return -1;
  }
  t.cap = (uint32_t)cap;
  m.d.data = base;
  m.bytes = bytes;
  m.d.ix = 0;
  if (r.push_map(fd) < 0) return -1;
  lpm_touch(fd);
  if (t.dsz == 4) r.lpm_flat_pending.insert(fd);
  return 0;
}

static int lpm_pool_out_error(int fd) {
  set_error("LPM_TRIE map fd " + std::to_string(fd) +
            ": an ORDERED batch's program-side update ran out of the device node pool; the trie keeps its state "
            "from before that batch (bpftime_amd_map_ack_error clears this report)");
  errno = ENOMEM;
  return -1;
}

int lpm_pull(int fd) {
  Runtime &r = rt();
  if (r.kind[fd] == HKind::MAP && r.maps[fd].lpm_pool_out) return lpm_pool_out_error(fd);
  if (!r.lpm_dev_dirty.count(fd)) return 0;
  MapRec &m = r.maps[fd];
  r.lpm_dev_dirty.erase(fd);
  if (r.kind[fd] != HKind::MAP || !m.lpm) return 0;
  if (hipDeviceSynchronize() != hipSuccess) return -1;  // the batch that wrote it
  uint32_t hdr[4];
  if (hipMemcpy(hdr, (void *)m.d.data, 16, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  if (hdr[3] & kLpmPoolOut) {
    // a program's update ran out of the replica's node pool (sized before
    // the launch for two nodes per update site and unit,
    // lpm_prepare_launch): the reference's trie would have grown, so the
    // batch's results are not the reference's.  The host keeps its trie (the
    // state before that batch) and reports it
    lpm_touch(fd);
    m.lpm_pool_out = true;
    return lpm_pool_out_error(fd);
  }
  const uint64_t bytes = 16 + (uint64_t)std::min(hdr[1], m.lpm->cap) * m.d.slot_size;
  std::vector<uint8_t> img(bytes);
  if (hipMemcpy(img.data(), (void *)m.d.data, bytes, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  if (!m.lpm->from_image(img.data(), bytes, m.d.slot_size, m.d.key_off, m.d.val_off)) {
    set_error("LPM replica is corrupt");
    return -1;
  }
  // the replica is current; the flat table of the old trie is not
  if (m.d.ix) {
    m.d.ix = 0;
    if (r.push_map(fd) < 0) return -1;
  }
  if (m.lpm->dsz == 4) r.lpm_flat_pending.insert(fd);
  return 0;
}

static int lpm_upload(int fd) {
  Runtime &r = rt();
  MapRec &m = r.maps[fd];
  std::vector<uint8_t> img;
  m.lpm->image(img, m.d.slot_size, m.d.key_off, m.d.val_off);
  if (hipDeviceSynchronize() != hipSuccess) return -1;  // no batch still reading the replica
  if (hipMemcpy((void *)m.d.data, img.data(), img.size(), hipMemcpyHostToDevice) != hipSuccess) return -1;
  r.lpm_stale.erase(fd);
  // device lookups walk the replica until a launch large enough builds the
  // flat table (lpm_flat_build)
  m.d.ix = 0;
  if (m.lpm->dsz == 4) r.lpm_flat_pending.insert(fd);
  return r.push_map(fd);
}

// IPv4 tries also get the flat table (LpmTrie::flat) device lookups of
// full-length keys take in one or two loads instead of the trie walk; the
// map record owns its device block (MapRec::lpm_flat)
static int lpm_flat_build(int fd) {
  Runtime &r = rt();
  MapRec &m = r.maps[fd];
  if (lpm_pull(fd) < 0) return -1;
  r.lpm_flat_pending.erase(fd);
  uint64_t flat = 0;
  std::vector<uint32_t> t;
  if (m.lpm->dsz == 4 && !getenv("BPFTIME_AMD_NO_LPM_FLAT") && m.lpm->flat(t, 1u << 16)) {
    const uint64_t bytes = 4ull * t.size();
    if (m.lpm_flat_bytes < bytes) {
      lpm_drop_flat(m);
      if (hipMalloc(&m.lpm_flat, bytes) == hipSuccess) m.lpm_flat_bytes = bytes;
    }
    if (m.lpm_flat && hipMemcpy(m.lpm_flat, t.data(), bytes, hipMemcpyHostToDevice) == hipSuccess)
      flat = (uint64_t)(uintptr_t)m.lpm_flat;
  }
  m.d.ix = flat;
  return r.push_map(fd);
}

int lpm_prepare_launch(Runtime &r, uint64_t units, const std::vector<int> &lpm_written, uint32_t lpm_update_sites,
                       bool lpm) {
  // a trie whose device update ran out of its pool fails every launch of a
  // program naming a trie until acknowledged
  // (a trie a writer left on the device: its header's pool flag, 16 bytes)
  for (int fd = 0; lpm && fd < (int)kMaxFds; fd++) {
    if (r.kind[fd] != HKind::MAP || !r.maps[fd].lpm) continue;
    if (r.maps[fd].lpm_pool_out) return lpm_pool_out_error(fd);
    if (!r.lpm_dev_dirty.count(fd)) continue;
    uint32_t hdr[4];
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(hdr, (void *)r.maps[fd].d.data, 16, hipMemcpyDeviceToHost) != hipSuccess)
      return -1;
    if ((hdr[3] & kLpmPoolOut) && lpm_pull(fd) < 0) return -1;
  }
  // every launch of a program that names a trie reads the current LPM tries
  while (lpm && !r.lpm_stale.empty()) {
    const int fd = *r.lpm_stale.begin();
    if (r.kind[fd] != HKind::MAP || !r.maps[fd].lpm) {
      r.lpm_stale.erase(fd);
      continue;
    }
    if (lpm_upload(fd) < 0) return -1;
  }
  // the flat tables only for launches that pay for their build (a host fill
  // of 2^24 entries and a 64-MiB upload after every change of the trie)
  // tries the program may write keep walking the replica: their flat
  // table is dropped and rebuilt once the host has the trie back; their
  // node pool gets room for two new nodes per update call site and unit
  // (an insert makes at most two), up to 2^22 nodes more
  for (const int fd : lpm_written) {
    if (r.kind[fd] != HKind::MAP || !r.maps[fd].lpm) continue;
    if (lpm_pull(fd) < 0) return -1;
    const uint64_t room = std::min<uint64_t>(2 * units * std::max<uint32_t>(lpm_update_sites, 1), 1ull << 22);
    if (r.maps[fd].lpm->nodes.size() + room > r.maps[fd].lpm->cap &&
        lpm_grow(fd, r.maps[fd].lpm->nodes.size() + room) < 0)
      return -1;
    if (r.lpm_stale.count(fd) && lpm_upload(fd) < 0) return -1;
    if (r.maps[fd].d.ix) {
      r.maps[fd].d.ix = 0;
      if (r.push_map(fd) < 0) return -1;
    }
    if (r.maps[fd].lpm->dsz == 4) r.lpm_flat_pending.insert(fd);
  }
  if (lpm && units >= kLpmFlatMinUnits) {
    std::vector<int> pending(r.lpm_flat_pending.begin(), r.lpm_flat_pending.end());
    for (const int fd : pending) {
      if (r.kind[fd] != HKind::MAP || !r.maps[fd].lpm) {
        r.lpm_flat_pending.erase(fd);
        continue;
      }
      if (std::find(lpm_written.begin(), lpm_written.end(), fd) != lpm_written.end()) continue;
      if (lpm_flat_build(fd) < 0) return -1;
    }
  }
  return 0;
}

static const void *lpm_lookup(MapRec &m, int fd, const void *key) {
  if (!key) {
    errno = EINVAL;
    return nullptr;
  }
  std::lock_guard<std::mutex> g(rt().mu);
  if (lpm_pull(fd) < 0) return nullptr;
  const LpmTrie::Node *n = m.lpm->lookup((const uint8_t *)key);
  if (!n) return nullptr;
  tl_lookup_buf = n->value;  // the reference also hands out a copy (lpm_trie_map.cpp:252-263)
  return tl_lookup_buf.data();
}

static long lpm_update(MapRec &m, int fd, const void *key, const void *value, uint64_t flags) {
  if (!key || !value) {
    errno = EINVAL;
    return -1;
  }
  std::lock_guard<std::mutex> g(rt().mu);
  if (lpm_pull(fd) < 0) return -1;
  if (m.lpm->nodes.size() + 2 > m.lpm->cap && lpm_grow(fd, m.lpm->nodes.size() + 2) < 0) return -1;
  const long rc = m.lpm->update((const uint8_t *)key, value, flags);
  if (rc == 0) lpm_touch(fd);
  return rc;
}

static long lpm_erase(MapRec &m, int fd, const void *key) {
  if (!key) {
    errno = EINVAL;
    return -1;
  }
  std::lock_guard<std::mutex> g(rt().mu);
  if (lpm_pull(fd) < 0) return -1;
  const long rc = m.lpm->remove((const uint8_t *)key);
  if (rc == 0) lpm_touch(fd);
  return rc;
}

static int lpm_next_key(MapRec &m, int fd, const void *key, void *next_key) {
  if (!next_key || key) {  // lpm_trie_map.cpp:543-590: only the first key
    errno = next_key ? ENOENT : EINVAL;
    return -1;
  }
  std::lock_guard<std::mutex> g(rt().mu);
  if (lpm_pull(fd) < 0) return -1;
  return m.lpm->first_key((uint8_t *)next_key);
}

const MapOps kLpmTrieOps = {
    lpm_create, lpm_lookup, lpm_update, lpm_erase, lpm_next_key,
    /*percpu=*/false, /*counter_line=*/false, /*lru_stamps=*/false, /*prog_shadow=*/false, /*lookup_index=*/false,
    map_no_push, map_no_pop, map_no_peek};

}  // namespace bpftime_amd

extern "C" int bpftime_amd_map_ack_error(int fd) {
  using namespace bpftime_amd;
  Runtime &r = rt();
  std::lock_guard<std::mutex> g(r.mu);
  if (fd < 0 || fd >= (int)kMaxFds || r.kind[fd] != HKind::MAP) return -1;
  const bool had = r.maps[fd].lpm_pool_out;
  r.maps[fd].lpm_pool_out = false;
  return had ? 1 : 0;
}
