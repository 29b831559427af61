// bpftime_amd: bpftime_amd_map_dump (include/bpftime_amd.h, "Map dump and
// drain"): the argument checks, the runtime's scratch and staging buffer, the
// wait before and after the kernels and the copy to the caller.  The
// compaction of a hash table is on the device (map_dump.hip); an array is one
// contiguous copy and takes no kernel.
//
// The checks of args, flags and fd run before the first HIP call, so a call
// they refuse needs no device.  The call is synchronous: it holds the runtime
// lock, waits for the device first (as hash_erase and ix_rebuild do: a batch
// on any stream has finished, its deferred counter adds are in the table),
// runs the kernels on the null stream and reads their result back.
//
// Scratch: one device buffer of the Runtime holding the result words, the
// tile counts and the dense key and value staging arrays, allocated when a
// call first needs more than there is and kept for the calls after it
// (bpftime_amd_reset frees it).  Nothing in it is set to zero: the kernels
// write every word they read.
#include <errno.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/bpftime_amd.h"
#include "map_dump.hpp"
#include "map_ops.hpp"

using namespace bpftime_amd;

namespace {

int fail(const std::string &what, int err = EINVAL) {
  set_error("map dump: " + what);
  errno = err;
  return -1;
}

int hip_fail(const char *what, hipError_t e) { return fail(std::string(what) + ": " + hipGetErrorString(e), EIO); }

const char *type_name(uint32_t type) {
  switch (type) {
    case MT_HASH: return "HASH";
    case MT_ARRAY: return "ARRAY";
    case MT_PROG_ARRAY: return "PROG_ARRAY";
    case MT_PERF_EVENT_ARRAY: return "PERF_EVENT_ARRAY";
    case MT_PERCPU_HASH: return "PERCPU_HASH";
    case MT_PERCPU_ARRAY: return "PERCPU_ARRAY";
    case MT_STACK_TRACE: return "STACK_TRACE";
    case MT_LRU_HASH: return "LRU_HASH";
    case MT_LPM_TRIE: return "LPM_TRIE";
    case MT_ARRAY_OF_MAPS: return "ARRAY_OF_MAPS";
    case MT_QUEUE: return "QUEUE";
    case MT_STACK: return "STACK";
    case MT_RINGBUF: return "RINGBUF";
    case MT_BLOOM_FILTER: return "BLOOM_FILTER";
  }
  return "?";
}
std::string type_text(uint32_t type) { return "map type " + std::to_string(type) + " (" + type_name(type) + ")"; }

uint64_t round256(uint64_t v) { return (v + 255) & ~255ull; }

// elements start .. start + count - 1: the values one copy, the keys their indices
int dump_array(MapRec &m, struct bpftime_amd_map_dump_args *a) {
  const uint64_t vs = user_value_size(m);
  const uint64_t count = std::min<uint64_t>(a->cap, a->end - a->start);
  hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) return hip_fail("wait", e);
  if (a->values && (e = hipMemcpy(a->values, (void *)(m.d.data + a->start * vs), count * vs, hipMemcpyDefault)) !=
                       hipSuccess)
    return hip_fail("values", e);
  if (a->keys) {
    std::vector<uint32_t> k(count);
    for (uint64_t i = 0; i < count; i++) k[i] = (uint32_t)(a->start + i);
    if ((e = hipMemcpy(a->keys, k.data(), 4 * count, hipMemcpyDefault)) != hipSuccess) return hip_fail("keys", e);
  }
  a->count = count;
  a->next = a->start + count;
  return 0;
}

int dump_hash(Runtime &r, MapRec &m, struct bpftime_amd_map_dump_args *a, bool erase) {
  const uint64_t nb = m.d.nbuckets, ks = m.key_size, vb = user_value_size(m);
  if ((uint64_t)m.d.key_off + ks > m.d.slot_size || (uint64_t)m.d.val_off + vb > m.d.slot_size ||
      nb * m.d.slot_size > m.bytes)
    return fail("fd " + std::to_string(a->fd) + ": the slot layout does not hold its key and value");
  hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) return hip_fail("wait", e);
  // (no launch that trusts its lookup cache is still running: hash_erase's rule)
  if (erase && r.lcache_inflight.load()) {
    r.lcache_inflight = false;
    r.deleter_inflight = false;
  }
  const uint64_t bound = std::min<uint64_t>(a->cap, nb - a->start);  // entries the kernels may write
  MdParams p{};
  p.tiles = (uint32_t)((nb - a->start + kMdTile - 1) / kMdTile);
  const uint64_t counts_at = 256, keys_at = counts_at + round256(4ull * p.tiles),
                 values_at = keys_at + (a->keys ? round256(bound * ks) : 0),
                 need = values_at + (a->values ? round256(bound * vb) : 0);
  if (r.dump_bytes < need) {
    if (r.dump_buf && (e = hipFree(r.dump_buf)) != hipSuccess) return hip_fail("scratch", e);
    r.dump_buf = nullptr;
    r.dump_bytes = 0;
    if (hipMalloc(&r.dump_buf, need) != hipSuccess) {
      r.dump_buf = nullptr;
      return fail("scratch allocation of " + std::to_string(need) + " bytes failed", ENOMEM);
    }
    r.dump_bytes = need;
  }
  uint8_t *buf = (uint8_t *)r.dump_buf;
  p.table = (uint8_t *)m.d.data;
  p.nbuckets = nb;
  p.slot_size = m.d.slot_size;
  p.key_off = m.d.key_off;
  p.val_off = m.d.val_off;
  p.key_size = (uint32_t)ks;
  p.val_bytes = (uint32_t)vb;
  p.start = a->start;
  p.cap = bound;
  p.erase = erase ? 1 : 0;
  // 16 B per lane: a lane per entry for small slots, up to a wave per entry
  const uint64_t widest = std::max<uint64_t>(a->keys ? ks : 0, a->values ? vb : 0);
  p.group = 1;
  while (p.group < 64 && 16ull * p.group < widest) p.group <<= 1;
  p.keys = a->keys ? buf + keys_at : nullptr;
  p.values = a->values ? buf + values_at : nullptr;
  p.tile_counts = (uint32_t *)(buf + counts_at);
  p.result = (uint64_t *)buf;
  if ((e = bpftime_amd_launch_map_dump(&p, nullptr)) != hipSuccess) return hip_fail("launch", e);
  uint64_t res[kMdResultWords] = {0};
  if ((e = hipMemcpy(res, p.result, sizeof(res), hipMemcpyDeviceToHost)) != hipSuccess) return hip_fail("result", e);
  const uint64_t count = res[kMdCount];
  if (count > bound || res[kMdNext] > nb) return fail("the kernels returned a count past the bound", EIO);
  if (a->keys && count && (e = hipMemcpy(a->keys, p.keys, count * ks, hipMemcpyDefault)) != hipSuccess)
    return hip_fail("keys", e);
  if (a->values && count && (e = hipMemcpy(a->values, p.values, count * vb, hipMemcpyDefault)) != hipSuccess)
    return hip_fail("values", e);
  if (erase && count) {
    ix_invalidate(a->fd);
    write_count(m, read_count(m) - count);
  }
  a->count = count;
  // (a cap above the buckets left was clamped: the bucket of that rank cannot exist)
  a->next = res[kMdNext];
  return 0;
}

}  // namespace

extern "C" uint32_t bpftime_amd_map_dump_tile(void) { return kMdTile; }
extern "C" uint32_t bpftime_amd_map_dump_scan_tiles(void) { return kMdScanTiles; }

extern "C" int bpftime_amd_map_dump(struct bpftime_amd_map_dump_args *a) {
  if (!a) return fail("args is NULL");
  a->count = 0;
  a->next = a->start;
  a->end = 0;
  if (a->flags & ~(uint32_t)BPFTIME_AMD_DUMP_DELETE) return fail("unknown flags " + std::to_string(a->flags));
  const bool erase = (a->flags & BPFTIME_AMD_DUMP_DELETE) != 0;
  Runtime &r = rt();
  std::lock_guard<std::mutex> g(r.mu);
  MapRec *m = map_of(a->fd);
  if (!m) return fail("fd " + std::to_string(a->fd) + " is not a map", ENOENT);
  const bool array = m->type == MT_ARRAY || m->type == MT_PERCPU_ARRAY;
  const bool hash = m->type == MT_HASH || m->type == MT_PERCPU_HASH || m->type == MT_LRU_HASH;
  if (!array && !hash) return fail(type_text(m->type) + " has no dump", ENOTSUP);
  if (erase && array) return fail(type_text(m->type) + ": an array element cannot be deleted");  // array_erase
  if (erase && m->type == MT_LRU_HASH)
    return fail(type_text(m->type) + ": BPFTIME_AMD_DUMP_DELETE is not served (tombstones stay with the map's own delete)",
                ENOTSUP);
  a->end = array ? m->max_entries : m->d.nbuckets;
  if (a->start > a->end)
    return fail("start " + std::to_string(a->start) + " is past the end " + std::to_string(a->end));
  if (a->start == a->end) {
    a->next = a->end;
    return 0;
  }
  if (a->cap == 0) return 0;  // (next = start; no launch)
  return array ? dump_array(*m, a) : dump_hash(r, *m, a, erase);
}
