// bpftime_amd: the host side of RINGBUF maps (runtime/src/bpf_map/userspace/
// ringbuf_map.cpp): the consumer.  Lookup / update / delete / next key are
// unsupported there.
#include "../../include/bpftime_amd.h"
#include "map_ops.hpp"

namespace bpftime_amd {

static int ringbuf_create(Runtime &, MapRec &m) {
  // ringbuf_map.cpp: positions + 2 x max_entries data bytes; mask =
  // max_entries - 1 needs a power of two
  if (m.max_entries == 0 || (m.max_entries & (m.max_entries - 1))) {
    errno = EINVAL;
    set_error("ring buffer size must be a power of two");
    return -1;
  }
  m.bytes = 256 + 2ull * m.max_entries;
  return 0;
}

static const void *ringbuf_lookup(MapRec &, int, const void *) {
  errno = ENOTSUP;
  return nullptr;
}
static long ringbuf_update(MapRec &, int, const void *, const void *, uint64_t) {
  errno = ENOTSUP;
  return -1;
}
static long ringbuf_erase(MapRec &, int, const void *) {
  errno = ENOTSUP;
  return -1;
}
static int ringbuf_next_key(MapRec &, int, const void *, void *) {
  errno = ENOTSUP;
  return -1;
}

const MapOps kRingbufOps = {
    ringbuf_create, ringbuf_lookup, ringbuf_update, ringbuf_erase, ringbuf_next_key,
    /*percpu=*/false, /*counter_line=*/false, /*lru_stamps=*/false, /*prog_shadow=*/false, /*lookup_index=*/false,
    map_no_push, map_no_pop, map_no_peek};

}  // namespace bpftime_amd

using namespace bpftime_amd;

// ringbuf::fetch_data (ringbuf_map.cpp): committed records from the consumer
// position on, stopping at a record still being written; discarded records
// are skipped.  Each delivered record is written to out as [u32 len][bytes].
extern "C" int64_t bpftime_amd_ringbuf_fetch(int fd, void *out, uint64_t cap, uint64_t *used) {
  MapRec *m = map_of(fd);
  if (used) *used = 0;
  if (!m || m->type != MT_RINGBUF) {
    errno = EINVAL;
    return -1;
  }
  if (hipDeviceSynchronize() != hipSuccess) return -1;  // producers of queued batches first
  uint64_t pos[2];
  std::vector<uint8_t> data(2ull * m->max_entries);
  if (hipMemcpy(&pos[0], (void *)m->d.data, 8, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(&pos[1], (void *)(m->d.data + 128), 8, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(data.data(), (void *)(m->d.data + 256), data.size(), hipMemcpyDeviceToHost) != hipSuccess)
    return -1;
  const uint64_t mask = m->max_entries - 1;
  uint64_t cons = pos[0], off = 0;
  int64_t cnt = 0;
  while (cons < pos[1]) {
    uint32_t len;
    memcpy(&len, data.data() + (cons & mask), 4);
    if (len & 0x80000000u) break;  // BUSY
    const uint32_t n = len & 0x3fffffffu;
    if (!(len & 0x40000000u)) {     // not DISCARD
      if (off + 4 + n > cap) break;
      memcpy((uint8_t *)out + off, &n, 4);
      memcpy((uint8_t *)out + off + 4, data.data() + (cons & mask) + 8, n);
      off += 4 + n;
      cnt++;
    }
    cons += ((uint64_t)n + 8 + 7) / 8 * 8;
  }
  if (hipMemcpy((void *)m->d.data, &cons, 8, hipMemcpyHostToDevice) != hipSuccess) return -1;
  if (used) *used = off;
  return cnt;
}
