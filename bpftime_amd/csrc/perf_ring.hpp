// bpftime_amd: the consumer's walk over a software perf event's ring
// (software_perf_event_buffer::copy_next_record_to and read_wrapped,
// runtime/src/handler/perf_event_handler.cpp:393-450, restated for a ring
// copied to the host).  Plain C++ with no device call, so a stand-alone
// program can drive it.
#pragma once
#include <stdint.h>
#include <string.h>

namespace bpftime_amd {

// `n` bytes at ring position `pos` of a ring of `data_bytes` (a power of two),
// unwrapped into dst
inline void perf_ring_read(const uint8_t *data, uint64_t data_bytes, uint64_t pos, void *dst, uint64_t n) {
  const uint64_t at = pos & (data_bytes - 1);
  const uint64_t first = n <= data_bytes - at ? n : data_bytes - at;
  memcpy(dst, data + at, first);
  if (n > first) memcpy((uint8_t *)dst + first, data, n - first);
}

// Copies the whole records between *tail and head to out, back to back and as
// they lie in the ring (perf_event_header, u32 size, data, padding), and
// advances *tail past them.  Stops at the first record that does not fit the
// rest of `cap`, or that reaches past head (:437-439).  A record whose header
// size is < 8 or larger than the ring drops everything left (*tail = head,
// :430-436); head < *tail does the same (:421-426).  Returns the record count,
// *used the bytes written.
inline int64_t perf_ring_walk(const uint8_t *data, uint64_t data_bytes, uint64_t head, uint64_t *tail, uint8_t *out,
                              uint64_t cap, uint64_t *used) {
  *used = 0;
  if (data_bytes == 0) return 0;
  if (head < *tail) {
    *tail = head;
    return 0;
  }
  int64_t n = 0;
  while (*tail != head) {
    uint8_t hdr[8];
    perf_ring_read(data, data_bytes, *tail, hdr, 8);
    uint16_t size;
    memcpy(&size, hdr + 6, 2);
    if (size < 8 || size > data_bytes) {
      *tail = head;
      break;
    }
    if (size > head - *tail) break;
    if (size > cap - *used) break;
    perf_ring_read(data, data_bytes, *tail, out + *used, size);
    *used += size;
    *tail += size;
    n++;
  }
  return n;
}

}  // namespace bpftime_amd
