// bpftime_amd: STACK_TRACE maps (runtime/src/bpf_map/userspace/
// stack_trace_map.cpp / .hpp).  Slot id holds the stack whose hash is id
// modulo max_entries (common.hpp, STACK_TRACE: {u64 claim, u32 nframes, u32
// full, u64 frames[value_size / 8]}); programs fill the slots through
// bpf_get_stackid (dev_helpers.hpp helper_stackid, stack_commit.hip).  The
// slots in the arena are the only copy: a host operation reads and writes
// them there after the device has finished what it was running, so it sees a
// finished batch's stacks.
#include "../../include/bpftime_amd.h"
#include "map_ops.hpp"

namespace bpftime_amd {

static int st_create(Runtime &, MapRec &m) {
  if (m.key_size != 4) {  // stack_trace_map.cpp:22-26 (the reference throws)
    errno = EINVAL;
    set_error("Key size of stack trace map must be 4");
    return -1;
  }
  if (m.value_size % 8 != 0) {  // :27-32
    errno = EINVAL;
    set_error("value_size of stack_trace_map must be a multiple of 8, unexpected: " + std::to_string(m.value_size));
    return -1;
  }
  if (m.max_entries == 0) {  // (the reference would divide by zero in fill_stack_trace)
    errno = EINVAL;
    set_error("max_entries of stack_trace_map must not be 0");
    return -1;
  }
  m.d.slot_size = kStHdr + m.value_size;
  m.bytes = (uint64_t)m.d.slot_size * m.max_entries;
  return 0;
}

// bpftime_maps_create zeroes the storage; no slot is claimed
int stacktrace_init(MapRec &m) {
  std::vector<uint8_t> img(m.bytes, 0);
  for (uint64_t i = 0; i < m.max_entries; i++) memcpy(img.data() + i * m.d.slot_size, &kStNoClaim, 8);
  return hipMemcpy((void *)m.d.data, img.data(), m.bytes, hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
}

// the slot of *key after the device has finished: its address, or 0 with
// errno (NULL key: EINVAL; past the end or empty: ENOENT)
static uint64_t st_host_slot(MapRec &m, const void *key, uint32_t hdr[2]) {
  if (!key) {
    errno = EINVAL;
    return 0;
  }
  uint32_t k;
  memcpy(&k, key, 4);
  if (k >= m.max_entries) {
    errno = ENOENT;
    return 0;
  }
  const uint64_t slot = st_slot(m.d, k);
  if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(hdr, (void *)(slot + 8), 8, hipMemcpyDeviceToHost) != hipSuccess) {
    errno = EIO;
    return 0;
  }
  if (!hdr[1]) {
    errno = ENOENT;
    return 0;
  }
  return slot;
}

// :36-61.  value_size bytes: the stored frames, then zeros (the reference's
// vector has just the frames)
static const void *st_lookup(MapRec &m, int, const void *key) {
  uint32_t hdr[2];
  const uint64_t slot = st_host_slot(m, key, hdr);
  if (!slot) return nullptr;
  tl_lookup_buf.resize(m.value_size ? m.value_size : 1);
  if (m.value_size &&
      hipMemcpy(tl_lookup_buf.data(), (void *)(slot + kStHdr), m.value_size, hipMemcpyDeviceToHost) != hipSuccess)
    return nullptr;
  return tl_lookup_buf.data();
}

static long st_update(MapRec &, int, const void *, const void *, uint64_t) { return -ENOTSUP; }  // :63-68

static long st_erase(MapRec &m, int, const void *key) {  // :70-87
  uint32_t hdr[2];
  const uint64_t slot = st_host_slot(m, key, hdr);
  if (!slot) return -1;
  const uint64_t none = 0;
  return hipMemcpy((void *)(slot + 8), &none, 8, hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
}

static int st_next_key(MapRec &, int, const void *, void *) {  // :89-94
  errno = ENOTSUP;
  return -1;
}

const MapOps kStackTraceOps = {
    st_create, st_lookup, st_update, st_erase, st_next_key,
    /*percpu=*/false, /*counter_line=*/false, /*lru_stamps=*/false, /*prog_shadow=*/false, /*lookup_index=*/false,
    map_no_push, map_no_pop, map_no_peek};

}  // namespace bpftime_amd

using namespace bpftime_amd;

extern "C" {

// The frames slot `id` holds, to out (at most cap): the frame count, or -1 +
// ENOENT for an empty slot or an id past the end, -1 + EINVAL for an fd that
// is no STACK_TRACE map.
int bpftime_amd_stack_trace_get(int fd, uint32_t id, uint64_t *out, uint32_t cap) {
  MapRec *m = map_of(fd);
  if (!m || m->type != MT_STACK_TRACE) {
    errno = EINVAL;
    return -1;
  }
  uint32_t hdr[2];
  const uint64_t slot = st_host_slot(*m, &id, hdr);
  if (!slot) return -1;
  const uint32_t n = hdr[0] < cap ? hdr[0] : cap;
  if (n && hipMemcpy(out, (void *)(slot + kStHdr), 8ull * n, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return (int)hdr[0];
}

}  // extern "C"
