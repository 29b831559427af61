// bpftime_amd: QUEUE and STACK maps (runtime/src/bpf_map/userspace/queue.cpp,
// stack.cpp): one ring with a LIFO flag.  The ring in the arena (common.hpp,
// QUEUE / STACK) is the only copy: a host operation reads and writes `head` /
// `tail` and the one slot it names there, so it sees a finished batch's
// pushes and the next batch sees the host's.
#include "../../include/bpftime_amd.h"
#include "map_ops.hpp"

namespace bpftime_amd {

static int qs_create(Runtime &, MapRec &m) {
  // queue.cpp:11-30, stack.cpp:11-29: value_size and max_entries only (the
  // key size is not looked at, map_handler.cpp:846-858)
  if (m.value_size == 0 || m.max_entries == 0) {
    errno = EINVAL;
    set_error("queue / stack map needs value_size > 0 and max_entries > 0");
    return -1;
  }
  const uint64_t stride = ((uint64_t)m.value_size + 3) & ~3ull;
  if (stride > 0xffffffffull) {
    errno = EINVAL;
    set_error("queue / stack map value_size too large");
    return -1;
  }
  m.d.slot_size = (uint32_t)stride;  // common.hpp qs_stride / qs_slot
  m.d.val_off = kQsHeader;
  m.bytes = kQsHeader + stride * m.max_entries;
  return 0;
}

namespace {
struct Ends {
  uint64_t head, tail;
};
}  // namespace

static bool read_ends(const MapRec &m, Ends &e) {
  return hipMemcpy(&e, (void *)m.d.data, 16, hipMemcpyDeviceToHost) == hipSuccess;
}
static bool write_ends(const MapRec &m, const Ends &e) {
  return hipMemcpy((void *)m.d.data, &e, 16, hipMemcpyHostToDevice) == hipSuccess;
}

// queue.cpp:128-169 / stack.cpp:119-157 (`check_flags`: map_push_elem) and
// queue.cpp:66-105 / stack.cpp:61-97 (elem_update: the flags are not
// validated, only BPF_EXIST on a full map differs)
static long qs_push(MapRec &m, const void *value, uint64_t flags, bool check_flags) {
  if (!value) {
    errno = EINVAL;
    return -1;
  }
  if (check_flags && flags != 0 && flags != 2) {  // BPF_ANY = 0, BPF_EXIST = 2
    errno = EINVAL;
    return -1;
  }
  Ends e;
  if (!read_ends(m, e)) return -1;
  if (e.tail - e.head >= m.max_entries) {
    if (flags != 2) {
      errno = E2BIG;
      return -1;
    }
    e.head++;  // the oldest element: the queue's head, the stack's bottom
  }
  // (the slot's pad bytes stay zero, as the device's push leaves them)
  std::vector<uint8_t> slot(m.d.slot_size, 0);
  memcpy(slot.data(), value, m.value_size);
  if (hipMemcpy((void *)qs_slot(m.d, e.tail), slot.data(), slot.size(), hipMemcpyHostToDevice) != hipSuccess) return -1;
  e.tail++;
  return write_ends(m, e) ? 0 : -1;
}

// pop (`remove`; value may be null only for a delete: queue.cpp:107-120,
// :171-194, stack.cpp:99-111, :159-182) and peek (queue.cpp:196-215,
// stack.cpp:184-204)
static long qs_take(MapRec &m, void *value, bool remove, bool need_value) {
  if (need_value && !value) {
    errno = EINVAL;
    return -1;
  }
  Ends e;
  if (!read_ends(m, e)) return -1;
  if (e.tail == e.head) {
    errno = ENOENT;
    return -1;
  }
  const bool lifo = m.type == MT_STACK;
  const uint64_t ticket = lifo ? e.tail - 1 : e.head;
  if (value && hipMemcpy(value, (void *)qs_slot(m.d, ticket), m.value_size, hipMemcpyDeviceToHost) != hipSuccess)
    return -1;
  if (!remove) return 0;
  if (lifo) e.tail--;
  else e.head++;
  return write_ends(m, e) ? 0 : -1;
}

static const void *qs_lookup(MapRec &m, int, const void *) {  // queue.cpp:52-64, stack.cpp:46-59: a peek
  tl_lookup_buf.resize(m.value_size);
  return qs_take(m, tl_lookup_buf.data(), false, true) < 0 ? nullptr : tl_lookup_buf.data();
}

static long qs_update(MapRec &m, int, const void *, const void *value, uint64_t flags) {
  return qs_push(m, value, flags, false);
}

static long qs_erase(MapRec &m, int, const void *) { return qs_take(m, nullptr, true, false); }

static int qs_next_key(MapRec &, int, const void *, void *) {  // queue.cpp:122-126, stack.cpp:113-117
  errno = EINVAL;
  return -1;
}

static long qs_push_elem(MapRec &m, const void *value, uint64_t flags) { return qs_push(m, value, flags, true); }
static long qs_pop_elem(MapRec &m, void *value) { return qs_take(m, value, true, true); }
static long qs_peek_elem(MapRec &m, void *value) { return qs_take(m, value, false, true); }

const MapOps kQueueOps = {
    qs_create, qs_lookup, qs_update, qs_erase, qs_next_key,
    /*percpu=*/false, /*counter_line=*/false, /*lru_stamps=*/false, /*prog_shadow=*/false, /*lookup_index=*/false,
    qs_push_elem, qs_pop_elem, qs_peek_elem};
const MapOps kStackOps = {  // (the LIFO flag is the map's type)
    qs_create, qs_lookup, qs_update, qs_erase, qs_next_key,
    /*percpu=*/false, /*counter_line=*/false, /*lru_stamps=*/false, /*prog_shadow=*/false, /*lookup_index=*/false,
    qs_push_elem, qs_pop_elem, qs_peek_elem};

uint64_t qs_count(const MapRec &m) {
  Ends e;
  return read_ends(m, e) ? e.tail - e.head : 0;
}

}  // namespace bpftime_amd
