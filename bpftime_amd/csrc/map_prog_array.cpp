// bpftime_amd: PROG_ARRAY maps (runtime/src/bpf_map/userspace/prog_array.cpp).
// Slots hold bpftime prog fds (the reference encodes them as -fd-2 beside
// kernel prog ids; kernel programs do not exist here).
#include "../../include/bpftime_amd.h"
#include "map_ops.hpp"

namespace bpftime_amd {

static thread_local int32_t tl_prog_fd;

static int prog_array_create(Runtime &, MapRec &m) {
  // prog_array.cpp:101-110: key and value are both 4 bytes
  if (m.key_size != 4 || m.value_size != 4) {
    errno = EINVAL;
    set_error("Key size and value size of prog_array must be 4");
    return -1;
  }
  m.bytes = 4ull * m.max_entries;
  return 0;
}

static int32_t prog_array_read(const MapRec &m, int32_t k) {
  int32_t v = -1;
  if (hipMemcpy(&v, (const void *)(m.d.data + 4ull * (uint32_t)k), 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return v;
}

// prog_array.cpp:113-143
static const void *prog_array_lookup(MapRec &m, int, const void *key) {
  int32_t k;
  memcpy(&k, key, 4);
  if (k < 0 || (uint32_t)k >= m.max_entries) {
    errno = EINVAL;
    return nullptr;
  }
  const int32_t v = prog_array_read(m, k);
  if (v < 0 || !bpftime_is_prog_fd(v)) {
    errno = ENOENT;
    return nullptr;
  }
  tl_prog_fd = v;
  return &tl_prog_fd;
}

// prog_array.cpp:146-176 (flags are not looked at); a value that is not a
// bpftime prog fd would be asked of the kernel, which has no such fd here
static long prog_array_update(MapRec &m, int, const void *key, const void *value, uint64_t) {
  int32_t k, v;
  memcpy(&k, key, 4);
  if (k < 0 || (uint32_t)k >= m.max_entries) {
    errno = EINVAL;
    return -1;
  }
  memcpy(&v, value, 4);
  if (!bpftime_is_prog_fd(v)) {
    errno = EBADF;
    return -1;
  }
  if (hipMemcpy((void *)(m.d.data + 4ull * (uint32_t)k), &v, 4, hipMemcpyHostToDevice) != hipSuccess) return -1;
  rt().prog_gen++;
  return 0;
}

// prog_array.cpp:180-189
static long prog_array_delete(MapRec &m, int, const void *key) {
  int32_t k;
  memcpy(&k, key, 4);
  if (k < 0 || (uint32_t)k >= m.max_entries) {
    errno = EINVAL;
    return -1;
  }
  const int32_t none = -1;
  if (hipMemcpy((void *)(m.d.data + 4ull * (uint32_t)k), &none, 4, hipMemcpyHostToDevice) != hipSuccess) return -1;
  rt().prog_gen++;
  return 0;
}

// prog_array.cpp:191-211: the last key is checked before the range
static int prog_array_next_key(MapRec &m, int, const void *key, void *next_key) {
  int32_t out = 0;
  if (key) {
    int32_t k;
    memcpy(&k, key, 4);
    if ((size_t)(k + 1) == m.max_entries) {
      errno = ENOENT;
      return -1;
    }
    if (k < 0 || (uint32_t)k >= m.max_entries) {
      errno = EINVAL;
      return -1;
    }
    out = k + 1;
  }
  memcpy(next_key, &out, 4);
  return 0;
}

const MapOps kProgArrayOps = {
    prog_array_create, prog_array_lookup, prog_array_update, prog_array_delete, prog_array_next_key,
    /*percpu=*/false, /*counter_line=*/false, /*lru_stamps=*/false, /*prog_shadow=*/true, /*lookup_index=*/false,
    map_no_push, map_no_pop, map_no_peek};

}  // namespace bpftime_amd
