// bpftime_amd: ARRAY and PERCPU_ARRAY maps (array_map.cpp:19-81,
// per_cpu_array_map.cpp:97-145) and the host views of ARRAY maps.  The two
// types share their operations: the syscall side of a per-CPU array moves
// every CPU's value (user_value_size).
#include <sys/mman.h>

#include <algorithm>

#include "../../include/bpftime_amd.h"
#include "map_ops.hpp"

namespace bpftime_amd {

static int array_create(Runtime &, MapRec &m) {
  m.bytes = user_value_size(m) * m.max_entries;
  return 0;
}

static const void *array_lookup(MapRec &m, int, const void *key) {
  uint32_t k;
  memcpy(&k, key, 4);
  if (k >= m.max_entries) {
    errno = ENOENT;
    return nullptr;
  }
  const uint64_t vs = user_value_size(m);
  std::vector<uint8_t> &buf = tl_lookup_buf;
  buf.resize(vs);
  if (hipMemcpy(buf.data(), (void *)(m.d.data + k * vs), vs, hipMemcpyDeviceToHost) != hipSuccess) return nullptr;
  return buf.data();
}

static long array_update(MapRec &m, int, const void *key, const void *value, uint64_t flags) {
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
  const uint64_t vs = user_value_size(m);
  return hipMemcpy((void *)(m.d.data + k * vs), value, vs, hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
}

static long array_erase(MapRec &, int, const void *) {
  errno = EINVAL;  // array_map.cpp:58-64
  return -1;
}

static int array_next_key(MapRec &m, int, const void *key, void *next_key) {  // array_map.cpp:66-81
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

const MapOps kArrayOps = {
    array_create, array_lookup, array_update, array_erase, array_next_key,
    /*percpu=*/false, /*counter_line=*/false, /*lru_stamps=*/false, /*prog_shadow=*/false, /*lookup_index=*/false,
    map_no_push, map_no_pop, map_no_peek};
const MapOps kPercpuArrayOps = {
    array_create, array_lookup, array_update, array_erase, array_next_key,
    /*percpu=*/true, /*counter_line=*/false, /*lru_stamps=*/false, /*prog_shadow=*/false, /*lookup_index=*/false,
    map_no_push, map_no_pop, map_no_peek};

// ---- host views of ARRAY maps (bpftime_shm.cpp:347-353 via the mocked
// mmap64, syscall_context.cpp:915-920) ---------------------------------------
// The reference hands a loader the array's bytes in its shared-memory
// segment.  Here they live in HBM: the view is page-aligned host memory
// holding the same bytes, exchanged with the device at batch boundaries --
// what a host write changed reaches the device before the next launch, what
// a batch changed reaches the view when a synchronous batch returns or on
// bpftime_amd_map_msync.
void drop_host_view(Runtime &r, int fd) {
  MapRec &m = r.maps[fd];
  if (m.host_view) munmap(m.host_view, m.host_view_bytes);
  m.host_view = nullptr;
  m.host_view_bytes = 0;
  m.host_shadow.clear();
  r.host_views.erase(fd);
}

// host writes -> device: exactly the bytes that differ from the last
// exchange, run by run.  A byte the host did not write is never uploaded,
// so a counter a batch advanced since the last exchange survives a host
// write next to it; batches still running on any stream finish first (they
// may be writing the same map).
static int view_push(MapRec &m) {
  bool synced = false;
  for (uint64_t i = 0; i < m.bytes;) {
    if (m.host_view[i] == m.host_shadow[i]) {
      i++;
      continue;
    }
    uint64_t j = i + 1;
    while (j < m.bytes && m.host_view[j] != m.host_shadow[j]) j++;
    if (!synced) {
      if (hipDeviceSynchronize() != hipSuccess) return -1;
      synced = true;
    }
    if (hipMemcpy((void *)(m.d.data + i), m.host_view + i, j - i, hipMemcpyHostToDevice) != hipSuccess) return -1;
    memcpy(m.host_shadow.data() + i, m.host_view + i, j - i);
    i = j;
  }
  return 0;
}

static int view_pull(MapRec &m) {
  if (hipMemcpy(m.host_shadow.data(), (void *)m.d.data, m.bytes, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  memcpy(m.host_view, m.host_shadow.data(), m.bytes);
  return 0;
}

int Runtime::host_views_push() {
  std::lock_guard<std::mutex> g(mu);
  for (int fd : host_views)
    if (view_push(maps[fd]) < 0) return -1;
  return 0;
}

int Runtime::host_views_pull() {
  std::lock_guard<std::mutex> g(mu);
  for (int fd : host_views)
    if (view_pull(maps[fd]) < 0) return -1;
  return 0;
}

}  // namespace bpftime_amd

using namespace bpftime_amd;

extern "C" {

int bpftime_is_array_map(int fd) {
  MapRec *m = map_of(fd);
  return m && m->type == MT_ARRAY;
}

void *bpftime_get_array_map_raw_data(int fd) {
  Runtime &r = rt();
  std::lock_guard<std::mutex> g(r.mu);
  MapRec *m = map_of(fd);
  if (!m || m->type != MT_ARRAY) {
    errno = EINVAL;
    return nullptr;
  }
  if (m->host_view) return m->host_view;
  const uint64_t pg = 4096, len = std::max<uint64_t>(pg, (m->bytes + pg - 1) / pg * pg);
  void *p = mmap(nullptr, len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
  if (p == MAP_FAILED) {
    errno = ENOMEM;
    return nullptr;
  }
  m->host_shadow.resize(m->bytes);
  if (m->bytes && hipMemcpy(m->host_shadow.data(), (void *)m->d.data, m->bytes, hipMemcpyDeviceToHost) != hipSuccess) {
    munmap(p, len);
    errno = EIO;
    return nullptr;
  }
  memcpy(p, m->host_shadow.data(), m->bytes);
  m->host_view = (uint8_t *)p;
  m->host_view_bytes = len;
  r.host_views.insert(fd);
  return p;
}

int bpftime_amd_map_msync(int fd) {
  Runtime &r = rt();
  std::lock_guard<std::mutex> g(r.mu);
  MapRec *m = map_of(fd);
  if (!m || !m->host_view) {
    errno = EINVAL;
    return -1;
  }
  if (hipDeviceSynchronize() != hipSuccess) return -1;  // batches still running first
  return view_push(*m) < 0 || view_pull(*m) < 0 ? -1 : 0;
}

}  // extern "C"
