// bpftime_amd: BLOOM_FILTER maps (runtime/src/bpf_map/userspace/bloom_filter.cpp).
// The bit array in the arena is the only copy: a host push or peek reads and
// writes the bytes its probes name there, so it sees a finished batch's
// pushes and the next batch sees its own.
#include <chrono>
#include <random>

#include "../../include/bpftime_amd.h"
#include "map_ops.hpp"

namespace bpftime_amd {

// A Bloom filter's jhash seed: random per map, as the reference's is
// (bloom_filter.cpp:91-92); the clock where the system has no entropy source
static uint32_t bloom_random_seed() {
  try {
    return (uint32_t)std::random_device{}();
  } catch (const std::exception &) {
    return (uint32_t)std::chrono::steady_clock::now().time_since_epoch().count();
  }
}

static int bloom_create(Runtime &, MapRec &m) {
  // map_handler.cpp:860-884, bloom_filter.cpp:50-101: no key, nr_hashes
  // in map_extra's low four bits (0: five), JHASH, a random seed per map
  if (m.key_size != 0 || m.value_size == 0 || m.max_entries == 0) {
    errno = EINVAL;
    set_error("bloom filter needs key_size 0, value_size > 0, max_entries > 0");
    return -1;
  }
  const uint32_t k = (uint32_t)(m.map_extra & 0xF) ? (uint32_t)(m.map_extra & 0xF) : 5;
  const uint64_t bits = bloom_bits(m.max_entries, k);
  m.d.nbuckets = (uint32_t)(bits - 1);  // common.hpp bloom_mask / bloom_hashes / bloom_seed
  m.d.slot_size = k;
  m.d.key_off = bloom_random_seed();
  m.bytes = bits / 8;
  return 0;
}

static long bloom_host_op(MapRec &m, const void *value, bool push) {
  if (!value) {
    errno = EINVAL;
    return -1;
  }
  // the value as zero-padded little-endian words (common.hpp bloom_jhash_words)
  std::vector<uint32_t> w((m.value_size + 11) / 12 * 3, 0);
  memcpy(w.data(), value, m.value_size);
  for (uint32_t i = 0; i < bloom_hashes(m.d); i++) {
    const uint32_t bit = bloom_jhash_words(w.data(), m.value_size, bloom_seed(m.d) + i) & bloom_mask(m.d);
    void *at = (void *)(m.d.data + bit / 8);
    uint8_t b = 0;
    if (hipMemcpy(&b, at, 1, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (b & (1u << (bit % 8))) continue;
    if (!push) {
      errno = ENOENT;
      return -1;
    }
    b |= (uint8_t)(1u << (bit % 8));
    if (hipMemcpy(at, &b, 1, hipMemcpyHostToDevice) != hipSuccess) return -1;
  }
  return 0;
}

static const void *bloom_lookup(MapRec &, int, const void *) {  // bloom_filter.cpp:283-289: peek is the lookup
  errno = EOPNOTSUPP;
  return nullptr;
}

static long bloom_update(MapRec &m, int, const void *, const void *value, uint64_t flags) {
  if (flags != 0) {  // bloom_filter.cpp:291-322: a push, the key ignored
    errno = EINVAL;
    return -1;
  }
  return bloom_host_op(m, value, true);
}

static long bloom_erase(MapRec &, int, const void *) {  // bloom_filter.cpp:324-335 (and next key below)
  errno = EOPNOTSUPP;
  return -1;
}

static int bloom_next_key(MapRec &, int, const void *, void *) {
  errno = ENOTSUP;  // (= EOPNOTSUPP)
  return -1;
}

static long bloom_push_elem(MapRec &m, const void *value, uint64_t flags) {
  if (flags != 0) {  // bloom_filter.cpp:346-352: BPF_ANY only
    errno = EINVAL;
    return -1;
  }
  return bloom_host_op(m, value, true);
}

static long bloom_peek_elem(MapRec &m, void *value) { return bloom_host_op(m, value, false); }

static long bloom_pop_elem(MapRec &, void *) {
  errno = EOPNOTSUPP;  // bloom_filter.cpp:364-369
  return -1;
}

const MapOps kBloomFilterOps = {
    bloom_create, bloom_lookup, bloom_update, bloom_erase, bloom_next_key,
    /*percpu=*/false, /*counter_line=*/false, /*lru_stamps=*/false, /*prog_shadow=*/false, /*lookup_index=*/false,
    bloom_push_elem, bloom_pop_elem, bloom_peek_elem};

}  // namespace bpftime_amd

using namespace bpftime_amd;

extern "C" {

int bpftime_amd_bloom_seed(int fd, const uint32_t *set, uint32_t *out) {
  Runtime &r = rt();
  std::lock_guard<std::mutex> g(r.mu);
  MapRec *m = map_of(fd);
  if (!m || m->type != MT_BLOOM_FILTER) {
    errno = EINVAL;
    return -1;
  }
  if (set) {
    // bits set under another seed mean nothing: the array starts over
    // (batches still running finish first)
    if (hipDeviceSynchronize() != hipSuccess || hipMemset((void *)m->d.data, 0, m->bytes) != hipSuccess) return -1;
    m->d.key_off = *set;
    if (r.push_map(fd) < 0) return -1;
  }
  if (out) *out = bloom_seed(m->d);
  return 0;
}

}  // extern "C"
