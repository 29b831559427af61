// bpftime_amd: device-side helpers of the interpreter (maps, XDP helpers,
// wave utilities).  Included by interp.hip only.
#pragma once
#include <hip/hip_runtime.h>
#include "common.hpp"
#include "mem_guard.hpp"  // is_lds_addr, is_scratch_addr, Win, the range guard
#include "trace_fmt.hpp"  // bpf_trace_printk: the format scanner and the log's record

namespace bpftime_amd {

typedef uint16_t u16u __attribute__((aligned(1)));
typedef uint32_t u32u __attribute__((aligned(1)));
typedef uint64_t u64u __attribute__((aligned(1)));

// Sized load/store on a flat address (LDS, scratch or global); the size is
// wave-uniform so the switch is a scalar branch.
__device__ __forceinline__ uint64_t mem_load(uint64_t a, uint32_t sz) {
  switch (sz) {
    case 1: return *(const volatile uint8_t *)a;
    case 2: return *(const u16u *)a;
    case 4: return *(const u32u *)a;
    default: return *(const u64u *)a;
  }
}
__device__ __forceinline__ void mem_store(uint64_t a, uint32_t sz, uint64_t v) {
  switch (sz) {
    case 1: *(uint8_t *)a = (uint8_t)v; break;
    case 2: *(u16u *)a = (uint16_t)v; break;
    case 4: *(u32u *)a = (uint32_t)v; break;
    default: *(u64u *)a = v; break;
  }
}

// ---------------------------------------------------------------------------
// Device maps (helpers 1/2/3).  Semantics follow the reference helper view:
//   array_map.cpp:27-64, fix_hash_map.cpp:27-45 over bpftime_hash_map.hpp,
//   per_cpu_array_map.cpp:34-80, per_cpu_hash_map.cpp:48-107.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint64_t key_hash(uint64_t key, uint32_t ks) {
  // bpftime_hash_map.hpp:40-47: h = h*31 + byte over size_t
  uint64_t h = 0;
  for (uint32_t i = 0; i < ks; i++) h = h * 31 + *(const volatile uint8_t *)(key + i);
  return h;
}

// Hash-table words are shared between workgroups on different XCDs while a
// batch runs: every access is a GLOBAL (address_space(1)) agent-scope atomic
// (sc1), never a flat access (MI355X_MICROARCH.md, inter-workgroup visibility).
typedef __attribute__((address_space(1))) uint32_t gu32;
typedef __attribute__((address_space(1))) unsigned long long gu64;
#define G32(a) ((gu32 *)(uintptr_t)(a))
#define G64(a) ((gu64 *)(uintptr_t)(a))

__device__ __forceinline__ uint32_t ald32(uint64_t a) {
  return __hip_atomic_load(G32(a), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint8_t ald8(uint64_t a) {
  uint64_t w = a & ~3ull;
  uint32_t v = ald32(w);
  return (uint8_t)(v >> ((a & 3) * 8));
}

// Coherent read: an atomic is performed at the coherence point, so it sees
// every store another XCD has drained, even when this XCD's L2 still holds
// an older copy of the line (an sc1 load is served by the local L2).
__device__ __forceinline__ uint32_t acoh32(uint64_t a) {
  return __hip_atomic_fetch_or(G32(a), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Compare the program-side key (any alignment, any memory) with a slot key
// (8-aligned, published with agent-scope stores).  `coh` selects coherent
// reads: needed when the slot's FILLED state was learned from an atomic
// rather than from a load of the same (line-contained) slot.
__device__ __forceinline__ bool key_eq(uint64_t slot_key, uint64_t key, uint32_t ks, bool coh) {
  uint32_t i = 0;
  for (; i + 4 <= ks; i += 4) {
    uint32_t kv = *(const u32u *)(key + i);
    if ((coh ? acoh32(slot_key + i) : ald32(slot_key + i)) != kv) return false;
  }
  for (; i < ks; i++) {
    uint64_t w = (slot_key + i) & ~3ull;
    uint32_t v = coh ? acoh32(w) : ald32(w);
    if ((uint8_t)(v >> (((slot_key + i) & 3) * 8)) != *(const volatile uint8_t *)(key + i)) return false;
  }
  return true;
}

__device__ __forceinline__ void copy_bytes_publish(uint64_t dst, uint64_t src, uint32_t n) {
  // dst is 8-aligned device memory; src is any flat address.
  uint32_t i = 0;
  for (; i + 4 <= n; i += 4)
    __hip_atomic_store(G32(dst + i), *(const u32u *)(src + i), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  if (i < n) {
    uint32_t w = 0;
    for (uint32_t j = 0; i + j < n; j++) w |= (uint32_t)(*(const volatile uint8_t *)(src + i + j)) << (8 * j);
    __hip_atomic_store(G32(dst + i), w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__device__ __forceinline__ void copy_bytes(uint64_t dst, uint64_t src, uint32_t n) {
  for (uint32_t i = 0; i < n; i++)
    *(volatile uint8_t *)(dst + i) = *(const volatile uint8_t *)(src + i);
}

constexpr uint32_t ST_EMPTY = 0, ST_FILLED = 1, ST_BUSY = 2;

__device__ __forceinline__ uint64_t ald64(uint64_t a) {
  return __hip_atomic_load(G64(a), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// An insert into a table whose lookup index is valid (common.hpp kIxRes),
// holding the index entry `ea` reserved for its key, which is absent: claim
// the first EMPTY bucket of the reference probe from h % nb
// (bpftime_hash_map.hpp:127-180) -- found through the table's bucket bitmap
// (64 buckets per word, a stale bit is only a failed claim), claimed by
// compare-and-swap on its state -- publish key and value, then the index
// entry.  Never waits on another lane: a lane of the same wave that waits on
// the reservation re-reads it on its next loop trip (hash_find_ix).
#ifdef BPFTIME_AMD_INSERT_STATS
// (experiment build only: insert-path counters, tools/insert_stats.py)
__device__ unsigned long long g_istats[8];
#define ISTAT(i, v) atomicAdd(&g_istats[i], (unsigned long long)(v))
#define ISTAT_MAX(i, v) atomicMax(&g_istats[i], (unsigned long long)(v))
#else
#define ISTAT(i, v) ((void)0)
#define ISTAT_MAX(i, v) ((void)0)
#endif
__device__ uint64_t ix_insert(const DMap &m, uint64_t key, uint64_t h, uint64_t ea, uint64_t init,
                              uint32_t init_bytes, bool *inserted, uint64_t part, uint32_t part_off,
                              uint32_t part_bytes) {
  const uint64_t nb = m.nbuckets, bm = ix_bitmap(m.ix, m.ix_mask, m.key_size), nw = (nb + 63) >> 6;
  uint64_t b = h % nb, left = nb;
  uint32_t words = 0;
  while (left) {
    // the next kScan bitmap words at once (one memory round trip for 64 *
    // kScan buckets: the late inserts of a nearly full table scan far), then
    // the first clear bit in probe order
    constexpr uint32_t kScan = 8;
    uint64_t wv[kScan];
    {
      uint64_t w = b >> 6;
#pragma unroll
      for (uint32_t k = 0; k < kScan; k++) {
        wv[k] = ald64(bm + 8 * w);
        w = w + 1 == nw ? 0 : w + 1;
      }
    }
    bool found = false;
#pragma unroll
    for (uint32_t k = 0; k < kScan; k++) {
      if (!left) break;
      words++;
      const uint64_t o = b & 63;
      uint64_t span = 64 - o;
      if (span > left) span = left;
      if (span > nb - b) span = nb - b;
      uint64_t freeb = ~wv[k] >> o;
      if (span < 64) freeb &= (1ull << span) - 1;
      if (freeb) {
        const uint64_t i = (uint64_t)__builtin_ctzll(freeb);
        b += i;
        left -= i;
        found = true;
        break;
      }
      b += span;
      left -= span;
      if (b == nb) b = 0;
    }
    if (!found) continue;
    const uint64_t s = m.data + b * (uint64_t)m.slot_size;
    const uint64_t bit = 1ull << (b & 63);
    uint32_t prev = ST_EMPTY;
    __hip_atomic_compare_exchange_strong(G32(s), &prev, ST_BUSY, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_or(G64(bm + 8 * (b >> 6)), bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (prev == ST_EMPTY) {
      // the element count check (bpftime_hash_map.hpp:153-156) by the lane
      // that owns the bucket, as in hash_find
      unsigned long long c = __hip_atomic_fetch_add(G64(m.count_addr), 1ull, __ATOMIC_RELAXED,
                                                    __HIP_MEMORY_SCOPE_AGENT);
      if (c >= m.max_entries) {
        __hip_atomic_fetch_add(G64(m.count_addr), ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(G32(s), ST_EMPTY, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_and(G64(bm + 8 * (b >> 6)), ~bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
      copy_bytes_publish(s + m.key_off, key, m.key_size);
      if (init)
        copy_bytes_publish(s + m.val_off, init, init_bytes);
      else
        for (uint32_t k = 0; k < init_bytes; k += 4)
          __hip_atomic_store(G32(s + m.val_off + k), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (part) copy_bytes_publish(s + m.val_off + part_off, part, part_bytes);
      // a keyed index (common.hpp ix_key_stride): the key at the entry's
      // position before the entry is published
      // (one 8- or 16-B store: a reader's line holds all of it or none, so a
      // stale key line reads zero, gen_fast.py index_probe)
      if (const uint32_t ks = ix_key_stride(m.key_size)) {
        uint32_t w[4] = {0, 0, 0, 0};
        for (uint32_t i = 0; i < m.key_size; i++) ((uint8_t *)w)[i] = *(const volatile uint8_t *)(key + i);
        const uint64_t ka = ix_keys(m.ix, m.ix_mask) + (ea - m.ix) / 4 * ks;
        typedef __attribute__((ext_vector_type(2))) uint32_t v2u;
        typedef __attribute__((ext_vector_type(4))) uint32_t v4u;
        if (ks == 8)
          *(__attribute__((address_space(1))) v2u *)(uintptr_t)ka = v2u{w[0], w[1]};
        else
          *(__attribute__((address_space(1))) v4u *)(uintptr_t)ka = v4u{w[0], w[1], w[2], w[3]};
      }
      __atomic_signal_fence(__ATOMIC_SEQ_CST);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // key/value stores drained first
      __hip_atomic_store(G32(s), ST_FILLED, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(G32(ea), (uint32_t)b + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      *inserted = true;
      ISTAT(0, 1);
      ISTAT(1, words);
      ISTAT_MAX(4, words);
      return s;
    }
    ISTAT(2, 1);
    // claimed by another insert: go on after it
    b = b + 1 == nb ? 0 : b + 1;
    left--;
  }
  // full: the reservation goes back (a lane waiting on it tries its own)
  __hip_atomic_store(G32(ea), 0u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  return 0;
}

// hash_find over a valid lookup index: the index holds exactly the keys the
// reference probe reaches (map_hash.cpp ix_rebuild; device inserts index what
// they publish), so walking it from ix_pos(h) to an empty entry decides
// presence without the reference probe's walk of a nearly full table (config
// 3: 65,536 flows in 65,537 buckets).  An empty entry is confirmed at the
// coherence point (a line of this XCD's L2 may predate another XCD's
// insert).  An insert reserves the empty entry that proved its key absent
// (0 -> kIxRes): any other insert of the same key walks the same entries and
// waits at the reservation until it holds the new bucket, so two inserts of
// one key meet in one element; lookups pass reserved entries (an insert in
// flight).  Waiting is re-reading on the next loop trip, never a spin inside
// a trip, so a lane never waits on a lane of its own wave.
__device__ uint64_t hash_find_ix(const DMap &m, uint64_t key, uint64_t h, bool insert, uint64_t init,
                                 uint32_t init_bytes, bool *inserted, uint64_t part, uint32_t part_off,
                                 uint32_t part_bytes) {
  uint32_t p = ix_pos(h, m.ix_mask), spins = 0;
  const uint32_t ks = ix_key_stride(m.key_size);
  ISTAT(insert ? 5 : 6, 1);
  for (uint32_t t = 0; t <= m.ix_mask;) {
    ISTAT(7, 1);
    const uint64_t ea = m.ix + 4ull * p;
    uint32_t e = ald32(ea);
    // an empty entry is confirmed at the coherence point; a reservation is
    // polled with loads, confirmed every 16th trip (thousands of lanes may
    // wait on a hot new key's: same-address atomics serialize)
    if (e == 0 || (e == kIxRes && (spins & 15) == 15)) e = acoh32(ea);
    if (e == 0) {
      if (!insert) return 0;
      uint32_t z = 0;
      if (__hip_atomic_compare_exchange_strong(G32(ea), &z, kIxRes, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT))
        return ix_insert(m, key, h, ea, init, init_bytes, inserted, part, part_off, part_bytes);
      e = z;
    }
    if (e == kIxRes) {
      if (insert) {  // maybe this key's: read the entry again on the next trip
        ISTAT(3, 1);
        if (++spins > (1u << 22)) return 0;  // bounded: never hang the GPU
        __builtin_amdgcn_s_sleep(1);
        continue;
      }
    } else if (ks) {
      // a keyed index: the entry's key was published before the entry (read
      // coherently when the entry was: ix_insert)
      if (key_eq(ix_keys(m.ix, m.ix_mask) + (uint64_t)p * ks, key, m.key_size, true))
        return m.data + (uint64_t)(e - 1) * m.slot_size;
    } else {
      const uint64_t s = m.data + (uint64_t)(e - 1) * m.slot_size;
      uint32_t st = ald32(s);
      bool coh = false;
      if (st != ST_FILLED) {
        st = acoh32(s);
        coh = true;
      }
      if (st == ST_FILLED && key_eq(s + m.key_off, key, m.key_size, coh)) return s;
    }
    p = (p + 1) & m.ix_mask;
    t++;
  }
  return 0;
}

// Find `key`; if absent and `insert`, claim a slot and publish key + init
// value (init == 0 -> zero).  Returns slot address or 0.  A table with a
// valid lookup index goes through it (hash_find_ix); the rest of this
// function is the reference probe, for tables without one.  *inserted tells
// whether this lane created the element.  The probe order is the
// reference's: start at hash % nbuckets, linear, wrap once
// (bpftime_hash_map.hpp:127-180).  Lanes never wait on a lane of their own
// wave: a BUSY slot is re-read on the next loop trip, by which time the
// claiming lane (same wave, same trip) has published it.
// (part / part_off / part_bytes: bytes written over the zero-initialised
// value of a new element before it is published -- a per-CPU element's
// value for the inserting lane's CPU, which a lane adding to that CPU's
// slot right after the publish must not see overwritten)
__device__ uint64_t hash_find(const DMap &m, uint64_t key, bool insert, uint64_t init,
                              uint32_t init_bytes, bool *inserted, uint64_t part = 0, uint32_t part_off = 0,
                              uint32_t part_bytes = 0) {
  *inserted = false;
  const uint64_t nb = m.nbuckets;
  const uint64_t h = key_hash(key, m.key_size);
  if (m.ix) return hash_find_ix(m, key, h, insert, init, init_bytes, inserted, part, part_off, part_bytes);
  uint64_t idx = h % nb;
  uint64_t start = idx;
  uint32_t spins = 0;
  for (;;) {
    uint64_t s = m.data + idx * (uint64_t)m.slot_size;
    // A slot never straddles a 128-B line (map_hash.cpp hash_geometry), so a
    // FILLED state read by a load comes with the key bytes of that same
    // line snapshot.  Anything else is confirmed at the coherence point: a
    // stale EMPTY from this XCD's L2 would end the probe with a false miss.
    uint32_t st = ald32(s);
    bool coh = false;
    if (st != ST_FILLED) {
      st = acoh32(s);
      coh = true;
    }
    if (st == ST_EMPTY) {
      if (!insert) return 0;
      uint32_t prev = ST_EMPTY;
      __hip_atomic_compare_exchange_strong(G32(s), &prev, ST_BUSY, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
      if (prev == ST_EMPTY) {
        // Element count check (bpftime_hash_map.hpp:153-156), made only by
        // the lane that owns the slot: reserving before the claim lets
        // thousands of concurrent losers over-count a table that is not full.
        unsigned long long c = __hip_atomic_fetch_add(G64(m.count_addr), 1ull, __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_AGENT);
        if (c >= m.max_entries) {
          __hip_atomic_fetch_add(G64(m.count_addr), ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(G32(s), ST_EMPTY, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
          return 0;
        }
        copy_bytes_publish(s + m.key_off, key, m.key_size);
        if (init)
          copy_bytes_publish(s + m.val_off, init, init_bytes);
        else
          for (uint32_t i = 0; i < init_bytes; i += 4)
            __hip_atomic_store(G32(s + m.val_off + i), 0u, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        if (part) copy_bytes_publish(s + m.val_off + part_off, part, part_bytes);
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // key/value stores drained first
        __hip_atomic_store(G32(s), ST_FILLED, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        *inserted = true;
        return s;
      }
      st = prev;  // lost the claim: BUSY or FILLED, learned at the coherence point
    }
    if (st == ST_BUSY) {
      if (++spins > (1u << 22)) return 0;  // bounded: never hang the GPU
      __builtin_amdgcn_s_sleep(1);
      continue;  // re-read the same slot on the next trip
    }
    if (key_eq(s + m.key_off, key, m.key_size, coh)) return s;
    idx = idx + 1 == nb ? 0 : idx + 1;
    if (idx == start) return 0;
  }
}

// ---------------------------------------------------------------------------
// LRU hash (runtime/src/bpf_map/userspace/lru_var_hash_map.cpp) over the
// HASH slot layout with tombstones and per-bucket last-use stamps (common.hpp
// DMap, kLruSeqShift).  Every state and key read is made at the coherence
// point: slots change owner within a launch (evictions, deletions, reuse).
//   lookup  (:27-41)  a hit raises the element's stamp (move_to_head)
//   update  (:43-90)  exact flags 0/1/2; an existing key: value + stamp; a new
//                     key claims the first tombstone / empty bucket of its
//                     probe, and past max_entries evicts the smallest stamp:
//                     over every bucket when the batch is ORDERED (the
//                     reference's list tail), over kLruScan buckets from a
//                     hashed start in parallel batches
//   delete  (:92-103) the element becomes a tombstone, ENOENT when absent
// Two parallel inserts of one key converge on one bucket (the first free
// bucket of the same probe), except when a deletion or eviction frees an
// earlier bucket between their probes; the later-probing copy then folds
// itself into the earlier one after publishing (lru_dedup).
// ---------------------------------------------------------------------------
constexpr uint32_t ST_TOMB = 3;

__device__ __forceinline__ uint64_t lru_stamp_at(const DMap &m, uint64_t idx) { return m.count_addr + 128 + 8 * idx; }

__device__ __forceinline__ void lru_touch(const DMap &m, uint64_t idx, uint64_t stamp) {
  __hip_atomic_fetch_max(G64(lru_stamp_at(m, idx)), (unsigned long long)stamp, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
}

// the FILLED bucket holding key (-1 absent, -2 gave up on a BUSY bucket);
// *free_idx = the first tombstone or empty bucket of the probe (-1 none)
__device__ int64_t lru_probe(const DMap &m, uint64_t key, int64_t *free_idx, uint32_t *free_st) {
  const uint64_t nb = m.nbuckets;
  uint64_t idx = key_hash(key, m.key_size) % nb;
  const uint64_t start = idx;
  *free_idx = -1;
  *free_st = ST_EMPTY;
  uint32_t spins = 0;
  for (;;) {
    const uint64_t s = m.data + idx * (uint64_t)m.slot_size;
    const uint32_t st = acoh32(s);
    if (st == ST_BUSY) {
      if (++spins > (1u << 22)) return -2;  // bounded: never hang the GPU
      __builtin_amdgcn_s_sleep(1);
      continue;
    }
    if (st == ST_EMPTY || st == ST_TOMB) {
      if (*free_idx < 0) {
        *free_idx = (int64_t)idx;
        *free_st = st;
      }
      if (st == ST_EMPTY) return -1;
    } else if (key_eq(s + m.key_off, key, m.key_size, true)) {
      return (int64_t)idx;
    }
    idx = idx + 1 == nb ? 0 : idx + 1;
    if (idx == start) return -1;
  }
}

__device__ __forceinline__ bool lru_kill(const DMap &m, uint64_t idx) {
  uint32_t prev = ST_FILLED;
  if (!__hip_atomic_compare_exchange_strong(G32(m.data + idx * (uint64_t)m.slot_size), &prev, ST_TOMB,
                                            __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    return false;
  __hip_atomic_fetch_add(G64(m.count_addr), ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_fetch_add(G64(m.count_addr + 8), 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return true;
}

// evict one element: the smallest stamp among the FILLED buckets examined
__device__ bool lru_evict(const DMap &m, uint64_t h, uint64_t stamp, bool exact) {
  const uint64_t nb = m.nbuckets;
  const uint64_t span = exact || nb <= kLruScan ? nb : kLruScan;
  for (uint32_t attempt = 0; attempt < 16; attempt++) {
    const uint64_t start = span == nb ? 0 : ((h ^ (stamp * 0x9E3779B97F4A7C15ull)) + attempt * span) % nb;
    int64_t best = -1;
    uint64_t bs = ~0ull;
    for (uint64_t k = 0, i = start; k < span; k++, i = i + 1 == nb ? 0 : i + 1) {
      if (acoh32(m.data + i * (uint64_t)m.slot_size) != ST_FILLED) continue;
      const uint64_t t = __hip_atomic_load(G64(lru_stamp_at(m, i)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (t < bs) {
        bs = t;
        best = (int64_t)i;
      }
    }
    if (best >= 0 && lru_kill(m, (uint64_t)best)) return true;
  }
  return false;
}

// After publishing bucket f for key: another copy of key on the probe
// (possible only when a deletion or eviction freed an earlier bucket between
// two inserts' probes) is resolved by probe position, the earlier copy
// staying.  Each insert scans the whole probe once its own copy is visible,
// so of two copies at least the later-scanning insert sees the other one.
// The dropped copy's value is dropped with it, as if its insert had come
// first and the other one had overwritten it.
__device__ void lru_dedup(const DMap &m, uint64_t key, uint64_t f, uint64_t stamp) {
  const uint64_t nb = m.nbuckets;
  const uint64_t home = key_hash(key, m.key_size) % nb;
  const uint64_t fdist = (f + nb - home) % nb;
  uint64_t idx = home;
  uint32_t spins = 0;
  for (uint64_t k = 0; k < nb;) {
    const uint64_t s = m.data + idx * (uint64_t)m.slot_size;
    const uint32_t st = acoh32(s);
    if (st == ST_BUSY && idx != f) {
      if (++spins > (1u << 22)) return;
      __builtin_amdgcn_s_sleep(1);
      continue;
    }
    if (st == ST_EMPTY) return;
    if (idx != f && st == ST_FILLED && key_eq(s + m.key_off, key, m.key_size, true)) {
      if (k < fdist) {  // an earlier copy: this one goes
        if (lru_kill(m, f)) lru_touch(m, idx, stamp);
        return;
      }
      lru_kill(m, idx);  // a later copy goes
    }
    idx = idx + 1 == nb ? 0 : idx + 1;
    k++;
  }
}

__device__ uint64_t lru_lookup(const DMap &m, uint64_t key, uint64_t stamp) {
  int64_t fi;
  uint32_t fst;
  const int64_t idx = lru_probe(m, key, &fi, &fst);
  if (idx < 0) return 0;
  lru_touch(m, (uint64_t)idx, stamp);
  return m.data + (uint64_t)idx * m.slot_size + m.val_off;
}

__device__ uint64_t lru_update(const DMap &m, uint64_t key, uint64_t val, uint64_t flags, uint64_t stamp, bool exact,
                               bool keep_existing) {
  if (flags > 2) return (uint64_t)-1;  // is_good_update_flag (:8-11): EINVAL
  for (uint32_t tries = 0; tries < 64; tries++) {
    int64_t fi;
    uint32_t fst;
    const int64_t idx = lru_probe(m, key, &fi, &fst);
    if (idx == -2) return (uint64_t)-1;
    if (idx >= 0) {
      if (flags == 1) return (uint64_t)-1;  // BPF_NOEXIST: EEXIST
      if (!keep_existing) copy_bytes_publish(m.data + (uint64_t)idx * m.slot_size + m.val_off, val, m.value_size);
      lru_touch(m, (uint64_t)idx, stamp);
      return 0;
    }
    if (flags == 2) return (uint64_t)-1;  // BPF_EXIST: ENOENT
    if (fi < 0) return (uint64_t)-1;      // no free bucket on the probe
    const uint64_t s = m.data + (uint64_t)fi * m.slot_size;
    uint32_t prev = fst;
    if (!__hip_atomic_compare_exchange_strong(G32(s), &prev, ST_BUSY, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT))
      continue;  // the bucket changed under the probe: probe again
    if (fst == ST_TOMB)
      __hip_atomic_fetch_add(G64(m.count_addr + 8), ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long c =
        __hip_atomic_fetch_add(G64(m.count_addr), 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (c >= m.max_entries && !lru_evict(m, key_hash(key, m.key_size), stamp, exact)) {
      // nothing evictable (every element in flight): give the bucket back
      __hip_atomic_fetch_add(G64(m.count_addr), ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_add(G64(m.count_addr + 8), 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(G32(s), ST_TOMB, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      return (uint64_t)-1;
    }
    copy_bytes_publish(s + m.key_off, key, m.key_size);
    copy_bytes_publish(s + m.val_off, val, m.value_size);
    __hip_atomic_store(G64(lru_stamp_at(m, (uint64_t)fi)), (unsigned long long)stamp, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // key / value / stamp before the state
    __hip_atomic_store(G32(s), ST_FILLED, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    if (!exact) lru_dedup(m, key, (uint64_t)fi, stamp);
    return 0;
  }
  return (uint64_t)-1;
}

__device__ uint64_t lru_delete(const DMap &m, uint64_t key) {
  int64_t fi;
  uint32_t fst;
  for (uint32_t tries = 0; tries < 64; tries++) {
    const int64_t idx = lru_probe(m, key, &fi, &fst);
    if (idx < 0) return (uint64_t)-1;  // ENOENT
    if (lru_kill(m, (uint64_t)idx)) return 0;
  }
  return (uint64_t)-1;
}

// LPM trie lookup on the device replica: the walk of lpm_trie_map.cpp:
// 192-264 (longest prefix match down the trie, the last non-intermediate
// node on the path wins; an exact full-length match ends the walk).  The
// replica changes during a batch only in ORDERED batches of a program that
// updates / deletes (lpm_update / lpm_remove below).
__device__ __forceinline__ uint32_t lpm_bit(const uint8_t *d, uint32_t i) { return (d[i >> 3] >> (7 - (i & 7))) & 1; }

__device__ uint64_t lpm_lookup(const DMap &m, uint64_t key) {
  const uint32_t dsz = m.key_size - 4, maxp = dsz * 8;
  const uint32_t kp = *(const u32u *)key;
  if (kp > maxp) return 0;
  const uint8_t *kd = (const uint8_t *)(uintptr_t)(key + 4);
  if (m.ix && kp == 32 && dsz == 4) {
    // IPv4 full-length key: the flat table (lpm_trie.hpp LpmTrie::flat)
    const uint32_t *t = (const uint32_t *)(uintptr_t)m.ix;
    uint32_t e = t[((uint32_t)kd[0] << 16) | ((uint32_t)kd[1] << 8) | kd[2]];
    if (e & 0x80000000u) e = t[(1u << 24) + 256u * (e & 0x7fffffffu) + kd[3]];
    return e ? m.data + 16 + (uint64_t)(e - 1) * m.slot_size + m.val_off : 0;
  }
  int32_t node = *(const int32_t *)(uintptr_t)m.data;
  uint64_t found = 0;
  for (uint32_t guard = 0; node >= 0 && guard <= maxp + 1; guard++) {
    const uint64_t nb = m.data + 16 + (uint64_t)node * m.slot_size;
    const uint32_t np = *(const uint32_t *)(uintptr_t)nb;
    const bool inter = *(const uint32_t *)(uintptr_t)(nb + 4) != 0;
    const uint8_t *nd = (const uint8_t *)(uintptr_t)(nb + m.key_off);
    const uint32_t lim = np < kp ? np : kp;
    uint32_t ml = 0;
    while (ml + 8 <= lim && nd[ml >> 3] == kd[ml >> 3]) ml += 8;  // whole bytes first
    while (ml < lim && lpm_bit(nd, ml) == lpm_bit(kd, ml)) ml++;
    if (ml == maxp) {
      found = inter ? 0 : nb;
      break;
    }
    if (ml < np) break;
    if (!inter) found = nb;
    if (ml >= kp) break;
    node = *(const int32_t *)(uintptr_t)(nb + 8 + 4 * lpm_bit(kd, np));
  }
  return found ? found + m.val_off : 0;
}

// Program-side LPM trie writes, ORDERED batches only (one lane runs the
// units in order; vm_upkeep.cpp refuses other batches of such programs):
// lpm_trie_map.cpp:266-488 (elem_update) and :490-541 (elem_delete, a
// logical deletion: the node becomes intermediate) restated over the
// replica exactly as the host's LpmTrie::update / remove (lpm_trie.hpp) do over
// its node pool -- new nodes appended at index `nodes`, the same numbering,
// so the host takes the replica back as its trie after the batch
// (map_lpm.cpp lpm_pull).  Replica header {i32 root, u32 nodes, u32 entries,
// u32 cap}; a node {u32 plen, u32 intermediate, i32 child[2], data at
// key_off, value at val_off}.  Errors return -1 like the reference helper.
struct LpmHdr {
  int32_t root;
  uint32_t nodes, entries, cap;  // (cap | kLpmPoolOut: an update found the pool full)
};

__device__ __forceinline__ uint32_t lpm_match(const DMap &m, uint64_t nb, const uint8_t *kd, uint32_t kp) {
  const uint32_t np = *(const uint32_t *)(uintptr_t)nb;
  const uint8_t *nd = (const uint8_t *)(uintptr_t)(nb + m.key_off);
  const uint32_t lim = np < kp ? np : kp;
  uint32_t ml = 0;
  while (ml < lim && lpm_bit(nd, ml) == lpm_bit(kd, ml)) ml++;
  return ml;
}

__device__ uint64_t lpm_update(const DMap &m, uint64_t key, uint64_t val, uint64_t flags) {
  if (flags != 0 && flags != 1 && flags != 2) return (uint64_t)-1;  // EINVAL
  const uint32_t dsz = m.key_size - 4, maxp = dsz * 8, vsz = m.value_size;
  const uint32_t kp = *(const u32u *)key;
  if (kp > maxp) return (uint64_t)-1;  // EINVAL
  const uint8_t *kd = (const uint8_t *)(uintptr_t)(key + 4);
  LpmHdr *h = (LpmHdr *)(uintptr_t)m.data;
  auto at = [&](int32_t i) { return m.data + 16 + (uint64_t)i * m.slot_size; };
  auto plen = [&](int32_t i) -> uint32_t & { return *(uint32_t *)(uintptr_t)at(i); };
  auto inter = [&](int32_t i) -> uint32_t & { return *(uint32_t *)(uintptr_t)(at(i) + 4); };
  auto child = [&](int32_t i, uint32_t b) -> int32_t & { return *(int32_t *)(uintptr_t)(at(i) + 8 + 4 * b); };
  auto value = [&](int32_t i) { return at(i) + m.val_off; };
  auto need_room = [&]() {
    if (flags == 2) return false;                    // ENOENT
    if (h->entries >= m.max_entries) return false;   // ENOSPC
    // the replica's node pool (map_lpm.cpp): running out of it is no answer
    // the reference gives (its heap grows), so it is flagged in the
    // header and the host fails the batch (map_lpm.cpp lpm_pull)
    if (h->nodes + 2 <= (h->cap & ~kLpmPoolOut)) return true;
    h->cap |= kLpmPoolOut;
    return false;
  };
  auto make = [&](uint32_t p, bool in) -> int32_t {
    const int32_t i = (int32_t)h->nodes++;
    plen(i) = p;
    inter(i) = in ? 1u : 0u;
    child(i, 0) = child(i, 1) = -1;
    copy_bytes(at(i) + m.key_off, (uint64_t)(uintptr_t)kd, dsz);
    for (uint32_t j = 0; j < vsz; j++) ((uint8_t *)(uintptr_t)value(i))[j] = 0;
    if (!in) copy_bytes(value(i), val, vsz);
    return i;
  };
  if (h->root < 0) {
    if (!need_room()) return (uint64_t)-1;
    h->root = make(kp, false);
    h->entries++;
    return 0;
  }
  int32_t parent = -1, cur = h->root;
  uint32_t pbit = 0, ml = 0;
  while (cur >= 0) {
    ml = lpm_match(m, at(cur), kd, kp);
    const uint32_t np = plen(cur);
    if (np != ml || np == kp || np == maxp) break;
    parent = cur;
    pbit = lpm_bit(kd, np);
    cur = child(cur, pbit);
  }
  auto set_slot = [&](int32_t v) {
    if (parent < 0)
      h->root = v;
    else
      child(parent, pbit) = v;
  };
  auto split = [&](int32_t c) {  // an intermediate node at the split point
    const int32_t nn = make(kp, false);
    const int32_t im = make(ml, true);
    const uint32_t b = lpm_bit(kd, ml);
    child(im, b) = nn;
    child(im, b ^ 1) = c;
    set_slot(im);
    h->entries++;
    return (uint64_t)0;
  };
  if (cur >= 0 && plen(cur) == kp) {  // case 1
    if (lpm_match(m, at(cur), kd, kp) == kp) {
      if (flags == 1) return (uint64_t)-1;               // EEXIST
      if (flags == 2 && inter(cur)) return (uint64_t)-1;  // ENOENT
      if (inter(cur)) {
        if (h->entries >= m.max_entries) return (uint64_t)-1;  // ENOSPC
        inter(cur) = 0;
        h->entries++;
      }
      copy_bytes(value(cur), val, vsz);
      return 0;
    }
    if (!need_room()) return (uint64_t)-1;
    return split(cur);
  }
  if (cur < 0) {  // case 2
    if (!need_room()) return (uint64_t)-1;
    set_slot(make(kp, false));
    h->entries++;
    return 0;
  }
  if (ml == kp) {  // case 3: the new prefix becomes cur's parent
    if (!need_room()) return (uint64_t)-1;
    const int32_t nn = make(kp, false);
    child(nn, lpm_bit((const uint8_t *)(uintptr_t)(at(cur) + m.key_off), ml)) = cur;
    set_slot(nn);
    h->entries++;
    return 0;
  }
  if (!need_room()) return (uint64_t)-1;  // case 4
  return split(cur);
}

__device__ uint64_t lpm_remove(const DMap &m, uint64_t key) {
  const uint32_t dsz = m.key_size - 4;
  const uint32_t kp = *(const u32u *)key;
  if (kp > dsz * 8) return (uint64_t)-1;  // EINVAL
  const uint8_t *kd = (const uint8_t *)(uintptr_t)(key + 4);
  LpmHdr *h = (LpmHdr *)(uintptr_t)m.data;
  auto at = [&](int32_t i) { return m.data + 16 + (uint64_t)i * m.slot_size; };
  int32_t cur = h->root, last = -1;
  while (cur >= 0) {
    last = cur;
    const uint32_t np = *(const uint32_t *)(uintptr_t)at(cur);
    if (np != lpm_match(m, at(cur), kd, kp) || np == kp) break;
    cur = *(const int32_t *)(uintptr_t)(at(cur) + 8 + 4 * lpm_bit(kd, np));
    last = cur;
  }
  if (last < 0) return (uint64_t)-1;  // ENOENT
  const uint64_t nb = at(last);
  uint32_t *in = (uint32_t *)(uintptr_t)(nb + 4);
  if (*(const uint32_t *)(uintptr_t)nb != kp || lpm_match(m, nb, kd, kp) != kp || *in) return (uint64_t)-1;
  *in = 1;
  for (uint32_t j = 0; j < m.value_size; j++) ((uint8_t *)(uintptr_t)(nb + m.val_off))[j] = 0;
  if (h->entries) h->entries--;
  return 0;
}

// ---------------------------------------------------------------------------
// Ring buffer (runtime/src/bpf_map/userspace/ringbuf_map.cpp, helpers
// bpf_helper.cpp:451-504).  Records are [u32 len | BUSY | DISCARD][i32 fd]
// + data, 8-aligned, at data + (pos & mask).  A reservation moves the
// producer position with a CAS after checking room against the consumer
// position, like ringbuf::reserve under its spin lock.  The lanes of a wave
// that reserve from one ring take one CAS for all of them (their records are
// laid out in lane order); a ring too full for the whole wave falls back to
// lane-by-lane reservations, so each reservation succeeds or fails exactly
// as a serial one would at that point.
// ---------------------------------------------------------------------------
constexpr uint32_t RB_BUSY = 0x80000000u, RB_DISCARD = 0x40000000u, RB_HDR = 8;
constexpr uint64_t kRbMaxWaves = 256 * 32;                 // CUs x resident waves per CU (upper bound)
constexpr uint64_t kRbWaveMax = 4096;                      // largest wave reservation on the fast path
constexpr uint64_t kRbSlack = kRbMaxWaves * kRbWaveMax;    // 32 MiB

// Block staging of ring-buffer records.  A block does not move the ring's
// producer position per record (a same-address atomic at the memory side,
// ~40 ns each under the whole chip's contention: it bounded the sampler at
// 1.5 Gpps).  Its first reservation, when the ring has ample room (the fast
// path's condition, counting promises), PROMISES itself kRbStageRec bytes:
// an add to the ring's promise counter (at data + 192), no ring position.
// The block's waves then claim records inside that budget with an LDS
// compare-and-swap on the bytes used, writing them to a per-block staging
// area.  When the block ends it reserves exactly the bytes it used with one
// fetch-and-add of the producer position, copies its records there and
// returns its promise: no ring byte is ever wasted, so a ring that goes from
// ample room to full inside one launch accepts exactly what a serial run
// accepts (the reference's ringbuf::reserve, ringbuf_map.cpp:262-295).
// Every reservation counts the outstanding promises as taken
// (rb_room), so a promised byte is always there at the block's end.  A
// reservation that does not fit while promises are outstanding first closes
// its own block's staging (the block's used bytes are reserved at once, its
// promise returned: a closed block's waves reserve directly) and then waits
// for the other blocks' promises to come back -- they do when those blocks
// end or close; no new promise is made that close to full -- so it fails only
// when the ring is really full, as a serial reservation would.  A wave whose
// records do not fit the block's budget reserves directly.  The consumer,
// bpftime_amd_ringbuf_fetch, synchronizes the device before it reads.
// Consumers see the same records in another parallel order.
// (sizes: common.hpp kRbStage*)
constexpr uint32_t kRbClosed = 0x80000000u;  // RbStage::used: the block's staging is closed
struct RbLds {       // LDS: the block's staging counters
  uint32_t used;     // bytes claimed (| kRbClosed)
  uint32_t nrec;     // records
  int32_t fd;        // the ring of the block's promise (-1 undecided, -3 deciding, -2 none)
  uint32_t pad;
  uint64_t base;     // the ring position of the block's records (set when it closes)
};
// (two pointers, passed by value: a struct the helpers take by reference
// lives in scratch, written by every lane of every launch)
struct RbStage {
  uint8_t *buf = nullptr;  // this block's area: records, then u32 offsets (nullptr: no staging)
  RbLds *lds = nullptr;
};

// the ring's room for a reservation: capacity - (producer - consumer) -
// the bytes blocks have promised themselves (RbStage)
__device__ __forceinline__ int64_t rb_room(const DMap &m, uint64_t *prod_out = nullptr) {
  const uint64_t cons = __hip_atomic_load(G64(m.data), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const uint64_t prod = __hip_atomic_load(G64(m.data + 128), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const uint64_t prom = __hip_atomic_load(G64(m.data + 192), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (prod_out) *prod_out = prod;
  return (int64_t)m.max_entries - (int64_t)(prod - cons) - (int64_t)prom;
}

// Close the block's staging (a reservation of the block needs the exact
// path): no claim succeeds after this, the bytes claimed so far are
// reserved in the ring now (rb_publish copies them there) and the promise
// is returned.
__device__ void rb_close(const DMap &m, RbStage st) {
  if (!st.buf || st.lds->fd < 0) return;
  const uint32_t u = __hip_atomic_fetch_or(&st.lds->used, kRbClosed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  if (u & kRbClosed) return;  // (closed by another wave of the block)
  st.lds->base = u ? __hip_atomic_fetch_add(G64(m.data + 128), (uint64_t)u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
               : 0;
  __hip_atomic_fetch_add(G64(m.data + 192), (uint64_t)0 - kRbStageRec, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint64_t rb_cas_reserve(const DMap *maps, const DMap &m, uint64_t total, RbStage st,
                                                   int32_t fd) {
  // returns the old producer position, or ~0 if total does not fit.  The
  // loop ends by a successful CAS or a failed room check, as the
  // reference's spin-locked reserve does: the consumer position does not
  // move while a launch runs (its only consumer, bpftime_amd_ringbuf_fetch,
  // synchronizes the device first), every lost CAS means another
  // reservation moved the producer position by >= 8 bytes, and promises
  // only come back.  A room that only the outstanding promises take is
  // waited for, this block's own promise returned first (rb_close) -- on
  // whichever ring it is: a block waiting on ring B while it holds a
  // promise on ring A could otherwise wait for a block that waits on A
  // (ADVICE r04), so no block waits holding a promise.
  uint32_t backoff = 1;
  const uint64_t bound = (uint64_t)m.max_entries / 8 + (1u << 20);
  for (uint64_t spin = 0; spin < bound; spin++) {
    uint64_t p;
    const int64_t room = rb_room(m, &p);
    if (room < (int64_t)total) {
      const uint64_t prom = __hip_atomic_load(G64(m.data + 192), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (!prom) return ~0ull;  // full, with nothing promised: the serial answer
      // (a launch without staging waits only)
      if (st.buf) {
        const int32_t pfd = __hip_atomic_load(&st.lds->fd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (pfd >= 0 && pfd < (int32_t)kMaxFds) rb_close(pfd == fd ? m : maps[pfd], st);
      }
    } else {
      unsigned long long e = p;
      if (__hip_atomic_compare_exchange_strong(G64(m.data + 128), &e, p + total, __ATOMIC_RELAXED,
                                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        return p;
    }
    // lost to another wave, or waiting for promises: back off (thousands of
    // waves share these words)
    for (uint32_t i = 0; i < backoff; i++) __builtin_amdgcn_s_sleep(2);
    backoff = backoff < 64 ? 2 * backoff : 64;
  }
  return ~0ull;
}

// The calling lanes that reserve from one ring (rb_reserve groups them).
__device__ uint64_t rb_reserve_ring(const DMap *maps, uint64_t fd, uint64_t size, RbStage st) {
  const bool ok = fd < kMaxFds && maps[fd < kMaxFds ? fd : 0].type == MT_RINGBUF &&
                  !(size & (RB_BUSY | RB_DISCARD));
  const DMap m = maps[ok ? fd : 0];
  const uint64_t total = ok ? (size + RB_HDR + 7) / 8 * 8 : 0;
  const bool fits = ok && total <= m.max_entries;
  // one CAS for the wave when every calling lane reserves from the same ring
  const uint64_t active = __ballot(1);
  const uint32_t me = __lane_id(), leader = (uint32_t)__builtin_ctzll(active);
  const uint64_t lfd = __shfl(fd, leader);
  uint64_t pos = ~0ull;
  if (__ballot(!fits || fd != lfd) == 0) {
    uint64_t before = 0, sum = 0;
    for (uint64_t rest = active; rest; rest &= rest - 1) {
      const uint32_t l = (uint32_t)__builtin_ctzll(rest);
      const uint64_t t = __shfl(total, l);
      if (l < me) before += t;
      sum += t;
    }
    if (st.buf) {
      // block staging (RbStage): the block's first reservation reserves
      // its chunk (a wave arriving while another decides reserves directly)
      int32_t sfd = __shfl(__hip_atomic_load(&st.lds->fd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP), leader);
      if (sfd == -1) {
        if (me == leader) {
          int32_t cur = -1;
          if (__hip_atomic_compare_exchange_strong(&st.lds->fd, &cur, -3, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_WORKGROUP)) {
            int32_t got = -2;
            // the fast path's condition (below), for a block's budget
            if (m.max_entries >= 2 * kRbSlack && rb_room(m) >= (int64_t)(kRbStageRec + kRbSlack)) {
              __hip_atomic_fetch_add(G64(m.data + 192), (uint64_t)kRbStageRec, __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_AGENT);
              got = (int32_t)fd;
            }
            __hip_atomic_store(&st.lds->fd, got, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            cur = got;
          }
          sfd = cur;
        }
        sfd = __shfl(sfd, leader);
      }
      if (sfd == (int32_t)fd) {
        uint32_t base = ~0u, rbase = 0;
        const uint32_t cnt = (uint32_t)__builtin_popcountll(active);
        if (me == leader) {
          // claim sum bytes of the budget (a compare-and-swap, so the used
          // count is exactly the claimed bytes: rb_close reserves them)
          uint32_t u = __hip_atomic_load(&st.lds->used, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          for (;;) {
            if ((u & kRbClosed) || (uint64_t)u + sum > kRbStageRec) {
              base = ~0u;  // closed, or the budget is spent: direct
              break;
            }
            if (__hip_atomic_compare_exchange_strong(&st.lds->used, &u, u + (uint32_t)sum, __ATOMIC_RELAXED,
                                                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) {
              base = u;  // (then the record slots fit too: >= 8 B each)
              rbase = __hip_atomic_fetch_add(&st.lds->nrec, cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
              break;
            }
          }
        }
        base = __shfl(base, leader);
        rbase = __shfl(rbase, leader);
        if (base != ~0u) {
          const uint32_t off = base + (uint32_t)before;
          const uint32_t rank = (uint32_t)__builtin_popcountll(active & ((1ull << me) - 1));
          uint8_t *rec = st.buf + off;
          *(uint32_t *)rec = (uint32_t)size | RB_BUSY;
          *(int32_t *)(rec + 4) = (int32_t)fd;
          ((uint32_t *)(st.buf + kRbStageRec))[rbase + rank] = off;
          return (uint64_t)(uintptr_t)(rec + RB_HDR);
        }
      }
    }
    uint64_t base = ~0ull;
    if (me == leader) {
      // Plenty of room: a fetch-and-add (same-address atomics serialize at
      // the memory side, ~12 ns each, while a CAS retry loop under the
      // contention of thousands of waves costs microseconds per record).
      // Safe because at most kRbMaxWaves reservations of <= kRbWaveMax
      // bytes can be between their room check and their add, so an add
      // admitted with kRbSlack bytes to spare never overruns the consumer.
      if (sum <= kRbWaveMax && rb_room(m) >= (int64_t)(sum + kRbSlack))
        base = __hip_atomic_fetch_add(G64(m.data + 128), sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else
        base = rb_cas_reserve(maps, m, sum, st, (int32_t)fd);
    }
    base = __shfl(base, leader);
    if (base != ~0ull) pos = base + before;
  }
  if (pos == ~0ull && fits) {  // lane by lane (full ring, mixed rings)
    for (uint64_t rest = __ballot(1); rest; rest &= rest - 1)
      if ((uint32_t)__builtin_ctzll(rest) == me) pos = rb_cas_reserve(maps, m, total, st, (int32_t)fd);
  }
  if (pos == ~0ull) return 0;
  const uint64_t mask = m.max_entries - 1, d = m.data + 256;
  __hip_atomic_store(G32(d + (pos & mask)), (uint32_t)size | RB_BUSY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(G32(d + (pos & mask) + 4), (uint32_t)fd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return d + ((pos + RB_HDR) & mask);
}

// bpf_ringbuf_reserve (bpf_helper.cpp:468-474) for the calling lanes: one
// group per distinct ring fd, each reserved the wave way (a wave whose lanes
// write two rings took the lane-by-lane path for all of them: one
// contended compare-and-swap per record)
__device__ uint64_t rb_reserve(const DMap *maps, uint64_t fd, uint64_t size, RbStage st) {
  const uint64_t all = __ballot(1);
  uint64_t done = 0, out = 0;
  while (all & ~done) {
    const uint64_t f0 = __shfl(fd, (uint32_t)__builtin_ctzll(all & ~done));
    if (fd == f0) out = rb_reserve_ring(maps, fd, size, st);
    done |= __ballot(fd == f0);
  }
  return out;
}

// fd < 0: the ring named by the record header's fd, ptr[-1]
// (bpf_helper.cpp:478-479, bpf_ringbuf_submit / _discard); for a record
// whose data wrapped to the ring's first byte that word is the zeroed end of
// the position area, fd 0, as the reference reads the zeroed end of its
// producer page.  bpf_ringbuf_output passes the fd it reserved from
// (bpf_helper.cpp:460-465).
__device__ void rb_submit(const DMap *maps, uint64_t sample, bool discard, RbStage st, int32_t fd = -1) {
  if (st.buf && sample >= (uint64_t)(uintptr_t)st.buf + RB_HDR &&
      sample < (uint64_t)(uintptr_t)st.buf + kRbStageRec) {  // a staged record: published at block end
    uint32_t *h = (uint32_t *)(uintptr_t)(sample - RB_HDR);
    *h = (*h & ~RB_BUSY) | (discard ? RB_DISCARD : 0u);
    return;
  }
  if (fd < 0) fd = *(const int32_t *)(uintptr_t)(sample - 4);
  if (fd < 0 || fd >= (int32_t)kMaxFds) return;
  const DMap m = maps[fd];
  if (m.type != MT_RINGBUF) return;
  const uint64_t mask = m.max_entries - 1, d = m.data + 256;
  const uint64_t hdr = d + ((mask + 1 + (sample - d) - RB_HDR) & mask);
  const uint32_t v = __hip_atomic_load(G32(hdr), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the record's bytes before its header
  __hip_atomic_exchange(G32(hdr), (v & ~RB_BUSY) | (discard ? RB_DISCARD : 0u), __ATOMIC_RELEASE,
                        __HIP_MEMORY_SCOPE_AGENT);
}

__device__ uint64_t rb_output(const DMap *maps, uint64_t fd, uint64_t data, uint64_t size, RbStage st) {
  const uint64_t buf = rb_reserve(maps, fd, size, st);
  if (!buf) return (uint64_t)-1;
  copy_bytes(buf, data, (uint32_t)size);
  rb_submit(maps, buf, false, st, (int32_t)fd);
  return 0;
}

// The block's staged records into the ring (every wave of the block is
// done; called by every thread of the block): thread 0 reserves exactly the
// bytes the block used (unless a wave closed the block's staging, which
// reserved them then) and returns the block's promise; then one thread per
// record copies it, with the flags submit / discard gave it.
__device__ void rb_publish(const DMap *maps, RbStage st, uint32_t tid, uint32_t nthreads) {
  if (!st.buf) return;
  const int32_t fd = st.lds->fd;
  if (fd < 0) return;
  const DMap m = maps[fd];
  const uint32_t used = st.lds->used & ~kRbClosed;
  if (tid == 0 && !(st.lds->used & kRbClosed)) {
    st.lds->base = used ? __hip_atomic_fetch_add(G64(m.data + 128), (uint64_t)used, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT)
                    : 0;
    __hip_atomic_fetch_add(G64(m.data + 192), (uint64_t)0 - kRbStageRec, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  const uint64_t base = st.lds->base, mask = m.max_entries - 1, d = m.data + 256;
  const uint32_t n = min(st.lds->nrec, kRbStageMaxRec);
  const uint32_t *offs = (const uint32_t *)(st.buf + kRbStageRec);
  for (uint32_t i = tid; i < n; i += nthreads) {
    const uint32_t off = offs[i];
    const uint32_t h = *(const uint32_t *)(st.buf + off);
    const uint32_t total = ((h & ~(RB_BUSY | RB_DISCARD)) + RB_HDR + 7) / 8 * 8;
    const uint64_t *src = (const uint64_t *)(st.buf + off);
    // where a direct reservation puts them (rb_reserve): the header at the
    // position, the data contiguous from the position after it -- at the
    // ring's start when the header takes its last 8 bytes (the ring area is
    // 2 x max_entries bytes, as the reference's is)
    const uint64_t pos = base + off;
    *(uint64_t *)(uintptr_t)(d + (pos & mask)) = src[0];
    uint64_t *dst = (uint64_t *)(uintptr_t)(d + ((pos + RB_HDR) & mask));
    for (uint32_t w = 1; w < total / 8; w++) dst[w - 1] = src[w];
  }
}

struct LaneEnv {
  uint64_t vcpu;
  uint64_t lru_stamp;  // this unit's LRU stamp base (common.hpp kLruSeqShift)
  uint32_t lru_ops;    // LRU operations the unit has made (the stamp's low byte)
  bool exact;          // ORDERED batch: LRU evictions scan every bucket
  uint64_t scratch;  // this lane's scratch word (KParams::lane_scratch), 0 = none
  // last lookup miss (map fd, key hash) for the lookup_or_try_init race rule
  int32_t miss_fd;
  uint64_t miss_hash;
  RbStage rb;        // the block's ring-buffer staging (RbStage)
  // syscall dispatch state of this unit (KParams::sys_state / sys_ret), the
  // bit this batch's phase sets; null outside a dispatch
  uint32_t *ovr_state;
  int64_t *ovr_val;
  uint32_t ovr_bit;
  uint64_t pid_tgid;  // bpf_get_current_pid_tgid's value for this unit
  uint64_t ktime;     // bpf_ktime_get_ns's value for this unit (a replay's recorded clock) ...
  bool kt_on;         // ... when set, else the device clock
};

// bpftime_override_return / bpftime_set_retval (attach/base_attach_impl/
// base_attach_impl.hpp:76-105): the dispatch's return callback records the
// value (syscall_trace_attach_impl.cpp:35-40); with no callback set the
// reference throws, which fails the unit here
__device__ __forceinline__ uint64_t helper_set_retval(uint64_t v, LaneEnv &env, uint32_t *err) {
  if (!env.ovr_state) {
    *err = E_BADOP;
    return 0;
  }
  *env.ovr_state |= env.ovr_bit;
  if (env.ovr_val) *env.ovr_val = (int64_t)v;
  return 0;
}

__device__ __forceinline__ uint64_t lru_next_stamp(LaneEnv &env) {
  const uint32_t op = env.lru_ops < 255 ? env.lru_ops : 255;
  env.lru_ops++;
  return env.lru_stamp | op;
}

// A map's descriptor for a helper call: through the scalar cache when every
// calling lane names the same map (the usual case: an lddw constant), else
// per lane.  The table only changes between launches.
__device__ __forceinline__ DMap load_dmap(const DMap *maps, uint64_t fd) {
  const uint32_t f0 = __builtin_amdgcn_readfirstlane((uint32_t)fd);
  if (__ballot(fd != f0) == 0) {
    typedef unsigned int u32x4c __attribute__((ext_vector_type(4)));
    typedef const u32x4c __attribute__((address_space(4))) *cvec;
    const cvec q = (cvec)(maps + f0);
    const u32x4c w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3];
    DMap m;
    __builtin_memcpy((uint8_t *)&m, &w0, 16);
    __builtin_memcpy((uint8_t *)&m + 16, &w1, 16);
    __builtin_memcpy((uint8_t *)&m + 32, &w2, 16);
    __builtin_memcpy((uint8_t *)&m + 48, &w3, 16);
    return m;
  }
  return maps[fd];
}

// ---------------------------------------------------------------------------
// BLOOM_FILTER (bloom_filter.cpp): bpf_map_push_elem / bpf_map_peek_elem
// (helpers 87 / 89, bpf_helper.cpp:410-429).  A probe is the bit jhash(value,
// value_size, seed + i) & mask of the array, i < nr_hashes; the bits live in
// 32-bit words read with agent-scope loads and set with agent-scope atomic
// ORs.  A bit is never cleared while a launch runs, so a word read from an
// XCD's L2 that another XCD's push has since changed only misses bits: a
// parallel batch's peek answers for some array between the one before the
// batch and the final one.  ORDERED batches (`coh`) read at the coherence
// point, where the one lane's earlier ORs were performed.
// ---------------------------------------------------------------------------
constexpr uint32_t kBloomMaxHashes = 15;  // map_extra & 0xF
constexpr uint32_t kBloomRegWords = 12;   // values of up to 48 bytes are hashed from registers

// Word i of the value as jhash sees it (little-endian, zero past the value's
// end), from a flat address of any alignment (a lane's stack, packet bytes).
__device__ __forceinline__ uint32_t bloom_value_word(uint64_t v, uint32_t i, uint32_t vs) {
  const uint32_t off = 4 * i;
  if (off + 4 <= vs) return *(const u32u *)(v + off);
  uint32_t w = 0;
  for (uint32_t j = 0; j < 3; j++)
    if (off + j < vs) w |= (uint32_t)(*(const volatile uint8_t *)(v + off + j)) << (8 * j);
  return w;
}

struct BloomVal {
  uint32_t w[kBloomRegWords];
};

// common.hpp bloom_jhash_words over the value's words held in registers: the
// value size is wave-uniform (scalar branches), every index a constant
__device__ __forceinline__ uint32_t bloom_hash_reg(const BloomVal &x, uint32_t vs, uint32_t initval) {
  uint32_t a, b, c;
  a = b = c = 0xdeadbeefu + vs + initval;
  uint32_t t0 = x.w[0], t1 = x.w[1], t2 = x.w[2];  // the last (partial or whole) 12 bytes
#pragma unroll
  for (uint32_t blk = 0; blk + 1 < kBloomRegWords / 3; blk++) {
    if (vs > 12 * (blk + 1)) {
      a += x.w[3 * blk];
      b += x.w[3 * blk + 1];
      c += x.w[3 * blk + 2];
      BA_JMIX(a, b, c)
      t0 = x.w[3 * blk + 3];
      t1 = x.w[3 * blk + 4];
      t2 = x.w[3 * blk + 5];
    }
  }
  a += t0;
  b += t1;
  c += t2;
  BA_JFINAL(a, b, c)
  return c;
}

// ... and for longer values, from memory on every probe
__device__ __forceinline__ uint32_t bloom_hash_mem(uint64_t v, uint32_t vs, uint32_t initval) {
  uint32_t a, b, c, i = 0, rem = vs;
  a = b = c = 0xdeadbeefu + vs + initval;
  for (; rem > 12; rem -= 12, i += 3) {
    a += bloom_value_word(v, i, vs);
    b += bloom_value_word(v, i + 1, vs);
    c += bloom_value_word(v, i + 2, vs);
    BA_JMIX(a, b, c)
  }
  a += bloom_value_word(v, i, vs);
  b += bloom_value_word(v, i + 1, vs);
  c += bloom_value_word(v, i + 2, vs);
  BA_JFINAL(a, b, c)
  return c;
}

// push (PUSH: sets the value's bits, returns 0) or peek (0 when every bit is
// set, else -1; never writes *value).  Three passes, each unrolled over the
// 15 possible probes under the wave-uniform nr_hashes: the bit positions,
// then every word load, then the tests -- so the loads are all in flight
// before the first is waited for.  A push issues an atomic OR only for a bit
// its load found clear: a hot value costs loads, not atomics.
template <bool PUSH>
__device__ __forceinline__ uint64_t bloom_probe(const DMap &m, uint64_t value, bool coh) {
  const uint32_t vs = m.value_size, k = bloom_hashes(m), seed = bloom_seed(m), mask = bloom_mask(m);
  uint32_t pos[kBloomMaxHashes], word[kBloomMaxHashes];
  if (vs <= 4 * kBloomRegWords) {
    BloomVal x;
#pragma unroll
    for (uint32_t i = 0; i < kBloomRegWords; i++) x.w[i] = bloom_value_word(value, i, vs);
#pragma unroll
    for (uint32_t i = 0; i < kBloomMaxHashes; i++) pos[i] = i < k ? bloom_hash_reg(x, vs, seed + i) & mask : 0;
  } else {
#pragma unroll
    for (uint32_t i = 0; i < kBloomMaxHashes; i++) pos[i] = i < k ? bloom_hash_mem(value, vs, seed + i) & mask : 0;
  }
#pragma unroll
  for (uint32_t i = 0; i < kBloomMaxHashes; i++) {
    const uint64_t a = m.data + 4ull * (pos[i] >> 5);
    word[i] = i < k ? (coh ? acoh32(a) : ald32(a)) : ~0u;
  }
  bool all = true;
#pragma unroll
  for (uint32_t i = 0; i < kBloomMaxHashes; i++) {
    const uint32_t bit = 1u << (pos[i] & 31);
    if (PUSH) {
      if (i < k && !(word[i] & bit))
        __hip_atomic_fetch_or(G32(m.data + 4ull * (pos[i] >> 5)), bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      all = all && (word[i] & bit);
    }
  }
  return PUSH || all ? 0 : (uint64_t)-1;
}

// The Bloom filter helpers' one entry (interp.hip call_helper, which sends a
// Bloom filter's helper-2 calls here too).  op: the helper id --
//   87 bpf_map_push_elem(map, value, flags)  bloom_filter.cpp:337-362
//   88 bpf_map_pop_elem(map, value)          :364-369 (nothing to pop)
//   89 bpf_map_peek_elem(map, value)         :371-393
//    2 bpf_map_update_elem on a Bloom filter :291-322 (a push, the key ignored)
// 87 / 88 / 89 on any other map type but QUEUE / STACK (helper_qs below):
// -ENOTSUP (map_handler.cpp:1378-1468).
__device__ __noinline__ uint64_t helper_bloom(const DMap *maps, uint64_t fd, uint64_t value, uint64_t flags,
                                              uint32_t op, bool exact) {
  if (fd >= kMaxFds) return (uint64_t)-1;
  const DMap m = load_dmap(maps, fd);
  if (m.type != MT_BLOOM_FILTER) return (uint64_t)(int64_t)-95;  // -ENOTSUP
  if (op == 88 || !value) return (uint64_t)-1;                    // EOPNOTSUPP / EINVAL
  if (op == 89) return bloom_probe<false>(m, value, exact);
  if (flags != 0) return (uint64_t)-1;                            // BPF_ANY only
  return bloom_probe<true>(m, value, exact);
}

// ---------------------------------------------------------------------------
// QUEUE / STACK (queue.cpp, stack.cpp): one ring for both (common.hpp, QUEUE /
// STACK).  `head` and `tail` are u64 tickets in the ring's header line; the
// element with ticket t lives in slot t % max_entries; count = tail - head.
//
// A parallel launch sees one kind of access per map (the loader's call-site
// analysis and vm_upkeep.cpp's launch check: add-only, remove-only or peek-only),
// so only one end moves while it runs and nothing reads a slot that a push of
// the same launch claimed.  The calling lanes of a wave that name the same
// map form a group; its first lane claims `take` tickets for all of them with
// one agent-scope compare-and-swap on the moving end (the scope rb_reserve
// uses) -- retried only when another wave moved that end, never waiting for a
// value another lane must produce -- and the group's lanes, ranked by lane
// id, take one ticket each; those past `take` fail as the serial run's
// pushes onto a full ring / pops from an empty one do.  The end that stands
// still is read with a plain agent-scope load.
//
// ORDERED batches (`exact`: one lane) run the reference's sequence -- mixed
// operations, BPF_EXIST evictions -- reading both ends at the coherence point,
// where the lane's own earlier atomics were performed.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint64_t qs_coh64(uint64_t a) {
  return __hip_atomic_fetch_add(G64(a), 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void qs_set64(uint64_t a, uint64_t v) {
  __hip_atomic_exchange(G64(a), (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ bool qs_cas64(uint64_t a, unsigned long long *expect, uint64_t want) {
  return __hip_atomic_compare_exchange_strong(G64(a), expect, (unsigned long long)want, __ATOMIC_RELAXED,
                                              __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The slot `o` (< 64) tickets after the one whose slot index is `bm` (<
// max_entries, which is no power of two in general)
__device__ __forceinline__ uint64_t qs_slot_after(const DMap &m, uint32_t bm, uint32_t o) {
  uint64_t x = (uint64_t)bm + o;
  if (x >= m.max_entries) {
    x -= m.max_entries;
    if (x >= m.max_entries) x = (uint32_t)x % m.max_entries;  // (x < 64 here)
  }
  return m.data + m.val_off + x * m.slot_size;
}

// The calling lanes that name one ring (helper_qs groups them).  op: the
// helper id --
//   87 bpf_map_push_elem(map, value, flags)  queue.cpp:128-169, stack.cpp:119-157
//   88 bpf_map_pop_elem(map, value)          queue.cpp:171-194, stack.cpp:159-182
//   89 bpf_map_peek_elem(map, value)         queue.cpp:196-215, stack.cpp:184-204
//    1 lookup: a peek that returns the slot   queue.cpp:52-64,   stack.cpp:46-59
//    2 update: a push, flags not validated    queue.cpp:66-105,  stack.cpp:61-97
//    3 delete: a pop that discards (value 0)  queue.cpp:107-120, stack.cpp:99-111
__device__ uint64_t qs_group(const DMap m, uint64_t value, uint64_t flags, uint32_t op, bool exact) {
  const bool lifo = m.type == MT_STACK, push = op == 87 || op == 2, remove = op == 88 || op == 3;
  const uint64_t ha = qs_head_addr(m), ta = qs_tail_addr(m), cap = m.max_entries, fail = op == 1 ? 0 : (uint64_t)-1;
  // EINVAL: a NULL value; flags other than BPF_ANY (0) / BPF_EXIST (2) on a push
  const bool ok = (op == 1 || op == 3 || value != 0) && (op != 87 || flags == 0 || flags == 2);
  if (exact) {
    if (!ok) return fail;
    uint64_t h = qs_coh64(ha);
    const uint64_t t = qs_coh64(ta);
    if (push) {
      if (t - h >= cap) {
        if (flags != 2) return fail;  // E2BIG
        qs_set64(ha, ++h);            // the oldest element: the queue's head, the stack's bottom
      }
      copy_bytes_publish(qs_slot(m, t), value, m.value_size);
      qs_set64(ta, t + 1);
      return 0;
    }
    if (t == h) return fail;  // ENOENT
    const uint64_t s = qs_slot(m, lifo ? t - 1 : h);
    if (op == 1) return s;
    if (value) copy_bytes(value, s, m.value_size);
    if (remove) {
      if (lifo) qs_set64(ta, t - 1);
      else qs_set64(ha, h + 1);
    }
    return 0;
  }
  const uint64_t grp = __ballot(ok);
  if (!ok) return fail;
  const uint32_t me = __lane_id(), leader = (uint32_t)__builtin_ctzll(grp);
  const uint32_t n = (uint32_t)__builtin_popcountll(grp);
  const uint32_t rank = (uint32_t)__builtin_popcountll(grp & ((1ull << me) - 1));
  if (!push && !remove) {  // peek-only launch: nothing moves
    const uint64_t h = ald64(ha), t = ald64(ta);
    if (t == h) return fail;
    const uint64_t s = qs_slot(m, lifo ? t - 1 : h);
    if (op == 1) return s;
    copy_bytes(value, s, m.value_size);
    return 0;
  }
  // (a parallel push is a flags-0 push: the launch check admits no other)
  uint32_t take = 0, bm = 0;
  if (me == leader) {
    unsigned long long h = ald64(ha), t = ald64(ta);
    uint64_t base;
    if (push) {  // add-only launch: `head` stands still
      for (;;) {
        const uint64_t used = t - h;
        take = used >= cap ? 0 : (uint32_t)(cap - used < n ? cap - used : n);
        if (!take || qs_cas64(ta, &t, t + take)) break;
      }
      base = t;
    } else if (lifo) {  // remove-only launch, downward on `tail`
      for (;;) {
        take = (uint32_t)(t - h < n ? t - h : n);
        if (!take || qs_cas64(ta, &t, t - take)) break;
      }
      base = t - take;
    } else {  // remove-only launch, upward on `head`
      for (;;) {
        take = (uint32_t)(t - h < n ? t - h : n);
        if (!take || qs_cas64(ha, &h, h + take)) break;
      }
      base = h;
    }
    bm = (uint32_t)(base % cap);
  }
  take = __shfl(take, leader);
  bm = __shfl(bm, leader);
  if (rank >= take) return fail;  // E2BIG / ENOENT
  // tickets base .. base + take - 1: pushes and a queue's pops in rank
  // order, a stack's pops from the top down
  const uint64_t s = qs_slot_after(m, bm, push || !lifo ? rank : take - 1 - rank);
  if (push) copy_bytes_publish(s, value, m.value_size);
  else if (value) copy_bytes(value, s, m.value_size);
  return 0;
}

// The QUEUE / STACK helpers' one entry (interp.hip call_helper sends helpers
// 87 / 88 / 89 and 1 / 2 / 3 here when the map is a QUEUE / STACK; fd <
// kMaxFds): one group per distinct map among the calling lanes, as
// rb_reserve groups by ring.
__device__ __noinline__ uint64_t helper_qs(const DMap *maps, uint64_t fd, uint64_t value, uint64_t flags,
                                           uint32_t op, bool exact) {
  const uint64_t all = __ballot(1);
  uint64_t done = 0, out = 0;
  while (all & ~done) {
    const uint64_t f0 = __shfl(fd, (uint32_t)__builtin_ctzll(all & ~done));
    if (fd == f0) out = qs_group(maps[fd], value, flags, op, exact);
    done |= __ballot(fd == f0);
  }
  return out;
}

// ---------------------------------------------------------------------------
// bpf_probe_read / _user / _kernel (4 / 112 / 113), bpf_probe_read_str /
// _user_str / _kernel_str (45 / 114 / 115) and bpf_strncmp (182):
// bpf_helper.cpp:153-209, :431-437, :78-81.  Every byte these helpers touch
// is inside a range mem_guard.hpp accepted first; a rejected range answers
// -EFAULT with the destination untouched.  All loops are per lane: no lane
// waits on another.
// ---------------------------------------------------------------------------
constexpr uint64_t kEfault = (uint64_t)(int64_t)-14;

__device__ __forceinline__ uint8_t mem_ld8(uint64_t a) { return *(const volatile uint8_t *)a; }
__device__ __forceinline__ void mem_st8(uint64_t a, uint8_t v) { *(volatile uint8_t *)a = v; }

// Copy n bytes between flat addresses of any alignment (scratch stack, LDS
// ctx, packet, map arena).  Contract: where the ranges overlap (|d - s| < n)
// the bytes are copied one at a time in ascending order, so a destination
// that starts inside the source repeats the bytes in front of it.  Disjoint
// ranges move naturally aligned 8-byte words when d and s are congruent
// modulo 8, 4-byte words when congruent modulo 4 (byte head and tail), and
// otherwise aligned 4-byte word loads of the source with byte extraction
// (the pattern of key_eq).  No access leaves [s, s + n) or [d, d + n).
__device__ __forceinline__ void mem_copy(uint64_t d, uint64_t s, uint64_t n) {
  uint64_t i = 0;
  if (d - s < n || s - d < n) {
    for (; i < n; i++) mem_st8(d + i, mem_ld8(s + i));
    return;
  }
  const uint32_t x = (uint32_t)(d ^ s);
  if ((x & 7) == 0) {
    for (; i < n && ((s + i) & 7); i++) mem_st8(d + i, mem_ld8(s + i));
    for (; i + 8 <= n; i += 8) *(volatile uint64_t *)(d + i) = *(const volatile uint64_t *)(s + i);
  } else if ((x & 3) == 0) {
    for (; i < n && ((s + i) & 3); i++) mem_st8(d + i, mem_ld8(s + i));
    for (; i + 4 <= n; i += 4) *(volatile uint32_t *)(d + i) = *(const volatile uint32_t *)(s + i);
  } else {
    for (; i < n && ((s + i) & 3); i++) mem_st8(d + i, mem_ld8(s + i));
    for (; i + 4 <= n; i += 4) {
      const uint32_t w = *(const volatile uint32_t *)(s + i);
      mem_st8(d + i, (uint8_t)w);
      mem_st8(d + i + 1, (uint8_t)(w >> 8));
      mem_st8(d + i + 2, (uint8_t)(w >> 16));
      mem_st8(d + i + 3, (uint8_t)(w >> 24));
    }
  }
  for (; i < n; i++) mem_st8(d + i, mem_ld8(s + i));
}

__device__ __forceinline__ void mem_zero(uint64_t d, uint64_t n) {
  uint64_t i = 0;
  for (; i < n && ((d + i) & 7); i++) mem_st8(d + i, 0);
  for (; i + 8 <= n; i += 8) *(volatile uint64_t *)(d + i) = 0;
  for (; i < n; i++) mem_st8(d + i, 0);
}

// The one entry of the seven helpers (interp.hip call_helper; the id is
// wave-uniform, pointers and sizes are per lane).
//   probe_read*(dst, size, src): size < 0 -EFAULT, 0 -> 0, else a copy.
//   probe_read*_str(buf, bufsz, src): strncpy -- the source up to and with
//     its first NUL, or bufsz bytes when it has none, the rest of buf zeroed;
//     returns 0 (the reference's answer, not the kernel's length).  The
//     length is found first, bounded by the room of the region the source
//     starts in, so no byte after the NUL or past the region is read; then
//     the copy.
//   strncmp(s1, s1_sz, s2): 0, or the difference of the first differing
//     bytes as unsigned chars.
__device__ __noinline__ uint64_t helper_mem(uint32_t id, uint64_t a1, uint64_t a2, uint64_t a3, Win win,
                                            MemLane ml) {
  if (id == 182) {
    if (a2 == 0) return 0;
    const uint64_t r1 = mem_room(win, ml, a1), r2 = mem_room(win, ml, a3);
    uint64_t lim = r1 < r2 ? r1 : r2;
    if (lim == 0) return kEfault;
    if (lim > a2) lim = a2;
    for (uint64_t i = 0; i < lim; i++) {
      const uint8_t c1 = mem_ld8(a1 + i), c2 = mem_ld8(a3 + i);
      if (c1 != c2) return (uint64_t)(int64_t)((int32_t)c1 - (int32_t)c2);
      if (c1 == 0) return 0;
    }
    return lim < a2 ? kEfault : 0;  // a region ended before the strings did
  }
  if (id == 45 || id == 114 || id == 115) {
    if (a2 == 0) return 0;
    if (!mem_range_ok(win, ml, a1, a2)) return kEfault;
    const uint64_t room = mem_room(win, ml, a3);
    const uint64_t lim = room < a2 ? room : a2;
    uint64_t len = 0;
    while (len < lim && mem_ld8(a3 + len) != 0) len++;
    if (len == lim && lim < a2) return kEfault;  // (room 0 too: no byte accepted)
    mem_copy(a1, a3, len);
    mem_zero(a1 + len, a2 - len);
    return 0;
  }
  // bpf_probe_write_user(dst, src, len) (36, bpf_helper.cpp:239-299): the same
  // copy with the length last
  if (id == 36) {
    const uint64_t t = a2;
    a2 = a3;
    a3 = t;
  }
  // 4 / 112 / 113: one function, as in the reference
  if ((int64_t)a2 < 0) return kEfault;
  if (a2 == 0) return 0;
  if (!mem_range_ok(win, ml, a1, a2) || !mem_range_ok(win, ml, a3, a2)) return kEfault;
  mem_copy(a1, a3, a2);
  return 0;
}

// ---------------------------------------------------------------------------
// Task identity and bpf_trace_printk (15 / 16 / 6): bpf_helper.cpp:350-355,
// :364-385, :64-76.  The identity is the launching VM's and travels in the
// kernel arguments (KParams::task_*; per attached program in SeqParams).
// ---------------------------------------------------------------------------
struct TaskEnv {
  uint64_t uid_gid;
  uint64_t comm[8];    // NUL-terminated, zero to the end
  uint8_t *trace_log;  // the trace log (trace_fmt.hpp), or null
  uint64_t trace_cap;  // its records
  uint64_t unit;       // the calling unit's global index
  // the batch's recorded call stacks (common.hpp StackSrc; arr null: no stack
  // source) and the calling unit's index in the batch, which indexes them
  StackSrc stacks;
  uint64_t stack_unit;
  // bpf_get_stackid calls the unit has made so far (common.hpp st_claim_key).
  // Here and not in LaneEnv, which every instance of the kernels passes to
  // out-of-line helpers by address: a field more there grew the scratch frame
  // of two LDS-stack instances of k_interp
  uint32_t st_calls;
  // the running attachment's probed function and cookie (bpf_get_func_ip /
  // bpf_get_attach_cookie, bpf_helper.cpp:684-700): launch constants like the
  // identity (KParams::attach_*; the cookie per attached program in SeqParams)
  uint64_t func_ip;
  uint64_t cookie;
};

// bpf_get_current_comm(buf, size) = strncpy(buf, comm, size): comm up to and
// with its NUL, the rest of `size` zeroed; size <= strlen(comm) copies `size`
// bytes and adds no NUL.  The 64 bytes of `comm` are zero after the name, so
// that is: their first min(size, 64), then zeros.  Returns 0; -EFAULT, nothing
// written, when [buf, buf + size) is no range the guard accepts.
__device__ __noinline__ uint64_t helper_comm(uint64_t buf, uint64_t size, const TaskEnv &te, Win win, MemLane ml) {
  if (size == 0) return 0;
  if (!mem_range_ok(win, ml, buf, size)) return kEfault;
  const uint64_t lim = size < 64 ? size : 64;
#pragma unroll
  for (uint32_t j = 0; j < 8; j++) {
    uint64_t w = te.comm[j];
    for (uint32_t b = 0; b < 8 && 8 * j + b < lim; b++, w >>= 8) mem_st8(buf + 8 * j + b, (uint8_t)w);
  }
  if (size > 64) mem_zero(buf + 64, size - 64);
  return 0;
}

// bpf_trace_printk(fmt, fmt_size, a3, a4, a5): one record in the trace log,
// formatted by the host when it reads the log (bpftime_amd_trace_read).
// Returns 0 whether the record was stored or the log was full, as the
// reference always does; -EINVAL / -EFAULT (trace_fmt.hpp) log
// nothing.  Every byte read -- the format, a %s argument's string -- lies in a
// range mem_room gave; every loop is per lane and bounded by a cap.
// Reservation: the calling lanes of the wave are ranked by lane id, one lane
// adds the group's size to `tail` with one relaxed agent-scope fetch-and-add,
// lane of rank r takes ticket base + r; a ticket at or past the capacity
// counts into `lost` (one add per wave).  No lane waits on another.
__device__ __noinline__ uint64_t helper_trace(uint64_t fmt, uint64_t fmt_size, uint64_t a3, uint64_t a4, uint64_t a5,
                                              const TaskEnv &te, Win win, MemLane ml) {
  constexpr uint64_t kEinval = (uint64_t)(int64_t)kTraceEinval;
  const int fl = trace_fmt_len([&](uint32_t i) { return mem_ld8(fmt + i); }, fmt_size, mem_room(win, ml, fmt));
  if (fl < 0) return (uint64_t)(int64_t)fl;
  const uint32_t flen = (uint32_t)fl;
  TraceConv cv[kTraceMaxArgs];
  const int n = trace_scan([&](uint32_t i) { return mem_ld8(fmt + i); }, flen, cv);
  if (n < 0) return kEinval;
  if (!te.trace_log) return 0;
  // the %s arguments: state and length, bounded by the room of the region
  // the string starts in, the per-string cap and the precision
  const uint64_t args[3] = {a3, a4, a5};
  uint8_t kind[3] = {TK_NONE, TK_NONE, TK_NONE}, state[3] = {0, 0, 0}, slen[3] = {0, 0, 0};
#pragma unroll
  for (int a = 0; a < 3; a++) {
    if (a >= n) continue;
    kind[a] = cv[a].conv == 's' ? TK_STR : TK_INT;
    if (kind[a] != TK_STR) continue;
    const uint64_t s = args[a];
    if (s == 0) {
      state[a] = TS_NULL;
      continue;
    }
    const uint64_t sroom = mem_room(win, ml, s);
    if (sroom == 0) {
      state[a] = TS_EFAULT;
      continue;
    }
    const uint64_t lim = trace_str_lim(sroom, cv[a].prec);
    uint32_t l = 0;
    while (l < lim && mem_ld8(s + l) != 0) l++;
    slen[a] = (uint8_t)l;
  }
  // the wave's calling lanes, ranked by lane id
  const uint64_t active = __ballot(1);
  const uint32_t me = __lane_id();
  const uint32_t leader = (uint32_t)__builtin_ctzll(active);
  const uint32_t cnt = (uint32_t)__builtin_popcountll(active);
  const uint32_t rank = (uint32_t)__builtin_popcountll(active & ((1ull << me) - 1));
  uint64_t base = 0;
  if (me == leader) {
    base = __hip_atomic_fetch_add((uint64_t *)te.trace_log, (uint64_t)cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint64_t fit = base < te.trace_cap ? te.trace_cap - base : 0;
    if (fit < cnt)
      __hip_atomic_fetch_add((uint64_t *)(te.trace_log + 8), (uint64_t)cnt - fit, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
  }
  base = __shfl(base, leader);
  const uint64_t ticket = base + rank;
  if (ticket >= te.trace_cap) return 0;
  const uint64_t rec = (uint64_t)(uintptr_t)te.trace_log + kTraceHdrBytes + ticket * kTraceRecBytes;
  *(volatile uint64_t *)(rec + 0) = te.unit;
  *(volatile uint64_t *)(rec + 8) = a3;
  *(volatile uint64_t *)(rec + 16) = a4;
  *(volatile uint64_t *)(rec + 24) = a5;
  *(volatile uint64_t *)(rec + 32) = (uint64_t)flen | ((uint64_t)n << 8) | ((uint64_t)kind[0] << 16) |
                                     ((uint64_t)kind[1] << 24) | ((uint64_t)kind[2] << 32) |
                                     ((uint64_t)state[0] << 40) | ((uint64_t)state[1] << 48) |
                                     ((uint64_t)state[2] << 56);
  *(volatile uint64_t *)(rec + 40) = (uint64_t)slen[0] | ((uint64_t)slen[1] << 8) | ((uint64_t)slen[2] << 16);
  mem_copy(rec + 48, fmt, flen);
  mem_st8(rec + 48 + flen, 0);
#pragma unroll
  for (int a = 0; a < 3; a++)
    if (kind[a] == TK_STR && state[a] == TS_OK) {
      mem_copy(rec + 144 + 48 * a, args[a], slen[a]);
      mem_st8(rec + 144 + 48 * a + slen[a], 0);
    }
  return 0;
}

// ---------------------------------------------------------------------------
// ARRAY_OF_MAPS (map_in_maps.hpp): the helpers 1 / 2 / 3 of a program on an
// outer map (interp.hip call_helper sends them here; fd < kMaxFds, and the
// calling lanes may name different outer maps).
//    1 lookup: the slot's int as the inner map's "pointer", (void *)
//      ((u_int64_t)map_id) (map_in_maps.hpp:25-30): sign-extended, an empty slot
//      (0) is NULL.  The key is a u32 at a flat address of any alignment.  An
//      out-of-range key answers NULL here; the reference dereferences
//      array_map_impl::elem_lookup's nullptr (array_map.cpp:27-35).
//    2 update, 3 delete: -EINVAL, "Map in maps only support update from
//      syscall" (map_handler.cpp:365-369, :680-684); the slots stay as they are.
// The fd a lookup yields is checked where it is used: every map helper
// answers NULL / -1 for an fd >= kMaxFds (a negative slot is one) and for a
// descriptor of type 0 (never created, or closed), touching no memory.
// ---------------------------------------------------------------------------
__device__ __noinline__ uint64_t helper_mapinmap(const DMap *maps, uint64_t fd, uint64_t key, uint32_t op) {
  if (op != 1) return (uint64_t)(int64_t)-22;  // -EINVAL
  const DMap m = load_dmap(maps, fd);
  const uint32_t k = *(const u32u *)key;
  if (k >= m.max_entries) return 0;
  return (uint64_t)(int64_t) * (const volatile int32_t *)(m.data + 4ull * k);
}

// ---------------------------------------------------------------------------
// bpf_perf_event_output(ctx, map, flags, data, size) (25): bpf_helper.cpp:506-566
// over software_perf_event_buffer::output_data / append_record_parts
// (perf_event_handler.cpp:355-376, :306-353).  ctx and flags are not read (the
// reference reads neither, BPF_F_CURRENT_CPU included).  Per lane, in order:
//   the map must be a live PERF_EVENT_ARRAY and cpu < max_entries, else -1;
//   the slot of `cpu` must name a software perf event (common.hpp DPerf::soft;
//     an empty slot is -1, an fd >= kMaxFds), else -1;
//   size > kPerfMaxData (unsigned): -1 (E2BIG there);
//   [data, data + size) must be a range mem_guard.hpp accepts, else -EFAULT
//     (the reference copies unchecked; a size of 0 reads nothing);
//   record_size = (12 + size + 7) & ~7.  No ring yet, record_size > data_bytes,
//     or data_bytes - (head - tail) <= record_size (one byte stays free): the
//     record is dropped and the call answers 0, as output_data ignores
//     append_record_parts' result;
//   else the record -- u32 type 9 (PERF_RECORD_SAMPLE), u16 misc 0, u16
//     record_size, u32 record_size - 12, the data; the padding is not written
//     -- lies at head & (data_bytes - 1), wrapping at the ring's end, head moves
//     on by record_size, and the call answers 0.
// Many lanes, waves and blocks produce into one ring; its one consumer
// (bpftime_amd_perf_event_fetch) synchronizes the device first, so data_tail
// stands still while a launch runs and no record needs a BUSY mark.  The
// calling lanes are grouped by ring (each lane may name another map, slot or
// ring).  One lane of a group claims for all of it: it loads head, decides in
// lane order which records fit -- each against the room left once the taken
// ones before it lie there, which is what the lanes calling one after another
// would get -- and moves head past the taken ones with one agent-scope
// compare-and-swap.  A claim that takes nothing does not touch head, so the
// stream between tail and head always parses.  A lost swap means another wave
// moved head by at least 16 bytes, and head never passes tail + data_bytes -
// 1: the retries are bounded by the ring's size, and no lane waits for
// another.  An ORDERED batch's single lane runs the same claim.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t readlane32(uint32_t v, uint32_t lane) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)lane);
}
__device__ __forceinline__ uint64_t readlane64u(uint64_t v, uint32_t lane) {
  return (uint64_t)readlane32((uint32_t)v, lane) | ((uint64_t)readlane32((uint32_t)(v >> 32), lane) << 32);
}

__device__ __noinline__ uint64_t helper_perf_output(const DMap *maps, uint64_t map, uint64_t data, uint64_t size,
                                                    uint32_t cpu, Win win, MemLane ml) {
  constexpr uint64_t kFail = ~0ull;
  // the slot's fd (kMaxFds: none), then the fd's perf record with one
  // unconditional load, so that what the claim reads across lanes (ring,
  // data_bytes, rs) comes from straight-line selects
  uint32_t pfd = kMaxFds;
  if (map < kMaxFds) {
    const DMap m = maps[map];
    if (m.type == MT_PERF_EVENT_ARRAY && cpu < m.max_entries)
      pfd = (uint32_t) * (const volatile int32_t *)(m.data + 4ull * cpu);
  }
  const bool have = pfd < kMaxFds;
  const volatile DPerf *pt = (const volatile DPerf *)(maps + kMaxFds) + (have ? pfd : 0);
  const uint64_t pe_ring = pt->ring, pe_bytes = pt->data_bytes;
  const uint32_t pe_soft = pt->soft;
  const bool sized = have && pe_soft != 0 && size <= kPerfMaxData;
  const bool range = sized && (size == 0 || mem_range_ok(win, ml, data, size));
  const uint64_t ret = !sized ? kFail : !range ? kEfault : 0;
  const uint32_t rs = sized ? (uint32_t)((kPerfRecHdr + size + 7) & ~7ull) : 0;
  const bool want = range && pe_ring != 0 && pe_bytes != 0 && rs <= pe_bytes;
  const uint64_t ring = want ? pe_ring : 0, db = want ? pe_bytes : 0;
  const uint32_t me = __lane_id();
  uint64_t pending = __ballot(want);
  uint64_t off = 0;
  bool took = false;
  while (pending) {
    const uint32_t leader = (uint32_t)__builtin_ctzll(pending);
    const uint64_t ring0 = readlane64u(ring, leader), db0 = readlane64u(db, leader);
    const bool mine = want && ring == ring0;
    const uint64_t grp = __ballot(mine);
    pending &= ~grp;
    // tail: constant while the launch runs
    uint64_t head = 0, tail = 0;
    if (me == leader) {
      head = __hip_atomic_load(G64(ring0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      tail = __hip_atomic_load(G64(ring0 + kPerfTailOff), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    tail = readlane64u(tail, leader);
    const uint64_t bound = db0 / 16 + 2;
    uint32_t backoff = 1;
    for (uint64_t tries = 0; tries < bound; tries++) {
      const uint64_t h = readlane64u(head, leader);
      uint64_t cur = h, taken = 0, myoff = 0;
      // (head < tail or a ring as full as it gets: an invalid state drops, :325-330)
      const bool valid = h >= tail && h - tail < db0;
      for (uint64_t b = valid ? grp : 0; b; b &= b - 1) {
        const uint32_t l = (uint32_t)__builtin_ctzll(b);
        const uint64_t x = readlane32(rs, l);
        if (db0 - (cur - tail) > x) {
          taken |= 1ull << l;
          myoff = l == me ? cur : myoff;
          cur += x;
        }
      }
      if (!taken) break;  // nothing fits: head stays
      uint32_t won = 0;
      if (me == leader) {
        unsigned long long e = h;
        won = __hip_atomic_compare_exchange_strong(G64(ring0), &e, cur, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_AGENT)
                  ? 1
                  : 0;
        head = e;  // (lost: the head another wave set)
      }
      if (readlane32(won, leader)) {
        if (mine && ((taken >> me) & 1)) {
          took = true;
          off = myoff;
        }
        break;
      }
      // lost to another wave: back off (thousands of waves share this word)
      for (uint32_t i = 0; i < backoff; i++) __builtin_amdgcn_s_sleep(2);
      backoff = backoff < 64 ? 2 * backoff : 64;
    }
  }
  if (took) {
    const uint64_t mask = db - 1, base = ring + kPerfRingHdr;
    // (records are 8-aligned in a ring of a power of two >= 64: neither word splits)
    *(volatile uint64_t *)(base + (off & mask)) = 9ull | ((uint64_t)rs << 48);
    *(volatile uint32_t *)(base + ((off + 8) & mask)) = rs - kPerfRecHdr;
    const uint64_t at = (off + kPerfRecHdr) & mask;
    const uint64_t first = size <= db - at ? size : db - at;
    mem_copy(base + at, data, first);
    if (size > first) mem_copy(base, data + first, size - first);
  }
  return ret;
}

// ---------------------------------------------------------------------------
// bpf_get_stackid(ctx, map, flags) (27) and bpf_get_stack(ctx, buf, size,
// flags) (67): bpf_helper.cpp:791-893 over stack_trace_map.cpp:96-137.  The
// stack is the unit's recorded one (TaskEnv::stacks), where the reference asks
// the uprobe attach implementation for the caller's.  Checks, in its order:
//   BPF_F_USER_STACK clear: -ENOTSUP;  (67) BPF_F_USER_BUILD_ID set: -ENOTSUP;
//   no stack source (the attach implementation not registered): -ENOTSUP;
//   a unit with no frames (generate_stack returned nullptr): -ENOENT;
//   the first `flags & 0xff` frames are dropped; a stack that loses all of
//   them is empty, and is still hashed and stored.
// 27 then needs a STACK_TRACE map in r2: anything else answers -EINVAL (the
// reference dereferences the empty optional try_get_stack_trace_impl returns).
// id = hash % max_entries is the answer whatever happens to the slot.
// Every loop is per lane and bounded by kStMaxDepth; no lane waits on another.
// ---------------------------------------------------------------------------
constexpr uint64_t kStEnotsup = (uint64_t)(int64_t)-95, kStEnoent = (uint64_t)(int64_t)-2,
                   kStEinval = (uint64_t)(int64_t)-22;

// An ORDERED batch's lane applies fill_stack_trace on the spot: an empty slot
// takes the stack; an occupied one keeps its own unless the lengths differ,
// FAST_STACK_CMP is clear and REUSE_STACKID is set (the reference's "equal" is
// the lengths' equality).  A parallel batch: a slot that was full before the
// batch stays; for any other the call lowers the slot's claim word to its
// serial-order key with one relaxed agent-scope atomic min, and k_stack_commit
// stores the winner's frames after the batch (the launch refuses REUSE_STACKID).
__device__ __noinline__ uint64_t helper_stackid(const DMap *maps, uint64_t map, uint64_t flags, TaskEnv &te,
                                                bool exact) {
  const uint32_t seq = te.st_calls++;
  if (!(flags & kStUserStack) || !te.stacks.arr) return kStEnotsup;
  const uint32_t depth = st_depth(te.stacks, te.stack_unit);
  if (depth == 0) return kStEnoent;
  const uint32_t skip = (uint32_t)(flags & 0xff);
  const uint32_t n = depth > skip ? depth - skip : 0;
  uint64_t h = st_hash_combine(0, n);
  for (uint32_t k = 0; k < n; k++) h = st_hash_combine(h, st_frame(te.stacks, te.stack_unit, skip + k));
  if (map >= kMaxFds) return kStEinval;
  const DMap m = maps[map];
  if (m.type != MT_STACK_TRACE) return kStEinval;
  const uint64_t id = h % m.max_entries;
  const uint64_t slot = st_slot(m, id);
  if (!exact) {
    if (*(const volatile uint32_t *)(slot + 12) == 0)
      __hip_atomic_fetch_min((uint64_t *)slot, st_claim_key(te.unit, seq, skip), __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
    return (uint32_t)id;
  }
  const uint32_t have = *(const volatile uint32_t *)(slot + 8), full = *(const volatile uint32_t *)(slot + 12);
  if (full && ((flags & kStFastCmp) || have == n || !(flags & kStReuse))) return (uint32_t)id;
  // (n <= stack_max_depth <= value_size / 8: the launch check)
  const uint32_t cap = m.value_size / 8, nn = n < cap ? n : cap;
  for (uint32_t k = 0; k < cap; k++)
    *(volatile uint64_t *)(slot + kStHdr + 8ull * k) = k < nn ? st_frame(te.stacks, te.stack_unit, skip + k) : 0;
  *(volatile uint64_t *)(slot + 8) = (uint64_t)nn | 1ull << 32;
  return (uint32_t)id;
}

// 67: the reference copies min(frames after the skip, size) BYTES of the
// frames (it compares a frame count with a byte count) and answers 0.  The
// bytes written are a range the guard accepted first, else -EFAULT and nothing
// is written; no bytes to write (size 0, or every frame skipped): 0.
__device__ __noinline__ uint64_t helper_getstack(uint64_t buf, uint64_t size, uint64_t flags, const TaskEnv &te, Win win,
                                                 MemLane ml) {
  if (!(flags & kStUserStack) || (flags & kStBuildId) || !te.stacks.arr) return kStEnotsup;
  const uint32_t depth = st_depth(te.stacks, te.stack_unit);
  if (depth == 0) return kStEnoent;
  const uint32_t skip = (uint32_t)(flags & 0xff);
  const uint64_t n = depth > skip ? depth - skip : 0;
  const uint64_t bytes = n < size ? n : size;
  if (bytes == 0) return 0;
  if (!mem_range_ok(win, ml, buf, bytes)) return kEfault;
  for (uint32_t i = 0; i < (uint32_t)bytes; i++)
    mem_st8(buf + i, (uint8_t)(st_frame(te.stacks, te.stack_unit, skip + i / 8) >> (8 * (i % 8))));
  return 0;
}

// A program's helpers 1 / 2 / 3 on a STACK_TRACE map (stack_trace_map.cpp:36-94;
// ORDERED batches only, the launch refuses 1 / 3 elsewhere): lookup yields the
// slot's frames or NULL, update answers -ENOTSUP, delete empties the slot (0)
// or answers -1; a NULL key is NULL / -1.
__device__ __noinline__ uint64_t helper_stmap(const DMap *maps, uint64_t fd, uint64_t key, uint32_t op) {
  if (op == 2) return kStEnotsup;
  const uint64_t fail = op == 1 ? 0 : (uint64_t)-1;
  if (key == 0) return fail;
  const DMap m = maps[fd];
  const uint32_t k = *(const u32u *)key;
  if (k >= m.max_entries) return fail;
  const uint64_t slot = st_slot(m, k);
  if (*(const volatile uint32_t *)(slot + 12) == 0) return fail;
  if (op == 1) return slot + kStHdr;
  *(volatile uint64_t *)(slot + 8) = 0;
  return 0;
}

__device__ uint64_t helper_lookup(const DMap *maps, uint64_t fd, uint64_t key, LaneEnv &env) {
  if (fd >= kMaxFds) return 0;
  const DMap m = load_dmap(maps, fd);
  switch (m.type) {
    case MT_ARRAY: {
      uint32_t k = *(const u32u *)key;
      if (k >= m.max_entries) return 0;
      return m.data + (uint64_t)k * m.value_size;
    }
    case MT_PERCPU_ARRAY: {
      uint32_t k = *(const u32u *)key;
      if (k >= m.max_entries) return 0;
      return m.data + ((uint64_t)k * m.ncpu + env.vcpu % m.ncpu) * m.value_size;
    }
    case MT_HASH:
    case MT_PERCPU_HASH: {
      bool ins;
      uint64_t s = hash_find(m, key, false, 0, 0, &ins);
      if (!s) {
        env.miss_fd = (int32_t)fd;
        env.miss_hash = key_hash(key, m.key_size);
        return 0;
      }
      uint64_t v = s + m.val_off;
      if (m.type == MT_PERCPU_HASH) v += (env.vcpu % m.ncpu) * m.value_size;
      return v;
    }
    case MT_LPM_TRIE:
      return lpm_lookup(m, key);
    case MT_LRU_HASH: {
      const uint64_t v = lru_lookup(m, key, lru_next_stamp(env));
      if (!v) {
        env.miss_fd = (int32_t)fd;
        env.miss_hash = key_hash(key, m.key_size);
      }
      return v;
    }
    case MT_PROG_ARRAY: {  // prog_array.cpp:113-143: a copy of the slot's prog fd
      const int32_t k = (int32_t)*(const u32u *)key;
      if (k < 0 || (uint32_t)k >= m.max_entries) return 0;
      const int32_t v = *(const volatile int32_t *)(m.data + 4ull * (uint32_t)k);
      if (v < 0) return 0;
      // the copy: this lane's scratch word when the launch has them (the
      // reference's thread-local), else the array's shadow half (maps.cpp bpftime_maps_create);
      // either way a write through the pointer never reaches the array
      const uint64_t c = env.scratch ? env.scratch : m.data + 4ull * m.max_entries + 4ull * (uint32_t)k;
      *(volatile int32_t *)c = v;
      return c;
    }
  }
  return 0;
}

__device__ uint64_t helper_update(const DMap *maps, uint64_t fd, uint64_t key, uint64_t val,
                                  uint64_t flags, LaneEnv &env) {
  if (fd >= kMaxFds) return (uint64_t)-1;
  const DMap m = load_dmap(maps, fd);
  uint64_t base = flags & 0xffffffffull;
  bool flags_ok = base == 0 || base == 1 || base == 2;  // map_common_def.hpp:83-94
  switch (m.type) {
    case MT_ARRAY:
    case MT_PERCPU_ARRAY: {
      if (!flags_ok) return (uint64_t)-1;
      uint32_t k = *(const u32u *)key;
      if (k < m.max_entries && flags == 1) return (uint64_t)-1;  // EEXIST
      if (k >= m.max_entries) return (uint64_t)-1;               // E2BIG
      uint64_t dst = m.type == MT_ARRAY
                         ? m.data + (uint64_t)k * m.value_size
                         : m.data + ((uint64_t)k * m.ncpu + env.vcpu % m.ncpu) * m.value_size;
      copy_bytes(dst, val, m.value_size);
      return 0;
    }
    case MT_HASH: {
      // fix_hash_map.cpp:34-39: flags ignored, returns 0 even when full.
      bool ins;
      uint32_t vbytes = (m.value_size + 3) & ~3u;
      uint64_t s = hash_find(m, key, true, val, m.value_size, &ins);
      if (s && !ins) {
        // Existing element: overwrite, except in the lookup-miss race (this
        // lane's previous lookup of the same key missed, so in any serial
        // order this update would have created the element): another lane
        // created it first, and overwriting would drop its updates.
        bool race = env.miss_fd == (int32_t)fd && env.miss_hash == key_hash(key, m.key_size);
        if (!race) copy_bytes(s + m.val_off, val, m.value_size);
      }
      (void)vbytes;
      env.miss_fd = -1;
      return 0;
    }
    case MT_PERCPU_HASH: {
      if (!flags_ok) return (uint64_t)-1;
      // per_cpu_hash_map.cpp:66-94: insert zeroed ncpu*vsize, then write
      // the slot (a new element's slot before it is published)
      bool ins;
      const uint32_t off = (uint32_t)(env.vcpu % m.ncpu) * m.value_size;
      uint64_t s = hash_find(m, key, true, 0, m.value_size * m.ncpu, &ins, val, off, m.value_size);
      if (!s) return 0;
      bool race = !ins && env.miss_fd == (int32_t)fd && env.miss_hash == key_hash(key, m.key_size);
      if (!ins && !race) copy_bytes(s + m.val_off + off, val, m.value_size);
      env.miss_fd = -1;
      return 0;
    }
    case MT_LPM_TRIE:
      return env.exact ? lpm_update(m, key, val, flags) : (uint64_t)-1;
    case MT_LRU_HASH: {
      // the lookup-miss race of MT_HASH above: an existing element is not
      // overwritten by the lane whose lookup of the key just missed
      const bool race = env.miss_fd == (int32_t)fd && env.miss_hash == key_hash(key, m.key_size);
      env.miss_fd = -1;
      return lru_update(m, key, val, flags, lru_next_stamp(env), env.exact, race);
    }
  }
  return (uint64_t)-1;
}

__device__ uint64_t helper_delete(const DMap *maps, uint64_t fd, uint64_t key, LaneEnv &env) {
  if (fd >= kMaxFds) return (uint64_t)-1;
  const DMap m = load_dmap(maps, fd);
  switch (m.type) {
    case MT_ARRAY:
    case MT_PERCPU_ARRAY:
      return (uint64_t)-1;  // EINVAL (array_map.cpp:58-64)
    case MT_HASH: {
      bool ins;
      uint64_t s = hash_find(m, key, false, 0, 0, &ins);
      if (s) {
        uint32_t prev = ST_FILLED;  // no tombstone (bpftime_hash_map.hpp:182-199)
        if (__hip_atomic_compare_exchange_strong(G32(s), &prev, ST_EMPTY, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
          __hip_atomic_fetch_add(G64(m.count_addr), ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      return 0;
    }
    case MT_PERCPU_HASH: {
      // per_cpu_hash_map.cpp:96-107: zeroes [0, cpu*vsize) of the element
      bool ins;
      uint64_t s = hash_find(m, key, false, 0, 0, &ins);
      if (s) {
        uint64_t n = (env.vcpu % m.ncpu) * m.value_size;
        for (uint64_t i = 0; i < n; i++) *(volatile uint8_t *)(s + m.val_off + i) = 0;
      }
      return 0;
    }
    case MT_LRU_HASH:
      return lru_delete(m, key);
    case MT_LPM_TRIE:
      return env.exact ? lpm_remove(m, key) : (uint64_t)-1;
  }
  return (uint64_t)-1;
}

// bpf_helper.cpp:713-744
__device__ uint64_t helper_csum_diff(uint64_t from, uint64_t from_size_, uint64_t to,
                                     uint64_t to_size_, uint64_t seed_) {
  int from_size = (int)from_size_, to_size = (int)to_size_;
  int csum = -22;
  if ((from_size % 4 != 0) || (to_size % 4 != 0)) return (uint64_t)(int64_t)csum;
  csum = (int)seed_;
  if (to)
    for (int i = 0; i < to_size / 2; i++) csum += (uint16_t)(*(const u16u *)(to + 2 * i));
  if (from)
    for (int i = 0; i < from_size / 2; i++) csum += (uint16_t)(~*(const u16u *)(from + 2 * i));
  if (csum < 0) csum = -22;
  return (uint64_t)(int64_t)csum;
}

// xdp_md_userspace (runtime/extension/userspace_xdp.h:6-17)
struct XdpCtx {
  uint64_t data, data_end;
  uint32_t data_meta, ingress_ifindex, rx_queue_index, egress_ifindex;
  uint64_t buffer_start, buffer_end;
};

// bpf_helper.cpp:748-764
__device__ uint64_t helper_adjust_head(uint64_t ctx, uint64_t off_) {
  volatile XdpCtx *x = (volatile XdpCtx *)ctx;
  int offset = (int)off_;
  uint64_t data = x->data + (int64_t)offset;
  if (data > x->data_end - 14 || data > x->buffer_end) return (uint64_t)(int64_t)-22;
  if (data < x->buffer_start) {
    // memmove(buffer_start + (buffer_start - data), data, data_end - data)
    uint64_t dst = x->buffer_start + (x->buffer_start - data), src = x->data;
    uint64_t n = x->data_end - x->data;
    if (dst > src)
      for (uint64_t i = n; i-- > 0;) *(volatile uint8_t *)(dst + i) = *(volatile uint8_t *)(src + i);
    else
      for (uint64_t i = 0; i < n; i++) *(volatile uint8_t *)(dst + i) = *(volatile uint8_t *)(src + i);
    data = x->buffer_start;
  }
  x->data = data;
  return 0;
}

// bpf_helper.cpp:766-776
__device__ uint64_t helper_adjust_tail(uint64_t ctx, uint64_t delta_) {
  volatile XdpCtx *x = (volatile XdpCtx *)ctx;
  int delta = (int)delta_;
  uint64_t data = x->data_end + (int64_t)delta;
  if (data < x->data || data < x->buffer_start || data > x->buffer_end) return (uint64_t)(int64_t)-22;
  x->data_end = data;
  return 0;
}

// bpf_helper.cpp:778-788 (defined in the reference, not registered by default)
__device__ uint64_t helper_xdp_load_bytes(uint64_t ctx, uint64_t off, uint64_t buf, uint64_t len) {
  volatile XdpCtx *x = (volatile XdpCtx *)ctx;
  uint64_t data = x->data + (uint32_t)off;
  if (data + (uint32_t)len > x->data_end) return (uint64_t)(int64_t)-22;
  copy_bytes(buf, data, (uint32_t)len);
  return 0;
}

// ---------------------------------------------------------------------------
__device__ __forceinline__ uint64_t readlane64(uint64_t v, int lane) {
  const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)v, lane);
  const uint32_t hi = __builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
  return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t wave_sum64(uint64_t x) {
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return readlane64(x, 0);
}

// One lane of the wave adds a cached counter delta (wave-uniform arguments).
__device__ __forceinline__ void flush_delta(uint64_t a, uint32_t sz, uint64_t delta) {
  if (a == 0 || delta == 0) return;
  if ((threadIdx.x & 63) == 0) {
    if (sz == 8)
      __hip_atomic_fetch_add((uint64_t *)a, delta, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
      __hip_atomic_fetch_add((uint32_t *)a, (uint32_t)delta, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// one tagged delta {address | (4-byte ? 1 : 0), delta} (LDS combining
// table entries, the block's combined wave caches)
__device__ __forceinline__ void flush_delta_tag(uint64_t tag, uint64_t delta) {
  if (!tag || !delta) return;
  if (tag & 1)
    __hip_atomic_fetch_add((uint32_t *)(uintptr_t)(tag & ~1ull), (uint32_t)delta, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
  else
    __hip_atomic_fetch_add((uint64_t *)(uintptr_t)tag, delta, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace bpftime_amd
