// bpftime_amd: device side of bpftime_amd_map_dump (map_dump.cpp; semantics:
// include/bpftime_amd.h, DESIGN.md §6 "Map dump and drain").
//
// A stable compaction of a hash table's live buckets (state word 1) at or
// after a cursor, in bucket-index order -- the order a get_next_key walk
// yields -- into dense key and value arrays.  The plan and the discipline are
// xdp_complete.hip's.  Three launches on one stream:
//   k_md_count    a workgroup per tile of kMdTile consecutive buckets: how many
//                 of them are live (ballot popcounts per wave, summed over the
//                 block's waves in LDS);
//   k_md_scan     one workgroup: the tile counts become exclusive prefix sums
//                 over the tiles, kMdScanTiles tiles per pass with the running
//                 total carried; it writes the total, the returned count
//                 min(total, cap) and next = end;
//   k_md_scatter  a workgroup per tile again: a live bucket's rank is its
//                 ballot popcount below its lane, plus the counts of the waves
//                 and rounds of the tile before it (LDS), plus the tile's
//                 offset.  The tile's live buckets are listed in LDS in rank
//                 order; then groups of lanes copy one entry each, ranks below
//                 cap only, and the one bucket whose rank equals cap stores
//                 its index as next.  With erase, the group that copied an
//                 entry then stores state 0 to that bucket.
// Every rank is a function of the table alone, so the output is in bucket order
// whatever order the workgroups run in.  No workgroup waits on another: the
// only ordering between workgroups is the launch boundary.  Nothing here
// spins, polls a flag or looks back at another tile's state; the kernels use no
// atomics at all.
//
// Both bucket passes read the state words from the table (the count pass
// stores no flag per bucket).  An erase cannot disturb that: a bucket's state
// is read by exactly one lane of one workgroup of the scatter, before that
// workgroup's copy phase (a barrier apart), and the count pass is a launch
// earlier.  Reads stay inside nbuckets * slot_size bytes; writes stay inside
// min(total, cap) entries whatever the table holds.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "map_dump.hpp"

namespace bpftime_amd {

constexpr uint32_t kMdWaves = kMdBlock / 64, kMdRounds = kMdTile / kMdBlock;
static_assert(kMdTile <= 65536, "a tile's local bucket index is kept in 16 bits");

__device__ __forceinline__ bool md_live(const MdParams &p, uint64_t i) {
  return i < p.nbuckets && *(const uint32_t *)(p.table + i * p.slot_size) == 1;
}

__global__ __launch_bounds__(kMdBlock) void k_md_count(MdParams p) {
  __shared__ uint32_t wsum[kMdWaves];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t first = p.start + (uint64_t)blockIdx.x * kMdTile;
  uint32_t c = 0;  // (wave-uniform)
#pragma unroll
  for (uint32_t r = 0; r < kMdRounds; r++)
    c += (uint32_t)__popcll(__ballot(md_live(p, first + r * kMdBlock + threadIdx.x)));
  if (lane == 0) wsum[wave] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
#pragma unroll
    for (uint32_t w = 0; w < kMdWaves; w++) t += wsum[w];
    p.tile_counts[blockIdx.x] = t;
  }
}

// The tile counts become exclusive prefix sums, in place.  Thread t takes tile
// b + t of each pass (neighbouring lanes, neighbouring words); the pass is
// scanned by shuffles inside each wave and over the wave totals through LDS.
__global__ __launch_bounds__(kMdScanTiles) void k_md_scan(MdParams p) {
  __shared__ uint32_t wtot[kMdScanTiles / 64];
  const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
  uint32_t carry = 0;
  for (uint32_t b = 0; b < p.tiles; b += kMdScanTiles) {
    const uint32_t i = b + t;
    const uint32_t v = i < p.tiles ? p.tile_counts[i] : 0;
    uint32_t x = v;  // inclusive over the wave
#pragma unroll
    for (uint32_t o = 1; o < 64; o <<= 1) {
      const uint32_t y = __shfl_up(x, o);
      if (lane >= o) x += y;
    }
    if (lane == 63) wtot[wave] = x;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < kMdScanTiles / 64; w++) {
      const uint32_t q = wtot[w];
      before += w < wave ? q : 0;
      all += q;
    }
    if (i < p.tiles) p.tile_counts[i] = carry + before + x - v;
    carry += all;
    __syncthreads();
  }
  if (t == 0) {
    p.result[kMdTotal] = carry;
    p.result[kMdCount] = carry < p.cap ? carry : p.cap;
    p.result[kMdNext] = p.nbuckets;  // (the bucket of rank cap, if there is one, stores over it)
  }
}

// `n` lanes (l = 0 .. n-1) copy len bytes: in the widest unit of 16, 8 or 4
// bytes in which source and destination share their offset, bytes at the
// ragged ends; bytes throughout when they share none.  Consecutive lanes take
// consecutive units.  Reads [src, src + len) and writes [dst, dst + len), no
// more.
template <typename T>
__device__ __forceinline__ void md_copy_units(uint8_t *dst, const uint8_t *src, uint32_t len, uint32_t l,
                                              uint32_t n) {
  uint32_t head = (uint32_t)(-(uintptr_t)src & (sizeof(T) - 1));
  if (head > len) head = len;
  for (uint32_t q = l; q < head; q += n) dst[q] = src[q];
  const uint32_t body = (len - head) / (uint32_t)sizeof(T);
  const T *s = (const T *)(src + head);
  T *d = (T *)(dst + head);
  for (uint32_t q = l; q < body; q += n) d[q] = s[q];
  const uint32_t done = head + body * (uint32_t)sizeof(T);
  for (uint32_t q = done + l; q < len; q += n) dst[q] = src[q];
}

__device__ __forceinline__ void md_copy(uint8_t *dst, const uint8_t *src, uint32_t len, uint32_t l, uint32_t n) {
  const uint32_t x = (uint32_t)((uintptr_t)dst ^ (uintptr_t)src);
  if ((x & 15) == 0)
    md_copy_units<uint4>(dst, src, len, l, n);
  else if ((x & 7) == 0)
    md_copy_units<uint2>(dst, src, len, l, n);
  else if ((x & 3) == 0)
    md_copy_units<uint32_t>(dst, src, len, l, n);
  else
    for (uint32_t q = l; q < len; q += n) dst[q] = src[q];
}

__global__ __launch_bounds__(kMdBlock) void k_md_scatter(MdParams p) {
  // per round and wave, the live buckets: a bucket's place in the tile sums
  // the entries before its own (round, wave)
  __shared__ uint32_t wcnt[kMdRounds * kMdWaves];
  // the tile's live buckets (their index in the tile) in rank order
  __shared__ uint16_t list[kMdTile];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t first = p.start + (uint64_t)blockIdx.x * kMdTile;
  const uint64_t below = (1ull << lane) - 1;
  bool live[kMdRounds];
  uint32_t mine[kMdRounds];  // live buckets in lower lanes
#pragma unroll
  for (uint32_t r = 0; r < kMdRounds; r++) {
    live[r] = md_live(p, first + r * kMdBlock + threadIdx.x);
    const uint64_t m = __ballot(live[r]);
    if (lane == 0) wcnt[r * kMdWaves + wave] = (uint32_t)__popcll(m);
    mine[r] = (uint32_t)__popcll(m & below);
  }
  __syncthreads();
#pragma unroll
  for (uint32_t r = 0; r < kMdRounds; r++) {
    if (!live[r]) continue;
    uint32_t local = mine[r];
    for (uint32_t j = 0; j < r * kMdWaves + wave; j++) local += wcnt[j];
    list[local] = (uint16_t)(r * kMdBlock + threadIdx.x);
  }
  uint32_t found = 0;
#pragma unroll
  for (uint32_t j = 0; j < kMdRounds * kMdWaves; j++) found += wcnt[j];
  __syncthreads();
  // groups of p.group lanes, an entry each
  const uint32_t shift = (uint32_t)__builtin_ctz(p.group);
  const uint32_t l = threadIdx.x & (p.group - 1), g = threadIdx.x >> shift, groups = kMdBlock >> shift;
  const uint64_t off = p.tile_counts[blockIdx.x];
  for (uint32_t j = g; j < found; j += groups) {
    const uint64_t rank = off + j;
    if (rank > p.cap) break;
    const uint64_t b = first + list[j];
    if (rank == p.cap) {
      if (l == 0) p.result[kMdNext] = b;
      break;
    }
    uint8_t *slot = p.table + b * p.slot_size;
    if (p.keys) md_copy(p.keys + rank * p.key_size, slot + p.key_off, p.key_size, l, p.group);
    if (p.values) md_copy(p.values + rank * p.val_bytes, slot + p.val_off, p.val_bytes, l, p.group);
    if (p.erase && l == 0) *(uint32_t *)slot = 0;
  }
}

}  // namespace bpftime_amd

using namespace bpftime_amd;

extern "C" hipError_t bpftime_amd_launch_map_dump(const MdParams *p, hipStream_t stream) {
  if (!p || !p->table || !p->tiles || !p->tile_counts || !p->result || !p->cap || p->start >= p->nbuckets ||
      !p->group || (p->group & (p->group - 1)) || p->group > 64 ||
      (uint64_t)p->tiles * kMdTile < p->nbuckets - p->start)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_md_count, dim3(p->tiles), dim3(kMdBlock), 0, stream, *p);
  hipLaunchKernelGGL(k_md_scan, dim3(1), dim3(kMdScanTiles), 0, stream, *p);
  hipLaunchKernelGGL(k_md_scatter, dim3(p->tiles), dim3(kMdBlock), 0, stream, *p);
  return hipGetLastError();
}
