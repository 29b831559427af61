// bpftime_amd: what map_dump.cpp hands its kernels (map_dump.hip).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace bpftime_amd {

// A workgroup of kMdBlock lanes takes a tile of kMdTile consecutive buckets,
// kMdBlock at a time; the scan takes kMdScanTiles tiles per pass.
constexpr uint32_t kMdBlock = 256, kMdTile = 1024, kMdScanTiles = 256;
// the words of MdParams::result
constexpr uint32_t kMdTotal = 0, kMdCount = 1, kMdNext = 2, kMdResultWords = 4;

struct MdParams {
  uint8_t *table;             // nbuckets slots of slot_size bytes: {u32 state, key at key_off, value at val_off}
  uint64_t nbuckets;          // < 2^32
  uint32_t slot_size, key_off, val_off;
  uint32_t key_size, val_bytes;  // the user view: ncpu values of a per-CPU map
  uint64_t start;             // the first bucket looked at, < nbuckets; tile t starts at start + t * kMdTile
  uint64_t cap;               // entries keys / values have room for, > 0
  uint32_t erase;             // store state 0 to every bucket returned
  uint32_t group;             // lanes that copy one entry together: a power of two, 1..64
  uint8_t *keys;              // cap * key_size bytes, or null
  uint8_t *values;            // cap * val_bytes bytes, or null
  // scratch: tile_counts[tile], after k_md_scan the exclusive prefix sums over
  // the tiles; result {live buckets at or after start, entries returned, next cursor}
  uint32_t tiles;
  uint32_t *tile_counts;
  uint64_t *result;           // [kMdResultWords]
};

}  // namespace bpftime_amd

extern "C" {
// k_md_count, k_md_scan, k_md_scatter on `stream`, in that order
hipError_t bpftime_amd_launch_map_dump(const bpftime_amd::MdParams *p, hipStream_t stream);
}
