// bpftime_amd: what xdp_complete.cpp hands its kernels (xdp_complete.hip).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace bpftime_amd {

// The partition's sets: the five verdict classes, the merged gather list, and
// the units the gather leaves out for their length (counted, never ranked).
constexpr uint32_t kXcClasses = 5, kXcGather = 5, kXcSkipped = 6, kXcSets = 7;
// A workgroup of kXcBlock lanes takes a tile of kXcTile consecutive units,
// kXcBlock at a time; the scan takes kXcScanTiles tiles per pass.
constexpr uint32_t kXcBlock = 256, kXcTile = 1024, kXcScanTiles = 1024;

struct XcParams {
  uint64_t n;                // < 2^32
  const uint32_t *verdicts;
  const uint64_t *descs;     // {u64 addr, u32 len, u32 options} per unit, or null: strided
  const int32_t *off;        // or null: 0
  const uint32_t *len;       // or null: the descriptor's
  const uint8_t *umem;
  uint64_t stride, umem_bytes;
  uint64_t *out[kXcClasses];  // entries as two u64 {addr, len | options << 32}
  uint32_t *index_out[kXcClasses];
  uint64_t cap[kXcClasses];
  uint32_t frame_mask, gather_mask;
  uint8_t *gather;            // null: no gather set
  uint64_t gather_stride, gather_cap;
  uint64_t *gather_descs;
  uint32_t *gather_index;
  // scratch: tile_counts[set * tiles + tile], after k_xc_scan the exclusive
  // prefix sums over the tiles; totals[set]
  uint32_t tiles;
  uint32_t *tile_counts;
  uint32_t *totals;           // [8]
  uint32_t *counts;           // the caller's u32[5], gather_count, gather_skipped (each nullable)
  uint32_t *gather_count;
  uint32_t *gather_skipped;
};

}  // namespace bpftime_amd

extern "C" {
// k_xc_count, k_xc_scan, k_xc_scatter on `stream`, in that order
hipError_t bpftime_amd_launch_xdp_complete(const bpftime_amd::XcParams *p, hipStream_t stream);
}
