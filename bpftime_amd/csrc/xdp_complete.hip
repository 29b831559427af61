// bpftime_amd: device side of bpftime_amd_xdp_complete (xdp_complete.cpp;
// semantics: include/bpftime_amd.h, DESIGN.md §6 "XDP completion").
//
// A stable multi-way partition of a finished XDP batch's units by verdict
// class, plus one more set -- the merged gather list -- ranked the same way,
// and the copy of the gathered frames.  Three launches on the caller's stream:
//   k_xc_count    a workgroup per tile of kXcTile units: how many units of the
//                 tile fall into each set (ballot popcounts per wave, summed
//                 over the block's waves in LDS);
//   k_xc_scan     a workgroup per set: the tile counts become exclusive prefix
//                 sums over the tiles, kXcScanTiles tiles per pass with the
//                 running total carried, and the set's total is written out;
//   k_xc_scatter  a workgroup per tile again: a unit's rank in its set is its
//                 ballot popcount below its lane, plus the counts of the
//                 waves and rounds of the tile before it (LDS), plus the
//                 tile's offset.  Every rank is a function of the inputs alone,
//                 so the lists are in unit order whatever order the workgroups
//                 run in.  Then the tile's gathered frames are copied, a wave
//                 per frame.
// No workgroup waits on another: the only ordering between workgroups is the
// launch boundary.  Nothing here spins, polls a flag or looks back at another
// tile's state; the kernels use no atomics at all.
//
// Both unit passes classify from the inputs (the count pass stores no class
// byte): the scatter needs the descriptor anyway, and writes are bounded by
// the caller's caps whatever the inputs hold by then.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "xdp_complete.hpp"

namespace bpftime_amd {

constexpr uint32_t kXcWaves = kXcBlock / 64, kXcRounds = kXcTile / kXcBlock;
constexpr uint32_t kXcRanked = kXcGather + 1;  // the sets whose members get a rank

struct XcUnit {
  uint32_t cls;       // 0..4
  bool gather;        // a member of the merged gather list
  bool skipped;       // left out of it for len > gather_stride
  uint64_t e_addr;    // its list entry {addr, len, options}
  uint32_t e_len, e_opt;
  uint64_t f_addr;    // a gather member's frame: umem offset and length
  uint32_t f_len;
};

// Unit i by the rules of include/bpftime_amd.h.  No sum here can wrap: the
// frame is placed relative to its chunk base (rel < stride) and every bound is
// tested by subtraction from a value known to be the larger.
__device__ __forceinline__ XcUnit xc_classify(const XcParams &p, uint64_t i, bool pow2) {
  XcUnit u;
  uint64_t addr;
  uint32_t dlen = 0, opt = 0;
  if (p.descs) {
    addr = p.descs[2 * i];
    const uint64_t w = p.descs[2 * i + 1];
    dlen = (uint32_t)w;
    opt = (uint32_t)(w >> 32);
  } else {
    addr = i * p.stride;  // (count * stride < 2^63: xdp_complete.cpp)
  }
  const int64_t off = p.off ? (int64_t)p.off[i] : 0;
  const uint32_t len = p.len ? p.len[i] : dlen;
  const uint32_t v = p.verdicts[i];
  const uint64_t rel = pow2 ? addr & (p.stride - 1) : addr % p.stride, base = addr - rel;
  const bool chunk_in = base <= p.umem_bytes && p.stride <= p.umem_bytes - base;
  bool frame_in = false;
  uint64_t srel = 0;  // the frame's start inside the chunk
  if (off < 0) {
    const uint64_t back = (uint64_t)(-off);
    if (rel >= back) {
      srel = rel - back;
      frame_in = true;
    }
  } else if ((uint64_t)off <= p.stride - rel) {
    srel = rel + (uint64_t)off;
    frame_in = true;
  }
  frame_in = frame_in && len <= p.stride - srel;
  const bool confined = !(chunk_in && frame_in);
  u.cls = confined || v >= kXcClasses ? 0 : v;
  if (!confined && ((p.frame_mask >> u.cls) & 1)) {
    u.e_addr = base + srel;
    u.e_len = len;
    u.e_opt = opt;
  } else {
    u.e_addr = chunk_in ? base : addr;
    u.e_len = 0;
    u.e_opt = 0;
  }
  const bool wanted = p.gather && !confined && ((p.gather_mask >> u.cls) & 1);
  u.gather = wanted && len <= p.gather_stride;
  u.skipped = wanted && !u.gather;
  u.f_addr = base + srel;
  u.f_len = len;
  return u;
}

__global__ __launch_bounds__(kXcBlock) void k_xc_count(XcParams p) {
  __shared__ uint32_t wsum[kXcWaves][kXcSets];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t first = (uint64_t)blockIdx.x * kXcTile;
  const bool pow2 = (p.stride & (p.stride - 1)) == 0;
  uint32_t c[kXcSets];  // (wave-uniform)
#pragma unroll
  for (uint32_t s = 0; s < kXcSets; s++) c[s] = 0;
#pragma unroll
  for (uint32_t r = 0; r < kXcRounds; r++) {
    const uint64_t i = first + r * kXcBlock + threadIdx.x;
    const bool in = i < p.n;
    XcUnit u{};
    if (in) u = xc_classify(p, i, pow2);
#pragma unroll
    for (uint32_t s = 0; s < kXcClasses; s++) c[s] += (uint32_t)__popcll(__ballot(in && u.cls == s));
    c[kXcGather] += (uint32_t)__popcll(__ballot(in && u.gather));
    c[kXcSkipped] += (uint32_t)__popcll(__ballot(in && u.skipped));
  }
  if (lane == 0) {
#pragma unroll
    for (uint32_t s = 0; s < kXcSets; s++) wsum[wave][s] = c[s];
  }
  __syncthreads();
  if (threadIdx.x < kXcSets) {
    uint32_t t = 0;
#pragma unroll
    for (uint32_t w = 0; w < kXcWaves; w++) t += wsum[w][threadIdx.x];
    p.tile_counts[(uint64_t)threadIdx.x * p.tiles + blockIdx.x] = t;
  }
}

// Workgroup s turns set s's tile counts into exclusive prefix sums, in place,
// and writes the set's total.  Thread t takes tile b + t of each pass
// (neighbouring lanes, neighbouring words); the pass is scanned by shuffles
// inside each wave and over the 16 wave totals through LDS.
__global__ __launch_bounds__(kXcScanTiles) void k_xc_scan(XcParams p) {
  __shared__ uint32_t wtot[kXcScanTiles / 64];
  const uint32_t s = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  uint32_t *col = p.tile_counts + (uint64_t)s * p.tiles;
  uint32_t carry = 0;
  for (uint32_t b = 0; b < p.tiles; b += kXcScanTiles) {
    const uint32_t i = b + t;
    const uint32_t v = i < p.tiles ? col[i] : 0;
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
    for (uint32_t w = 0; w < kXcScanTiles / 64; w++) {
      const uint32_t q = wtot[w];
      before += w < wave ? q : 0;
      all += q;
    }
    if (i < p.tiles) col[i] = carry + before + x - v;
    carry += all;
    __syncthreads();
  }
  if (t == 0) {
    p.totals[s] = carry;
    if (s < kXcClasses) {
      if (p.counts) p.counts[s] = carry;
    } else if (s == kXcGather) {
      if (p.gather_count) *p.gather_count = carry;
    } else if (p.gather_skipped) {
      *p.gather_skipped = carry;
    }
  }
}

// One wave copies one frame: 16 B per lane where source and destination share
// their offset in a 16-B line, bytes at the ragged ends; bytes throughout when
// they do not.  Reads [src, src + len) and writes [dst, dst + len), no more.
__device__ __forceinline__ void xc_copy(uint8_t *dst, const uint8_t *src, uint32_t len, uint32_t lane) {
  if ((((uintptr_t)dst ^ (uintptr_t)src) & 15) == 0) {
    uint32_t head = (uint32_t)(-(uintptr_t)src & 15);
    if (head > len) head = len;
    if (lane < head) dst[lane] = src[lane];
    const uint32_t body = (len - head) >> 4;
    const uint4 *s4 = (const uint4 *)(src + head);
    uint4 *d4 = (uint4 *)(dst + head);
    for (uint32_t q = lane; q < body; q += 64) d4[q] = s4[q];
    const uint32_t done = head + (body << 4), tail = len - done;  // tail < 16
    if (lane < tail) dst[done + lane] = src[done + lane];
  } else {
    for (uint32_t q = lane; q < len; q += 64) dst[q] = src[q];
  }
}

__global__ __launch_bounds__(kXcBlock) void k_xc_scatter(XcParams p) {
  // per round and wave, the members of each ranked set: a unit's rank sums
  // the entries before its own (round, wave)
  __shared__ uint32_t wcnt[kXcRounds * kXcWaves][kXcRanked];
  __shared__ uint32_t tile_off[kXcRanked];
  // the lists by class, read with a lane's class as the index
  __shared__ uint64_t *s_out[kXcClasses];
  __shared__ uint32_t *s_index[kXcClasses];
  __shared__ uint64_t s_cap[kXcClasses];
  // the tile's gathered frames in list order
  __shared__ uint64_t g_src[kXcTile];
  __shared__ uint32_t g_len[kXcTile];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t first = (uint64_t)blockIdx.x * kXcTile;
  const bool pow2 = (p.stride & (p.stride - 1)) == 0;
  if (threadIdx.x < kXcRanked) tile_off[threadIdx.x] = p.tile_counts[(uint64_t)threadIdx.x * p.tiles + blockIdx.x];
  if (threadIdx.x == 0) {
#pragma unroll
    for (uint32_t s = 0; s < kXcClasses; s++) {
      s_out[s] = p.out[s];
      s_index[s] = p.index_out[s];
      s_cap[s] = p.cap[s];
    }
  }
  const uint64_t below = (1ull << lane) - 1;
#pragma unroll 1
  for (uint32_t r = 0; r < kXcRounds; r++) {
    const uint64_t i = first + r * kXcBlock + threadIdx.x;
    const bool in = i < p.n;
    XcUnit u{};
    if (in) u = xc_classify(p, i, pow2);
    uint32_t mine = 0;  // members of my class in lower lanes
#pragma unroll
    for (uint32_t s = 0; s < kXcClasses; s++) {
      const uint64_t m = __ballot(in && u.cls == s);
      if (lane == 0) wcnt[r * kXcWaves + wave][s] = (uint32_t)__popcll(m);
      if (u.cls == s) mine = (uint32_t)__popcll(m & below);
    }
    const uint64_t mg = __ballot(in && u.gather);
    if (lane == 0) wcnt[r * kXcWaves + wave][kXcGather] = (uint32_t)__popcll(mg);
    __syncthreads();  // (also orders the setup stores above before the first reads)
    if (in) {
      uint32_t k = tile_off[u.cls] + mine;
      for (uint32_t j = 0; j < r * kXcWaves + wave; j++) k += wcnt[j][u.cls];
      if (k < s_cap[u.cls]) {
        uint64_t *o = s_out[u.cls];
        uint32_t *ix = s_index[u.cls];
        if (o) {
          o[2 * (uint64_t)k] = u.e_addr;
          o[2 * (uint64_t)k + 1] = (uint64_t)u.e_len | ((uint64_t)u.e_opt << 32);
        }
        if (ix) ix[k] = (uint32_t)i;
      }
      if (u.gather) {
        uint32_t local = (uint32_t)__popcll(mg & below);  // its place among the tile's frames
        for (uint32_t j = 0; j < r * kXcWaves + wave; j++) local += wcnt[j][kXcGather];
        g_src[local] = u.f_addr;
        g_len[local] = u.f_len;
        const uint64_t kg = (uint64_t)tile_off[kXcGather] + local;
        if (kg < p.gather_cap) {
          if (p.gather_descs) {
            p.gather_descs[2 * kg] = kg * p.gather_stride;
            p.gather_descs[2 * kg + 1] = (uint64_t)u.f_len | ((uint64_t)u.e_opt << 32);
          }
          if (p.gather_index) p.gather_index[kg] = (uint32_t)i;
        }
      }
    }
  }
  if (!p.gather) return;  // (uniform)
  __syncthreads();
  uint32_t frames = 0;
#pragma unroll
  for (uint32_t j = 0; j < kXcRounds * kXcWaves; j++) frames += wcnt[j][kXcGather];
  const uint64_t kg0 = tile_off[kXcGather];
  for (uint32_t j = wave; j < frames && kg0 + j < p.gather_cap; j += kXcWaves)
    xc_copy(p.gather + (kg0 + j) * p.gather_stride, p.umem + g_src[j], g_len[j], lane);
}

}  // namespace bpftime_amd

using namespace bpftime_amd;

extern "C" hipError_t bpftime_amd_launch_xdp_complete(const XcParams *p, hipStream_t stream) {
  if (!p || !p->n || !p->tiles || !p->tile_counts || !p->totals) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_xc_count, dim3(p->tiles), dim3(kXcBlock), 0, stream, *p);
  hipLaunchKernelGGL(k_xc_scan, dim3(kXcSets), dim3(kXcScanTiles), 0, stream, *p);
  hipLaunchKernelGGL(k_xc_scatter, dim3(p->tiles), dim3(kXcBlock), 0, stream, *p);
  return hipGetLastError();
}
