// bpftime_amd: device side of the uprobe replay dispatch (uprobe_dispatch.cpp).
//
// An attachment runs on the recorded calls of its function only.  They are
// gathered into compact 192-B rows {pt_regs, pid_tgid, clock, record index}
// in record order, so the interpreter runs an ordinary strided batch (no
// index indirection in k_interp) and every program works on a copy of its
// record, as the reference's callbacks do on their local pt_regs.
//
// Three launches: k_ug_count (matches per 64-record chunk: one ballot per
// wave, and one atomic add per wave for the total the host reads), k_ug_scan
// (the chunk counts to offsets; one block) and k_ug_gather.  The order of the
// rows is fixed by the offsets, not by the order the waves arrive in.
//
// Access shape of the gather: a wave owns a chunk whose m matches become m x
// 24 consecutive u64 of the output.  Lane l writes output words l, l + 64,
// ... of that range: neighbouring lanes write neighbouring 8-B words, 512
// contiguous bytes per wave store.  Word w belongs to row w / 24, field w %
// 24, so the same lanes read runs of up to 21 consecutive u64 of one source
// pt_regs (168 B, over two or three 64-B segments each); the three trailing
// words come from the pid, clock and index.  The alternative, a lane per
// record copying its 24 words, strides neighbouring lanes 168 B apart on the
// load side and 192 B on the store side: every wave access would touch 64
// different lines for 8 useful bytes each.
//
// The thread-ordered plan gathers nothing; its event-list form has two small
// passes here, k_ug_event_keys and k_ug_event_words (notes beside them).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "uprobe_dispatch.hpp"

namespace bpftime_amd {

constexpr uint32_t kUgBlock = 256;

// the position of the j-th (from 0) set bit of m; j < popcount(m)
__device__ __forceinline__ uint32_t nth_set(uint64_t m, uint32_t j) {
  uint32_t pos = 0;
#pragma unroll
  for (uint32_t s = 32; s; s >>= 1) {
    const uint32_t c = (uint32_t)__popcll(m & ((1ull << s) - 1));
    if (j >= c) {
      m >>= s;
      j -= c;
      pos += s;
    }
  }
  return pos;
}

__global__ __launch_bounds__(kUgBlock) void k_ug_count(UGather g) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = (blockIdx.x * kUgBlock + threadIdx.x) / 64, waves = gridDim.x * (kUgBlock / 64);
  uint32_t mine = 0;  // (wave-uniform)
  for (uint32_t c = wave; c < g.chunks; c += waves) {
    const uint64_t i = (uint64_t)c * 64 + lane;
    const bool hit = i < g.n && g.func[i] == g.target;
    const uint32_t m = (uint32_t)__popcll(__ballot(hit));
    if (lane == 0) g.counts[c] = m;
    mine += m;
  }
  if (lane == 0 && mine) atomicAdd(g.total, mine);
}

// counts[0 .. chunks) -> exclusive prefix sums, in place.  One block walks the
// array in tiles of 1024: thread t takes entry tile + t (neighbouring lanes,
// neighbouring words), the tile is scanned in LDS and the running total
// carried to the next tile.  Measured (profiles/uprobe_dispatch_measurement.txt):
// count + scan take 0.31 ms per attachment at 65536 chunks, 0.29 ms with a
// contiguous run per thread instead of tiles: the one-block scan, not its
// access shape, sets that time.  A scan over several blocks is the next step.
__global__ __launch_bounds__(1024) void k_ug_scan(uint32_t *counts, uint32_t chunks) {
  __shared__ uint32_t sums[1024];
  const uint32_t t = threadIdx.x;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < chunks; base += 1024) {
    const uint32_t i = base + t;
    const uint32_t v = i < chunks ? counts[i] : 0;
    sums[t] = v;
    __syncthreads();
    for (uint32_t o = 1; o < 1024; o <<= 1) {
      const uint32_t x = t >= o ? sums[t - o] : 0;
      __syncthreads();
      sums[t] += x;
      __syncthreads();
    }
    if (i < chunks) counts[i] = carry + sums[t] - v;
    carry += sums[1023];
    __syncthreads();
  }
}

__global__ __launch_bounds__(kUgBlock) void k_ug_gather(UGather g) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = (blockIdx.x * kUgBlock + threadIdx.x) / 64, waves = gridDim.x * (kUgBlock / 64);
  for (uint32_t c = wave; c < g.chunks; c += waves) {
    const uint64_t first = (uint64_t)c * 64;
    const bool hit = first + lane < g.n && g.func[first + lane] == g.target;
    const uint64_t mask = __ballot(hit);
    uint64_t base = g.counts[c];
    // (never past the rows the host sized, whatever func holds by now)
    if (base >= g.cap) continue;
    uint32_t m = (uint32_t)__popcll(mask);
    if (base + m > g.cap) m = (uint32_t)(g.cap - base);
    for (uint32_t w = lane; w < m * kRowWords; w += 64) {
      const uint32_t j = w / kRowWords, k = w % kRowWords;
      const uint64_t rec = first + nth_set(mask, j);
      uint64_t v;
      if (k < kRegsWords)
        v = g.regs[rec * kRegsWords + k];
      else if (k == kRegsWords)
        v = g.pid ? g.pid[rec] : g.pid_default;
      else if (k == kRegsWords + 1)
        v = g.clock ? g.clock[rec * 2 + g.phase] : 0;
      else
        v = rec;
      g.rows[base * kRowWords + w] = v;
    }
    if (!g.stack_rows) continue;
    const uint32_t D = g.stack_max_depth;
    auto depth_of = [&](uint64_t rec) {
      const uint32_t d = g.stack_depths ? g.stack_depths[rec] : g.stack_fixed_depth;
      return d < D ? d : D;
    };
    for (uint32_t w = lane; w < m * D; w += 64) {
      const uint32_t j = w / D, k = w % D;
      const uint64_t rec = first + nth_set(mask, j);
      g.stack_rows[base * D + w] =
          k < depth_of(rec) ? *(const uint64_t *)(g.stack_arr + rec * g.stack_unit_stride + k * g.stack_frame_stride)
                            : 0;
    }
    if (lane < m) g.stack_depths_out[base + lane] = depth_of(first + nth_set(mask, lane));
  }
}

__global__ void k_ug_scatter(const uint64_t *rows, uint64_t m, uint64_t n, const uint32_t *state, const int64_t *vals,
                             int replace, uint32_t *out_state, int64_t *out_rets) {
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t rec = rows[j * kRowWords + kRowIndexWord];
    if (rec >= n || !(replace || (state[j] & 1))) continue;
    out_state[rec] |= 1u;  // (a record has one row: the function's only attachment)
    out_rets[rec] = vals[j];
  }
}

// The event list's key pass (bpftime_amd_uprobe_dispatch_events): lane e reads
// events[e] (4 B per lane, contiguous) and writes the thread of its record,
// keys[e] = pid[events[e] >> 1] (8 B per lane, contiguous; the pid load is the
// one gather).  An event whose record is not below nrec gets key 0, is never
// dereferenced and is counted: one ballot per wave, one atomic add per wave
// that saw any.  Null keys: the range check alone (one thread walks the list).
__global__ __launch_bounds__(kUgBlock) void k_ug_event_keys(const uint32_t *events, uint64_t n, const uint64_t *pid,
                                                            uint64_t nrec, uint64_t *keys, uint32_t *bad) {
  const uint32_t lane = threadIdx.x & 63;
  uint32_t mine = 0;  // (wave-uniform)
  // (whole waves take the loop together: the bound is rounded up to 64)
  const uint64_t n64 = (n + 63) & ~63ull;
  for (uint64_t e = (uint64_t)blockIdx.x * kUgBlock + threadIdx.x; e < n64; e += (uint64_t)gridDim.x * kUgBlock) {
    const bool in = e < n;
    const uint64_t rec = in ? events[e] >> 1 : 0;
    const bool out = in && rec >= nrec;
    if (in && keys) keys[e] = out ? 0 : pid[rec];
    mine += (uint32_t)__popcll(__ballot(out));
  }
  if (lane == 0 && mine) atomicAdd(bad, mine);
}

// After the grouping: perm[k], an index into the event list, becomes the event
// word itself, so each step of the walk has one dependent load fewer
__global__ __launch_bounds__(kUgBlock) void k_ug_event_words(uint32_t *perm, const uint32_t *events, uint64_t n) {
  for (uint64_t k = (uint64_t)blockIdx.x * kUgBlock + threadIdx.x; k < n; k += (uint64_t)gridDim.x * kUgBlock) {
    const uint32_t e = perm[k];
    if (e < n) perm[k] = events[e];
  }
}

static uint32_t wave_grid(uint32_t chunks) {
  const uint32_t blocks = (chunks + kUgBlock / 64 - 1) / (kUgBlock / 64);
  return blocks > 4096 ? 4096 : blocks ? blocks : 1;
}

}  // namespace bpftime_amd

using namespace bpftime_amd;

extern "C" hipError_t bpftime_amd_launch_ug_count(const UGather *g, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(g->total, 0, 4, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_ug_count, dim3(wave_grid(g->chunks)), dim3(kUgBlock), 0, stream, *g);
  hipLaunchKernelGGL(k_ug_scan, dim3(1), dim3(1024), 0, stream, g->counts, g->chunks);
  return hipGetLastError();
}

extern "C" hipError_t bpftime_amd_launch_ug_gather(const UGather *g, hipStream_t stream) {
  hipLaunchKernelGGL(k_ug_gather, dim3(wave_grid(g->chunks)), dim3(kUgBlock), 0, stream, *g);
  return hipGetLastError();
}

static uint32_t lane_grid(uint64_t n) {
  const uint64_t blocks = (n + kUgBlock - 1) / kUgBlock;
  return blocks > 4096 ? 4096 : blocks ? (uint32_t)blocks : 1;
}

extern "C" hipError_t bpftime_amd_launch_ug_event_keys(const uint32_t *events, uint64_t n, const uint64_t *pid,
                                                       uint64_t nrec, uint64_t *keys, uint32_t *bad,
                                                       hipStream_t stream) {
  if (!events || !n || !bad || (keys && !pid)) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(bad, 0, 4, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_ug_event_keys, dim3(lane_grid(n)), dim3(kUgBlock), 0, stream, events, n, pid, nrec, keys, bad);
  return hipGetLastError();
}

extern "C" hipError_t bpftime_amd_launch_ug_event_words(uint32_t *perm, const uint32_t *events, uint64_t n,
                                                        hipStream_t stream) {
  if (!perm || !events || !n) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_ug_event_words, dim3(lane_grid(n)), dim3(kUgBlock), 0, stream, perm, events, n);
  return hipGetLastError();
}

extern "C" hipError_t bpftime_amd_launch_ug_scatter(const uint64_t *rows, uint64_t m, uint64_t n,
                                                    const uint32_t *state, const int64_t *vals, int replace,
                                                    uint32_t *out_state, int64_t *out_rets, hipStream_t stream) {
  if (!m) return hipSuccess;
  uint64_t blocks = (m + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(k_ug_scatter, dim3((uint32_t)blocks), dim3(256), 0, stream, rows, m, n, state, vals, replace,
                     out_state, out_rets);
  return hipGetLastError();
}
