// bpftime_amd: bpftime_amd_xdp_complete (include/bpftime_amd.h, "XDP
// completion"): the argument checks, the per-stream scratch and the wait of a
// synchronous call.  The work is on the device (xdp_complete.hip).
//
// Every check runs before the first HIP call, so a refused call launches
// nothing and needs no device.  Scratch: one buffer per stream holding the
// sets' totals (32 B) and the tile counts (7 sets x ceil(count / tile) u32),
// allocated with hipMalloc when a call first needs more than the stream has
// and kept for the calls after it; a call on a stream that has its buffer
// allocates nothing and sets nothing to zero -- the kernels write every word
// they read.  count == 0 launches nothing and zeroes the caller's counters
// with one hipMemsetAsync each.
#include <errno.h>

#include <map>
#include <memory>
#include <mutex>
#include <string>

#include "../../include/bpftime_amd.h"
#include "../../include/ebpf-vm.h"
#include "runtime.hpp"
#include "xdp_complete.hpp"

using namespace bpftime_amd;

namespace {

// A stream's scratch and the lock a call holds from taking it until its last
// launch is queued (as the dispatches')
std::mutex g_buf_mu;
struct StreamBuf {
  void *p = nullptr;
  uint64_t bytes = 0;
  std::shared_ptr<std::mutex> mu = std::make_shared<std::mutex>();
};
std::map<hipStream_t, StreamBuf> g_bufs;

int fail(const std::string &what, int err = EINVAL) {
  set_error("xdp complete: " + what);
  errno = err;
  return -1;
}

bool aligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

constexpr uint64_t kTotalsBytes = 32;

// "" when the arguments are good, else what is wrong with them
std::string check(const struct bpftime_amd_xdp_complete_args *a) {
  if (!a) return "args is NULL";
  if (a->struct_size != sizeof(*a))
    return "struct_size " + std::to_string(a->struct_size) + ": this library knows " + std::to_string(sizeof(*a));
  if (a->flags & ~(uint32_t)BPFTIME_AMD_XDP_COMPLETE_SYNC) return "unknown flags " + std::to_string(a->flags);
  if (a->count >= (1ull << 32)) return "count " + std::to_string(a->count) + ": must be below 2^32";
  if (!a->verdicts) return "verdicts is NULL";
  if (a->stride == 0) return "stride is 0";
  if (!aligned(a->verdicts, 4)) return "verdicts: misaligned, a 4-aligned array";
  if (!aligned(a->descs, 8)) return "descs: misaligned, an 8-aligned array";
  if (!aligned(a->data_off_out, 4)) return "data_off_out: misaligned, a 4-aligned array";
  if (!aligned(a->len_out, 4)) return "len_out: misaligned, a 4-aligned array";
  if (!aligned(a->counts, 4)) return "counts: misaligned, a 4-aligned array";
  for (int c = 0; c < BPFTIME_AMD_XDP_CLASSES; c++) {
    if (!aligned(a->out[c], 8)) return "out[" + std::to_string(c) + "]: misaligned, an 8-aligned array";
    if (!aligned(a->index_out[c], 4)) return "index_out[" + std::to_string(c) + "]: misaligned, a 4-aligned array";
  }
  if (!aligned(a->gather_descs, 8)) return "gather_descs: misaligned, an 8-aligned array";
  if (!aligned(a->gather_index, 4)) return "gather_index: misaligned, a 4-aligned array";
  if (!aligned(a->gather_count, 4)) return "gather_count: misaligned, a 4-aligned word";
  if (!aligned(a->gather_skipped, 4)) return "gather_skipped: misaligned, a 4-aligned word";
  if (!a->descs) {
    if (!a->data_off_out || !a->len_out)
      return "strided mode (descs NULL) needs data_off_out and len_out: it has no other length";
    if (a->count && a->stride >= (1ull << 63) / a->count) return "strided mode: count * stride must be below 2^63";
  }
  if (a->frame_mask >> BPFTIME_AMD_XDP_CLASSES)
    return "frame_mask " + std::to_string(a->frame_mask) + ": bits past the five classes";
  if (a->gather_mask & ~a->frame_mask)
    return "gather_mask " + std::to_string(a->gather_mask) + " is outside frame_mask " + std::to_string(a->frame_mask);
  if (a->gather) {
    if (a->gather_stride == 0) return "gather without gather_stride";
    if (!a->umem) return "gather without umem, the base of the frames";
    if (a->gather_cap && a->gather_stride >= (1ull << 63) / a->gather_cap)
      return "gather_cap * gather_stride must be below 2^63";
  }
  if ((a->flags & BPFTIME_AMD_XDP_COMPLETE_SYNC) && !a->host_counts)
    return "BPFTIME_AMD_XDP_COMPLETE_SYNC without host_counts";
  return "";
}

int hip_fail(const char *what, hipError_t e) { return fail(std::string(what) + ": " + hipGetErrorString(e), EIO); }

}  // namespace

extern "C" uint32_t bpftime_amd_xdp_complete_tile(void) { return kXcTile; }
extern "C" uint32_t bpftime_amd_xdp_complete_scan_tiles(void) { return kXcScanTiles; }

extern "C" int bpftime_amd_xdp_complete_from_batch(const struct ebpf_batch *b,
                                                   struct bpftime_amd_xdp_complete_args *a) {
  if (!b || !a) return fail("from_batch: a NULL pointer");
  if (b->ctx_kind != EBPF_CTX_XDP)
    return fail("from_batch: ctx kind " + std::to_string(b->ctx_kind) + " is not EBPF_CTX_XDP");
  *a = bpftime_amd_xdp_complete_args{};
  a->struct_size = sizeof(*a);
  a->count = b->count;
  a->verdicts = b->verdicts;
  a->descs = b->descs;
  a->data_off_out = b->data_off_out;
  a->len_out = b->len_out;
  a->umem = b->data;
  a->stride = b->stride;
  // (a product past 2^64 saturates; the call then refuses it)
  a->umem_bytes = b->descs ? b->umem_bytes
                  : b->count && b->stride > UINT64_MAX / b->count ? UINT64_MAX
                                                                   : b->count * b->stride;
  a->stream = b->stream;
  a->frame_mask = BPFTIME_AMD_XDP_FRAME_MASK_DEFAULT;
  return 0;
}

extern "C" int bpftime_amd_xdp_complete(const struct bpftime_amd_xdp_complete_args *a) {
  const std::string bad = check(a);
  if (!bad.empty()) return fail(bad);
  const bool sync = (a->flags & BPFTIME_AMD_XDP_COMPLETE_SYNC) != 0;
  hipStream_t s = (hipStream_t)a->stream;
  hipError_t e = hipSuccess;

  if (a->count == 0) {
    if (a->counts) e = hipMemsetAsync(a->counts, 0, 4 * BPFTIME_AMD_XDP_CLASSES, s);
    if (e == hipSuccess && a->gather_count) e = hipMemsetAsync(a->gather_count, 0, 4, s);
    if (e == hipSuccess && a->gather_skipped) e = hipMemsetAsync(a->gather_skipped, 0, 4, s);
    if (e == hipSuccess && sync && (a->counts || a->gather_count || a->gather_skipped)) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail("zero counts", e);
    if (sync) {
      for (int c = 0; c < BPFTIME_AMD_XDP_CLASSES; c++) a->host_counts[c] = 0;
      if (a->host_gather) a->host_gather[0] = a->host_gather[1] = 0;
    }
    return 0;
  }

  XcParams p{};
  p.n = a->count;
  p.verdicts = a->verdicts;
  p.descs = (const uint64_t *)a->descs;
  p.off = a->data_off_out;
  p.len = a->len_out;
  p.umem = (const uint8_t *)a->umem;
  p.stride = a->stride;
  p.umem_bytes = a->umem_bytes;
  for (uint32_t c = 0; c < kXcClasses; c++) {
    p.out[c] = (uint64_t *)a->out[c];
    p.index_out[c] = a->index_out[c];
    p.cap[c] = a->cap[c];
  }
  p.frame_mask = a->frame_mask;
  p.gather_mask = a->gather ? a->gather_mask : 0;
  p.gather = (uint8_t *)a->gather;
  p.gather_stride = a->gather_stride;
  p.gather_cap = a->gather ? a->gather_cap : 0;
  p.gather_descs = (uint64_t *)a->gather_descs;
  p.gather_index = a->gather_index;
  p.tiles = (uint32_t)((a->count + kXcTile - 1) / kXcTile);
  p.counts = a->counts;
  p.gather_count = a->gather_count;
  p.gather_skipped = a->gather_skipped;

  std::shared_ptr<std::mutex> mu;
  {
    std::lock_guard<std::mutex> g(g_buf_mu);
    mu = g_bufs[s].mu;
  }
  uint32_t host_totals[8] = {0};
  {
    std::lock_guard<std::mutex> g(*mu);
    StreamBuf *sb;
    {
      std::lock_guard<std::mutex> gb(g_buf_mu);
      sb = &g_bufs[s];  // (std::map: the node stays where it is)
    }
    const uint64_t need = kTotalsBytes + 4ull * kXcSets * p.tiles;
    if (sb->bytes < need) {
      // (what is queued on the stream may still use the old buffer)
      if (sb->p && (e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail("scratch", e);
      if (sb->p && (e = hipFree(sb->p)) != hipSuccess) return hip_fail("scratch", e);
      sb->p = nullptr;
      sb->bytes = 0;
      if ((e = hipMalloc(&sb->p, need)) != hipSuccess) return fail("scratch allocation failed", ENOMEM);
      sb->bytes = need;
    }
    p.totals = (uint32_t *)sb->p;
    p.tile_counts = (uint32_t *)((uint8_t *)sb->p + kTotalsBytes);
    if ((e = bpftime_amd_launch_xdp_complete(&p, s)) != hipSuccess) return hip_fail("launch", e);
    if (sync) {
      // (inside the lock: the next call on this stream overwrites the totals)
      e = hipMemcpyAsync(host_totals, p.totals, sizeof(host_totals), hipMemcpyDeviceToHost, s);
      if (e == hipSuccess) e = hipStreamSynchronize(s);
      if (e != hipSuccess) return hip_fail("wait", e);
    }
  }
  if (sync) {
    for (uint32_t c = 0; c < kXcClasses; c++) a->host_counts[c] = host_totals[c];
    if (a->host_gather) {
      a->host_gather[0] = host_totals[kXcGather];
      a->host_gather[1] = host_totals[kXcSkipped];
    }
  }
  return 0;
}
