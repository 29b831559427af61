// bpftime_amd: the memory windows of a launch and the range guard of the
// helpers that copy or compare byte ranges of run-time length
// (bpf_probe_read*, bpf_probe_read_*_str, bpf_strncmp: dev_helpers.hpp
// helper_mem).  Plain C++ apart from the address-space builtins, so the guard
// also compiles for the host (tests/cpp/mem_guard_test.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BA_DEV __device__ __forceinline__
#define BA_HD __host__ __device__ inline
#define BA_HDF __host__ __device__ __forceinline__
#else
#define BA_DEV inline
#define BA_HD inline
#define BA_HDF inline
#endif

namespace bpftime_amd {

BA_HDF bool is_lds_addr(uint64_t a) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_is_shared((const void *)a);
#else
  return false;
#endif
}
BA_HDF bool is_scratch_addr(uint64_t a) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_is_private((const void *)a);
#else
  return false;
#endif
}

// Global windows a program may access: the batch, the map arena, and the
// lanes' scratch words (PROG_ARRAY lookup copies; C++ tier only -- the asm
// window check leaves those accesses to it).
struct Win {
  uint64_t lo1, hi1, lo2, hi2, lo3, hi3;
  bool checked;
  BA_DEV bool ok(uint64_t a, uint32_t sz) const {
    if (!checked) return true;
    if (is_lds_addr(a) || is_scratch_addr(a)) return true;
    uint64_t e = a + sz;
    return (a >= lo1 && e <= hi1 && e >= a) || (a >= lo2 && e <= hi2 && e >= a) ||
           (a >= lo3 && e <= hi3 && e >= a);
  }
};

// The calling lane's own memory, as flat addresses: its stack and its ctx
// copy (size 0: the ctx is the unit itself, inside the batch window).
struct MemLane {
  uint64_t stack_lo, ctx_lo;
  uint32_t stack_size, ctx_size;
};

// Win::ok admits any LDS or scratch address of any size: harmless for a 1-
// to 8-byte access, not for a length a program chooses.  mem_room(a) is the
// number of bytes from `a` to the end of the region that holds it -- the
// lane's stack, the lane's ctx copy, or one of the three global windows (the
// largest, where regions nest) -- and 0 when none does: NULL, an address
// between windows, another lane's LDS or scratch.  A range is accepted when
// it starts in a region and ends inside the same one, so it never wraps and
// never spans two adjacent windows.  With bounds checking off (!checked) the
// global windows are not looked at -- every address outside the LDS and
// scratch apertures has room to the top of the address space -- and the
// stack and ctx rule stays.
BA_HD uint64_t mem_room_in(uint64_t a, uint64_t lo, uint64_t size) {
  const uint64_t o = a - lo;
  return o < size ? size - o : 0;
}

BA_HD uint64_t mem_room(const Win &w, const MemLane &l, uint64_t a) {
  uint64_t r = mem_room_in(a, l.stack_lo, l.stack_size);
  auto more = [&](uint64_t x) { r = x > r ? x : r; };
  more(mem_room_in(a, l.ctx_lo, l.ctx_size));
  if (!w.checked) {
    if (!is_lds_addr(a) && !is_scratch_addr(a)) more(0 - a);
    return r;
  }
  // (hi < lo, an unset window: size 0)
  more(mem_room_in(a, w.lo1, w.hi1 > w.lo1 ? w.hi1 - w.lo1 : 0));
  more(mem_room_in(a, w.lo2, w.hi2 > w.lo2 ? w.hi2 - w.lo2 : 0));
  more(mem_room_in(a, w.lo3, w.hi3 > w.lo3 ? w.hi3 - w.lo3 : 0));
  return r;
}

// [a, a + n), n >= 1
BA_HD bool mem_range_ok(const Win &w, const MemLane &l, uint64_t a, uint64_t n) {
  return n >= 1 && n <= mem_room(w, l, a);
}

}  // namespace bpftime_amd
