// The range guard of the copy / compare helpers (bpftime_amd/csrc/
// mem_guard.hpp mem_room / mem_range_ok) on the host: three global windows
// (two of them adjacent), a lane stack and a lane ctx copy.  No address is
// dereferenced.  Host-only: run by tests/test_mem_guard.py.
#include "../../bpftime_amd/csrc/mem_guard.hpp"

#include <stdio.h>

using namespace bpftime_amd;

static int bad = 0;
#define EXPECT(cond)                                         \
  do {                                                       \
    if (!(cond)) {                                           \
      printf("FAIL line %d: %s\n", __LINE__, #cond);         \
      bad++;                                                 \
    }                                                        \
  } while (0)

int main() {
  // batch [0x10000, 0x12000), arena [0x12000, 0x20000) right behind it,
  // scratch words [0x7f0000000000, +0x800); stack 512 B, ctx 48 B
  const Win w{0x10000, 0x12000, 0x12000, 0x20000, 0x7f0000000000ull, 0x7f0000000800ull, true};
  const MemLane l{0x500000, 0x600000, 512, 48};
  auto ok = [&](uint64_t a, uint64_t n) { return mem_range_ok(w, l, a, n); };
  const uint64_t lo[3] = {w.lo1, w.lo2, w.lo3}, hi[3] = {w.hi1, w.hi2, w.hi3};

  // NULL, and n = 0 anywhere
  EXPECT(!ok(0, 1));
  EXPECT(!ok(0, 8));
  EXPECT(mem_room(w, l, 0) == 0);
  EXPECT(!ok(w.lo1, 0));
  EXPECT(!ok(l.stack_lo, 0));
  EXPECT(!ok(0, 0));

  for (int k = 0; k < 3; k++) {
    const uint64_t size = hi[k] - lo[k];
    // the whole window, its first and last byte
    EXPECT(ok(lo[k], size));
    EXPECT(ok(lo[k], 1));
    EXPECT(ok(hi[k] - 1, 1));
    EXPECT(mem_room(w, l, lo[k]) == size);
    EXPECT(mem_room(w, l, hi[k] - 1) == 1);
    // one byte past the window's size, and a range straddling its end
    EXPECT(!ok(lo[k], size + 1));
    EXPECT(!ok(hi[k] - 4, 8));
    EXPECT(!ok(hi[k] - 1, 2));
  }
  // one byte before and one byte after each window (where no other window is)
  EXPECT(!ok(w.lo1 - 1, 1));
  EXPECT(!ok(w.lo1 - 1, 2));  // starts before, runs into the window
  EXPECT(ok(w.hi1, 1));       // (the arena's first byte)
  EXPECT(!ok(w.hi2, 1));
  EXPECT(!ok(w.lo3 - 1, 1));
  EXPECT(!ok(w.hi3, 1));
  // two adjacent windows: a range spanning both is rejected, each side alone is not
  EXPECT(w.hi1 == w.lo2);
  EXPECT(!ok(w.lo1, (w.hi1 - w.lo1) + 1));
  EXPECT(!ok(w.hi1 - 8, 16));
  EXPECT(ok(w.hi1 - 8, 8));
  EXPECT(ok(w.lo2, 8));
  EXPECT(!ok(w.lo1, w.hi2 - w.lo1));

  // wrap-around at 2^64 and huge lengths
  EXPECT(!ok(~0ull, 1));
  EXPECT(!ok(~0ull, 2));
  EXPECT(!ok(~0ull - 7, 16));
  EXPECT(!ok(w.lo1, ~0ull));
  EXPECT(!ok(w.lo1 + 8, 0 - (w.lo1 + 8)));           // a + n == 2^64
  EXPECT(!ok(0 - 0x100ull, 0x100 + w.lo1 + 16));      // a + n wraps into the batch window
  EXPECT(!ok(w.lo1, 1ull << 63));
  EXPECT(!ok(l.stack_lo, 1ull << 63));
  EXPECT(!ok(0, 1ull << 63));
  EXPECT(!ok(1ull << 63, 1ull << 63));

  // the lane's stack: inside, crossing its top, crossing its bottom
  EXPECT(ok(l.stack_lo, 512));
  EXPECT(ok(l.stack_lo + 504, 8));
  EXPECT(ok(l.stack_lo + 511, 1));
  EXPECT(!ok(l.stack_lo + 504, 16));  // fp - 8 for 16 bytes: over the top
  EXPECT(!ok(l.stack_lo + 512, 1));   // fp itself
  EXPECT(!ok(l.stack_lo, 513));
  EXPECT(!ok(l.stack_lo - 8, 16));    // under the bottom
  EXPECT(!ok(l.stack_lo - 1, 1));
  // ... and its ctx copy
  EXPECT(ok(l.ctx_lo, 48));
  EXPECT(ok(l.ctx_lo + 40, 8));
  EXPECT(!ok(l.ctx_lo + 40, 16));
  EXPECT(!ok(l.ctx_lo + 48, 1));
  EXPECT(!ok(l.ctx_lo - 1, 2));
  // no ctx copy (the ctx is the unit): size 0 accepts nothing
  {
    const MemLane nc{0x500000, 0, 512, 0};
    EXPECT(!mem_range_ok(w, nc, 0, 1));
    EXPECT(mem_range_ok(w, nc, w.lo1, 8));
  }
  // a ctx copy inside a global window (XDP ctxs kept in global memory): a
  // range may leave the lane's copy as far as the window goes
  {
    const MemLane gc{0x500000, w.lo3 + 48, 512, 48};
    EXPECT(mem_range_ok(w, gc, w.lo3 + 48, 96));
    EXPECT(!mem_range_ok(w, gc, w.lo3 + 48, w.hi3 - w.lo3));
  }

  // bounds checking off: any global range that does not wrap; the stack and
  // ctx rule stays
  {
    Win u = w;
    u.checked = false;
    auto uk = [&](uint64_t a, uint64_t n) { return mem_range_ok(u, l, a, n); };
    EXPECT(uk(0x30000, 1 << 20));
    EXPECT(uk(w.hi1 - 8, 16));
    EXPECT(uk(1, ~0ull));
    EXPECT(!uk(2, ~0ull));
    EXPECT(!uk(~0ull, 2));
    EXPECT(!uk(w.lo1, 0));
    EXPECT(uk(l.stack_lo + 504, 8));
    EXPECT(uk(l.ctx_lo, 48));
    // (on the host no address is in the LDS or scratch aperture, so a range
    // over the stack's top is an ordinary global range here; on the device
    // the stack is one, and mem_room keeps to the stack's extent: the first
    // term of mem_room, which this checks directly)
    EXPECT(mem_room_in(l.stack_lo + 504, l.stack_lo, l.stack_size) == 8);
    EXPECT(mem_room_in(l.stack_lo + 512, l.stack_lo, l.stack_size) == 0);
    EXPECT(mem_room_in(l.stack_lo - 1, l.stack_lo, l.stack_size) == 0);
  }
  // unset windows (k_sys_seq: the arena only)
  {
    const Win a{0, 0, 0x12000, 0x20000, 0, 0, true};
    EXPECT(!mem_range_ok(a, l, 0, 1));
    EXPECT(!mem_range_ok(a, l, 0x10000, 8));
    EXPECT(mem_range_ok(a, l, 0x12000, 8));
  }
  if (bad) {
    printf("%d failures\n", bad);
    return 1;
  }
  printf("OK\n");
  return 0;
}
