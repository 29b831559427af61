// bpftime_amd: bpf_trace_printk's format scanner, the record a call leaves in
// the device log, and the host formatter that turns a record into the line
// snprintf would print (dev_helpers.hpp helper_trace, vm_abi.cpp
// bpftime_amd_trace_read).  The scanner is plain C++ over a byte getter, so
// the device helper (bytes the range guard admitted) and the host formatter
// (the record's copy) run the same code (tests/cpp/trace_fmt_test.cpp).
#pragma once
#include <stdint.h>

#include "mem_guard.hpp"  // BA_HD

#if !defined(__HIP_DEVICE_COMPILE__)
#include <stdio.h>
#include <string.h>
#endif

namespace bpftime_amd {

// The caps (Trace and task helpers)
constexpr uint32_t kTraceFmtMax = 96;    // format bytes, the NUL included
constexpr uint32_t kTraceStrMax = 47;    // captured bytes of a %s argument (+ a NUL)
constexpr uint32_t kTraceMaxArgs = 3;    // conversions that consume an argument
constexpr uint32_t kTraceMaxField = 64;  // width and precision
constexpr uint32_t kTraceDefaultRecords = 65536;  // BPFTIME_AMD_TRACE_RECORDS

constexpr int kTraceEinval = -22;

// The log: a header line, then `cap` records.
//   +0  u64 tail   tickets handed out (may pass the capacity: those are lost)
//   +8  u64 lost   records that found the log full
constexpr uint32_t kTraceHdrBytes = 64;

// Argument states a record keeps for a %s conversion
constexpr uint8_t TS_OK = 0, TS_NULL = 1, TS_EFAULT = 2;
// Argument kinds
constexpr uint8_t TK_NONE = 0, TK_INT = 1, TK_STR = 2;

// One call.  8 + 24 + 16 + 96 + 3 x 48 = 288 bytes of content; records are
// 320 bytes apart so each starts on a 64-byte line.
struct TraceRec {
  uint64_t unit;      // global unit index (first_unit + i; a replay's record index)
  uint64_t args[3];   // r3..r5 as passed
  uint8_t fmt_len;    // format bytes, without the NUL (< kTraceFmtMax)
  uint8_t nargs;      // conversions that consume an argument
  uint8_t kind[3];    // TK_*
  uint8_t state[3];   // TS_* (TK_STR)
  uint8_t slen[3];    // captured bytes (TK_STR, TS_OK)
  uint8_t pad[5];
  uint8_t fmt[kTraceFmtMax];
  uint8_t str[3][kTraceStrMax + 1];
  uint8_t pad2[32];
};
static_assert(sizeof(TraceRec) == 320, "device and host agree on the record");
constexpr uint32_t kTraceRecBytes = 320;

// One conversion of a validated format
constexpr uint8_t TF_MINUS = 1, TF_PLUS = 2, TF_SPACE = 4, TF_HASH = 8, TF_ZERO = 16;
constexpr uint8_t TL_NONE = 0, TL_HH = 1, TL_H = 2, TL_L = 3, TL_LL = 4;
struct TraceConv {
  uint8_t start, end;  // [start, end) in the format: '%' .. the conversion character
  uint8_t flags;       // TF_*
  uint8_t width;       // 0..kTraceMaxField
  int8_t has_width;
  int8_t prec;         // -1: none
  uint8_t len;         // TL_*
  char conv;           // d i u x X o c p s
};

// Scans the `len` bytes get(0..len-1) (no NUL among them).  Accepted: literal
// bytes, %%, %[-+ #0]*[width][.precision][hh|h|l|ll] with one of d i u x X o
// c p, and %[-][width][.precision]s; at most kTraceMaxArgs conversions, width
// and precision at most kTraceMaxField.  Returns the number of conversions
// (cv[0..]) or kTraceEinval: '*', %n, floating conversions, a fourth
// argument, a trailing '%', an unknown conversion character, a width or
// precision above the cap.  Reads no byte at or past `len`.
template <class Get>
BA_HD int trace_scan(Get get, uint32_t len, TraceConv *cv) {
  auto at = [&](uint32_t i) -> uint8_t { return i < len ? (uint8_t)get(i) : (uint8_t)0; };
  uint32_t i = 0;
  int n = 0;
  while (i < len) {
    if (at(i) != '%') {
      i++;
      continue;
    }
    TraceConv c{};
    c.start = (uint8_t)i;
    i++;
    if (i >= len) return kTraceEinval;  // a trailing '%'
    if (at(i) == '%') {
      i++;
      continue;
    }
    for (;; i++) {
      const uint8_t f = at(i);
      if (f == '-') c.flags |= TF_MINUS;
      else if (f == '+') c.flags |= TF_PLUS;
      else if (f == ' ') c.flags |= TF_SPACE;
      else if (f == '#') c.flags |= TF_HASH;
      else if (f == '0') c.flags |= TF_ZERO;
      else break;
    }
    uint32_t w = 0;
    for (; at(i) >= '0' && at(i) <= '9'; i++) {
      w = w * 10 + (at(i) - '0');
      c.has_width = 1;
      if (w > kTraceMaxField) return kTraceEinval;
    }
    c.width = (uint8_t)w;
    c.prec = -1;
    if (at(i) == '.') {
      i++;
      uint32_t p = 0;
      for (; at(i) >= '0' && at(i) <= '9'; i++) {
        p = p * 10 + (at(i) - '0');
        if (p > kTraceMaxField) return kTraceEinval;
      }
      c.prec = (int8_t)p;
    }
    if (at(i) == 'h') {
      i++;
      c.len = TL_H;
      if (at(i) == 'h') {
        i++;
        c.len = TL_HH;
      }
    } else if (at(i) == 'l') {
      i++;
      c.len = TL_L;
      if (at(i) == 'l') {
        i++;
        c.len = TL_LL;
      }
    }
    const uint8_t k = at(i);  // (0 past the end: no conversion character)
    i++;
    switch (k) {
      case 'd': case 'i': case 'u': case 'x': case 'X': case 'o': case 'c': case 'p':
        break;
      case 's':
        if ((c.flags & ~TF_MINUS) || c.len != TL_NONE) return kTraceEinval;
        break;
      default:
        return kTraceEinval;
    }
    c.conv = (char)k;
    c.end = (uint8_t)i;
    if (n == (int)kTraceMaxArgs) return kTraceEinval;
    cv[n++] = c;
  }
  return n;
}

// The format string of a call: the bytes get(0..) up to the first NUL within
// the first `fmt_size` bytes, `room` being the bytes the range guard admits
// from its start (mem_room).  Its length, or kTraceEinval (fmt_size 0, no NUL
// in that span, longer than kTraceFmtMax with the NUL) or kTraceEfault (no
// room, or the region ends before fmt_size and the string do).  Reads no byte
// at or past min(fmt_size, room, kTraceFmtMax).
constexpr int kTraceEfault = -14;
template <class Get>
BA_HD int trace_fmt_len(Get get, uint64_t fmt_size, uint64_t room) {
  if (fmt_size == 0) return kTraceEinval;
  if (room == 0) return kTraceEfault;
  const uint64_t span = fmt_size < kTraceFmtMax ? fmt_size : kTraceFmtMax;
  for (uint32_t n = 0;; n++) {
    if (n >= span) return kTraceEinval;
    if (n >= room) return kTraceEfault;
    if (get(n) == 0) return (int)n;
  }
}

// Bytes of a %s argument that may be read: the room of the region it starts
// in, the per-string cap, the conversion's precision (-1: none)
BA_HD uint64_t trace_str_lim(uint64_t room, int prec) {
  uint64_t lim = room < kTraceStrMax ? room : kTraceStrMax;
  if (prec >= 0 && lim > (uint64_t)prec) lim = (uint64_t)prec;
  return lim;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The line of one record: exactly what snprintf gives for the record's format
// and arguments, each conversion re-emitted from the scanned spec with the
// C type its length modifier names -- hh / h / none take the low 8 / 16 / 32
// bits, l / ll all 64, %c the low byte, %p the raw word (both without a
// length modifier).  A %s prints the captured bytes; a NULL pointer goes to
// snprintf as NULL ("(null)", as glibc prints it), a pointer outside every
// region prints the string "(efault)".  Nothing in the record is trusted: the
// format is scanned again, lengths are clamped, no pointer a program passed
// is dereferenced.  Returns the line's length (a %c of 0 puts a NUL inside
// it); `out` holds min(length, cap - 1) bytes and a NUL.  A record whose
// format no longer scans (its source changed under the device's copy) gives
// "(bad format)".
inline int trace_format(const TraceRec &r, char *out, size_t cap) {
  if (cap == 0) return -1;
  const uint32_t flen = r.fmt_len < kTraceFmtMax ? r.fmt_len : kTraceFmtMax - 1;
  uint32_t n0 = 0;
  while (n0 < flen && r.fmt[n0]) n0++;
  TraceConv cv[kTraceMaxArgs];
  const int n = trace_scan([&](uint32_t i) { return r.fmt[i]; }, n0, cv);
  size_t o = 0;
  auto put = [&](const char *p, size_t k) {
    for (size_t j = 0; j < k; j++, o++)
      if (o + 1 < cap) out[o] = p[j];
  };
  if (n < 0) {
    put("(bad format)", 12);
    out[o < cap ? o : cap - 1] = 0;
    return (int)o;
  }
  uint32_t pos = 0;
  auto literal = [&](uint32_t to) {  // the bytes up to `to`, %% as %
    while (pos < to) {
      const char c = (char)r.fmt[pos];
      put(&c, 1);
      pos += (c == '%') ? 2 : 1;
    }
  };
  for (int a = 0; a < n; a++) {
    const TraceConv &c = cv[a];
    literal(c.start);
    pos = c.end;
    char spec[32];
    size_t s = 0;
    spec[s++] = '%';
    if (c.flags & TF_MINUS) spec[s++] = '-';
    if (c.flags & TF_PLUS) spec[s++] = '+';
    if (c.flags & TF_SPACE) spec[s++] = ' ';
    if (c.flags & TF_HASH) spec[s++] = '#';
    if (c.flags & TF_ZERO) spec[s++] = '0';
    if (c.has_width) s += (size_t)snprintf(spec + s, 8, "%u", (unsigned)c.width);
    if (c.prec >= 0) s += (size_t)snprintf(spec + s, 8, ".%u", (unsigned)c.prec);
    const bool integer = c.conv != 'c' && c.conv != 'p' && c.conv != 's';
    const bool wide = integer && (c.len == TL_L || c.len == TL_LL);
    if (integer && c.len == TL_HH) spec[s++] = 'h', spec[s++] = 'h';
    if (integer && c.len == TL_H) spec[s++] = 'h';
    if (wide) spec[s++] = 'l', spec[s++] = 'l';
    spec[s++] = c.conv;
    spec[s] = 0;
    char piece[192];  // (width and precision <= 64, a 64-bit value in octal 22 digits)
    const uint64_t v = r.args[a];
    int k;
#pragma GCC diagnostic push
#pragma GCC diagnostic ignored "-Wformat-nonliteral"
#pragma GCC diagnostic ignored "-Wformat-security"
    if (c.conv == 's') {
      char sbuf[kTraceStrMax + 1];
      const char *sp = "(efault)";
      if (r.kind[a] == TK_STR && r.state[a] == TS_NULL) {
        sp = nullptr;
      } else if (r.kind[a] == TK_STR && r.state[a] == TS_OK) {
        uint32_t l = r.slen[a] <= kTraceStrMax ? r.slen[a] : kTraceStrMax, j = 0;
        for (; j < l && r.str[a][j]; j++) sbuf[j] = (char)r.str[a][j];
        sbuf[j] = 0;
        sp = sbuf;
      }
      k = snprintf(piece, sizeof(piece), spec, sp);
    } else if (c.conv == 'p') {
      k = snprintf(piece, sizeof(piece), spec, (void *)(uintptr_t)v);
    } else if (c.conv == 'c') {
      k = snprintf(piece, sizeof(piece), spec, (int)(uint8_t)v);
    } else if (wide) {
      k = snprintf(piece, sizeof(piece), spec, (unsigned long long)v);
    } else if (c.conv == 'd' || c.conv == 'i') {
      k = snprintf(piece, sizeof(piece), spec, (int)(uint32_t)v);
    } else {
      k = snprintf(piece, sizeof(piece), spec, (unsigned)(uint32_t)v);
    }
#pragma GCC diagnostic pop
    if (k > 0) put(piece, (size_t)k < sizeof(piece) ? (size_t)k : sizeof(piece) - 1);
  }
  literal(n0);
  out[o < cap ? o : cap - 1] = 0;
  return (int)o;
}
#endif

}  // namespace bpftime_amd
