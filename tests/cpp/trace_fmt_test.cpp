// bpf_trace_printk's shared scanner and the host line formatter
// (bpftime_amd/csrc/trace_fmt.hpp) on the host.  capture() does what the
// device helper does (dev_helpers.hpp helper_trace) with the same shared
// functions over a window of host memory; the formatter's lines are compared
// with snprintf's.  Host-only: run by tests/test_trace_fmt.py.
#include "../../bpftime_amd/csrc/trace_fmt.hpp"

#include <limits.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

using namespace bpftime_amd;

static int bad = 0;
#define EXPECT(cond)                                         \
  do {                                                       \
    if (!(cond)) {                                           \
      printf("FAIL line %d: %s\n", __LINE__, #cond);         \
      bad++;                                                 \
    }                                                        \
  } while (0)

// one window of host memory: what a program may touch
static uint8_t g_mem[4096];
static Win g_win;
static const MemLane g_lane{0, 0, 0, 0};
static uint64_t A(size_t off) { return (uint64_t)(uintptr_t)(g_mem + off); }

// the device helper's steps; returns 0 (rec filled), -EINVAL or -EFAULT
static int capture(uint64_t fmt, uint64_t fmt_size, uint64_t a3, uint64_t a4, uint64_t a5, TraceRec &rec) {
  auto ld = [](uint64_t a) { return *(const uint8_t *)(uintptr_t)a; };
  const int fl = trace_fmt_len([&](uint32_t i) { return ld(fmt + i); }, fmt_size, mem_room(g_win, g_lane, fmt));
  if (fl < 0) return fl;
  TraceConv cv[kTraceMaxArgs];
  const int n = trace_scan([&](uint32_t i) { return ld(fmt + i); }, (uint32_t)fl, cv);
  if (n < 0) return n;
  memset(&rec, 0xa5, sizeof(rec));  // (the log's records are not zeroed either)
  rec.unit = 7;
  rec.args[0] = a3, rec.args[1] = a4, rec.args[2] = a5;
  rec.fmt_len = (uint8_t)fl;
  rec.nargs = (uint8_t)n;
  memcpy(rec.fmt, (const void *)(uintptr_t)fmt, (size_t)fl);
  rec.fmt[fl] = 0;
  for (int a = 0; a < 3; a++) {
    rec.kind[a] = a < n ? (cv[a].conv == 's' ? TK_STR : TK_INT) : TK_NONE;
    rec.state[a] = TS_OK;
    rec.slen[a] = 0;
    if (rec.kind[a] != TK_STR) continue;
    const uint64_t s = rec.args[a];
    if (s == 0) {
      rec.state[a] = TS_NULL;
      continue;
    }
    const uint64_t room = mem_room(g_win, g_lane, s);
    if (room == 0) {
      rec.state[a] = TS_EFAULT;
      continue;
    }
    const uint64_t lim = trace_str_lim(room, cv[a].prec);
    uint32_t l = 0;
    while (l < lim && ld(s + l)) l++;
    rec.slen[a] = (uint8_t)l;
    memcpy(rec.str[a], (const void *)(uintptr_t)s, l);
    rec.str[a][l] = 0;
  }
  return 0;
}

static uint64_t put_str(size_t off, const char *s) {
  memcpy(g_mem + off, s, strlen(s) + 1);
  return A(off);
}

static int scan_of(const char *f) {
  TraceConv cv[kTraceMaxArgs];
  return trace_scan([&](uint32_t i) { return (uint8_t)f[i]; }, (uint32_t)strlen(f), cv);
}

// the formatter's line for (fmt, args) against `want`
static void line_is(const char *f, uint64_t a3, uint64_t a4, uint64_t a5, const std::string &want, int line) {
  const uint64_t fa = put_str(0, f);
  TraceRec rec;
  const int rc = capture(fa, strlen(f) + 1, a3, a4, a5, rec);
  char out[1024];
  const int len = rc == 0 ? trace_format(rec, out, sizeof(out)) : -99;
  if (rc != 0 || len != (int)want.size() || memcmp(out, want.data(), want.size()) != 0) {
    printf("FAIL line %d: \"%s\" gave rc %d \"%s\" (%d), snprintf \"%s\" (%zu)\n", line, f, rc, rc == 0 ? out : "", len,
           want.c_str(), want.size());
    bad++;
  }
}

#pragma GCC diagnostic ignored "-Wformat-nonliteral"
#pragma GCC diagnostic ignored "-Wformat"
template <class T>
static std::string sn(const char *f, T v) {
  char b[1024];
  const int k = snprintf(b, sizeof(b), f, v);
  return std::string(b, (size_t)k);
}

int main() {
  g_win = Win{A(0), A(sizeof(g_mem)), 0, 0, 0, 0, true};

  // ---- the scanner: every accepted conversion with every length modifier
  for (const char *conv : {"d", "i", "u", "x", "X", "o", "c", "p"})
    for (const char *lm : {"", "hh", "h", "l", "ll"})
      for (const char *fl : {"", "-", "+", " ", "#", "0", "-+ #0", "08", "-12.5", ".0", "64.64"}) {
        const std::string f = std::string("a%") + fl + lm + conv + "z";
        EXPECT(scan_of(f.c_str()) == 1);
      }
  for (const char *fl : {"", "-", "10", "-10", ".3", "-20.7", "64.64", "."}) EXPECT(scan_of((std::string("%") + fl + "s").c_str()) == 1);
  EXPECT(scan_of("") == 0);
  EXPECT(scan_of("plain text\n") == 0);
  EXPECT(scan_of("100%%") == 0);
  EXPECT(scan_of("%%%d%%") == 1);
  EXPECT(scan_of("%d %llx %s") == 3);
  {
    TraceConv cv[3];
    const char *f = "ab%-08.3llxcd%.5s";
    EXPECT(trace_scan([&](uint32_t i) { return (uint8_t)f[i]; }, (uint32_t)strlen(f), cv) == 2);
    EXPECT(cv[0].start == 2 && cv[0].end == 11 && cv[0].flags == (TF_MINUS | TF_ZERO) && cv[0].width == 8 &&
           cv[0].has_width && cv[0].prec == 3 && cv[0].len == TL_LL && cv[0].conv == 'x');
    EXPECT(cv[1].start == 13 && cv[1].end == 17 && cv[1].prec == 5 && !cv[1].has_width && cv[1].conv == 's');
  }
  // ---- each rejection
  for (const char *f : {"%*d", "%.*d", "%n", "%f", "%e", "%g", "%a", "%F", "%E", "%G", "%Lf", "%d%d%d%d", "%d%s%c%p",
                        "%", "abc%", "%5", "%-", "%ll", "%.", "%q", "%z", "%zd", "%jd", "%td", "%hhhd", "%llld",
                        "%65d", "%.65d", "%65s", "%.65s", "%100000000000d", "%ls", "%hs", "%+s", "%0s", "%#s", "% s",
                        "%-%", "%5%", "%S", "%C", "%m", "%$"})
    EXPECT(scan_of(f) == kTraceEinval);
  // caps at, one below and one above
  EXPECT(scan_of("%63d") == 1 && scan_of("%64d") == 1 && scan_of("%65d") == kTraceEinval);
  EXPECT(scan_of("%.63x") == 1 && scan_of("%.64x") == 1 && scan_of("%.65x") == kTraceEinval);
  EXPECT(scan_of("%d%d") == 2 && scan_of("%d%d%d") == 3 && scan_of("%d%d%d%d") == kTraceEinval);
  EXPECT(scan_of("%d%d%d%%") == 3);
  {  // the scanner reads nothing at or past len: a '%' as the last byte of the span
    const char *f = "ab%d";
    int maxi = -1;
    TraceConv cv[3];
    EXPECT(trace_scan([&](uint32_t i) { maxi = (int)i > maxi ? (int)i : maxi; return (uint8_t)f[i]; }, 3, cv) == kTraceEinval);
    EXPECT(maxi <= 2);
  }

  // ---- the format string's extent
  TraceRec rec;
  {
    memset(g_mem, 'x', sizeof(g_mem));
    const uint64_t f = put_str(100, "hi %d");
    EXPECT(capture(f, 6, 1, 0, 0, rec) == 0 && rec.fmt_len == 5);
    EXPECT(capture(f, 64, 1, 0, 0, rec) == 0);
    EXPECT(capture(f, 0, 1, 0, 0, rec) == kTraceEinval);   // fmt_size 0
    EXPECT(capture(f, 5, 1, 0, 0, rec) == kTraceEinval);   // fmt_size ends before the NUL
    EXPECT(capture(f, 3, 1, 0, 0, rec) == kTraceEinval);   // ... right after a '%'
    EXPECT(capture(0, 6, 1, 0, 0, rec) == kTraceEfault);   // NULL
    EXPECT(capture(A(sizeof(g_mem)), 6, 1, 0, 0, rec) == kTraceEfault);  // the byte after the window
    EXPECT(capture(A(0) - 1, 6, 1, 0, 0, rec) == kTraceEfault);
    // a string that runs off the end of its region before fmt_size
    memset(g_mem + sizeof(g_mem) - 4, 'y', 4);
    EXPECT(capture(A(sizeof(g_mem) - 4), 16, 0, 0, 0, rec) == kTraceEfault);
    EXPECT(capture(A(sizeof(g_mem) - 4), 4, 0, 0, 0, rec) == kTraceEinval);  // fmt_size ends first
    g_mem[sizeof(g_mem) - 1] = 0;
    EXPECT(capture(A(sizeof(g_mem) - 4), 16, 0, 0, 0, rec) == 0 && rec.fmt_len == 3);
    // the cap: 94, 95 bytes and a NUL fit, 96 do not
    for (uint32_t len : {94u, 95u, 96u, 200u}) {
      memset(g_mem + 200, 'k', len);
      g_mem[200 + len] = 0;
      EXPECT(capture(A(200), 4096, 0, 0, 0, rec) == (len <= kTraceFmtMax - 1 ? 0 : kTraceEinval));
      if (len <= kTraceFmtMax - 1) EXPECT(rec.fmt_len == len);
    }
  }

  // ---- the formatter against snprintf
  const uint64_t edge[] = {0, 1, (uint64_t)-1, (uint64_t)(int64_t)INT_MIN, (uint64_t)INT_MAX, 1ull << 63, 0x80, 0xff,
                           0x8000, 0xffff, 0x123456789abcdef0ull, 0xffffffff00000000ull, 'A', 10};
  int lines = 0;
  for (const char *fl : {"", "-", "+", " ", "#", "0", "-#", "+0", "#0", " 0", "- "})
    for (const char *wp : {"", "1", "12", "24", ".0", ".1", ".12", "20.10", "64", ".64"})
      for (const uint64_t v : edge) {
        for (const char *conv : {"d", "i", "u", "x", "X", "o"}) {
          const bool sg = conv[0] == 'd' || conv[0] == 'i';
          for (const char *lm : {"", "hh", "h", "l", "ll"}) {
            const std::string f = std::string("[%") + fl + wp + lm + conv + "]";
            std::string want;
            if (lm[0] == 'l') want = sn(f.c_str(), (unsigned long long)v);
            else if (sg) want = sn(f.c_str(), (int)(uint32_t)v);
            else want = sn(f.c_str(), (unsigned)(uint32_t)v);
            line_is(f.c_str(), v, 0, 0, want, __LINE__);
            lines++;
          }
        }
        {  // %c: the low byte; %p: the raw word; a length modifier changes neither
          const std::string fc = std::string("[%") + fl + wp + "c]", fp = std::string("[%") + fl + wp + "p]";
          line_is(fc.c_str(), v, 0, 0, sn(fc.c_str(), (int)(uint8_t)v), __LINE__);
          line_is(fp.c_str(), v, 0, 0, sn(fp.c_str(), (void *)(uintptr_t)v), __LINE__);
          const std::string flc = std::string("[%") + fl + wp + "lc]", fllp = std::string("[%") + fl + wp + "llp]";
          line_is(flc.c_str(), v, 0, 0, sn(fc.c_str(), (int)(uint8_t)v), __LINE__);
          line_is(fllp.c_str(), v, 0, 0, sn(fp.c_str(), (void *)(uintptr_t)v), __LINE__);
          lines += 4;
        }
      }
  // three arguments, %% and literals around them
  {
    char want[256];
    snprintf(want, sizeof(want), "100%% %d|%llx|%-6u!\n", -5, 0xdeadbeefcafeull, 77u);
    line_is("100%% %d|%llx|%-6u!\n", (uint64_t)-5, 0xdeadbeefcafeull, 77, want, __LINE__);
    line_is("no arguments", 1, 2, 3, "no arguments", __LINE__);
    line_is("", 1, 2, 3, "", __LINE__);
  }
  // %s: captured through the guard, NULL, outside every region, cut strings
  {
    const uint64_t s = put_str(1000, "hello, world");
    for (const char *sp : {"%s", "%20s", "%-20s|", "%.5s", "%.0s", "%10.3s", "%.64s", "%64s"}) {
      line_is(sp, s, 0, 0, sn(sp, "hello, world"), __LINE__);
      line_is(sp, 0, 0, 0, sn(sp, (const char *)nullptr), __LINE__);  // (null), as glibc prints it
      line_is(sp, 0x10, 0, 0, sn(sp, "(efault)"), __LINE__);          // outside every region
      line_is(sp, A(sizeof(g_mem)), 0, 0, sn(sp, "(efault)"), __LINE__);
    }
    EXPECT(sn("%s", (const char *)nullptr) == "(null)");
    // the per-string cap: 46, 47 bytes whole, 48 and more cut to 47
    for (uint32_t len : {46u, 47u, 48u, 300u}) {
      std::string str(len, 'q');
      put_str(1200, str.c_str());
      line_is("<%s>", A(1200), 0, 0, "<" + str.substr(0, len < kTraceStrMax ? len : kTraceStrMax) + ">", __LINE__);
    }
    // the precision bounds what is read: no NUL needed after it
    memset(g_mem + 2000, 'r', 64);
    EXPECT(capture(put_str(0, "%.5s"), 5, A(2000), 0, 0, rec) == 0 && rec.slen[0] == 5);
    // a string with no NUL before its region ends is cut there
    memset(g_mem + sizeof(g_mem) - 3, 'e', 3);
    line_is("%s|", A(sizeof(g_mem) - 3), 0, 0, "eee|", __LINE__);
    EXPECT(capture(put_str(0, "%s"), 3, A(sizeof(g_mem) - 3), 0, 0, rec) == 0 && rec.slen[0] == 3 &&
           rec.state[0] == TS_OK);
    // three strings
    const uint64_t s2 = put_str(1100, "two");
    char want[256];
    snprintf(want, sizeof(want), "%s %s %.2s", "hello, world", "two", "hello, world");
    line_is("%s %s %.2s", s, s2, s, want, __LINE__);
  }
  // a record nobody validated never faults the formatter
  {
    memset(&rec, 0xff, sizeof(rec));
    char out[64];
    EXPECT(trace_format(rec, out, sizeof(out)) >= 0);
    memset(&rec, 0, sizeof(rec));
    memcpy(rec.fmt, "%s %n", 6);
    rec.fmt_len = 5;
    EXPECT(trace_format(rec, out, sizeof(out)) == 12 && !strcmp(out, "(bad format)"));
    memcpy(rec.fmt, "%s|%s", 6);  // kinds that do not match the format: no pointer is followed
    rec.kind[0] = TK_INT;
    rec.args[0] = 0x1234;
    rec.kind[1] = TK_STR;
    rec.state[1] = TS_OK;
    rec.slen[1] = 255;
    memset(rec.str[1], 'z', sizeof(rec.str[1]));
    EXPECT(trace_format(rec, out, sizeof(out)) == 9 + 47 && !strncmp(out, "(efault)|zzz", 12));
    // a small buffer: the length still reported, the text cut and terminated
    memcpy(rec.fmt, "0123456789", 11);
    rec.fmt_len = 10;
    char tiny[4];
    EXPECT(trace_format(rec, tiny, sizeof(tiny)) == 10 && !strcmp(tiny, "012"));
  }
  if (bad) {
    printf("%d failures\n", bad);
    return 1;
  }
  printf("%d lines compared\nOK\n", lines);
  return 0;
}
