"""The Python model of bpf_trace_printk's lines and bpf_get_current_comm
(tests/_tracehelpers.py) against libc: snprintf over the accepted grammar, a
few hundred seeded formats and the edge values; strncpy for the comm copy.
The GPU tests take their expected lines from the model, so the model itself
has to agree with what the reference would print."""
import ctypes as C
import random

import _tracehelpers as th

libc = C.CDLL(None)
EDGE = [0, 1, 7, 0x41, 0x7f, 0x80, 0xff, 0x7fff, 0x8000, 0xffff, 0x7fffffff, 0x80000000, 0xffffffff, 1 << 32,
        (1 << 63) - 1, 1 << 63, th.M64, 0x123456789abcdef0, 10, 100]


def c_snprintf(spec: bytes, conv: th.Conv, arg) -> bytes:
    buf = C.create_string_buffer(512)
    if conv.conv == "s":
        a = C.c_char_p(b"(efault)" if arg is th.EFAULTSTR else arg)  # (None: a NULL pointer)
    elif conv.conv == "p":
        a = C.c_void_p(arg)
    elif conv.conv == "c":
        a = C.c_int(arg & 0xff)
    elif conv.len in ("l", "ll"):
        a = C.c_ulonglong(arg)
    else:
        a = C.c_uint(arg & 0xffffffff)
    n = libc.snprintf(buf, C.c_size_t(512), spec, a)
    assert 0 <= n < 512
    return buf.raw[:n]


def one(flags, width, prec, lm, conv, arg):
    f = ("%" + flags + ("" if width is None else str(width)) + ("" if prec is None else "." + str(prec)) + lm +
         conv).encode()
    cv = th.scan(f)
    assert cv is not None and len(cv) == 1, f
    want = c_snprintf(th.respec(cv[0]), cv[0], arg)
    got = th.format_conv(cv[0], arg)
    assert got == want, (f, arg, got, want)
    assert th.format_line(b"<" + f + b">%%", [arg]) == b"<" + want + b">%"


def test_integer_conversions_match_snprintf():
    rng = random.Random(20260101)
    n = 0
    for conv in "diuxXocp":
        for lm in ("", "hh", "h", "l", "ll"):
            for v in EDGE:
                one("", None, None, lm, conv, v)
                n += 1
    for _ in range(600):
        flags = "".join(f for f in "-+ #0" if rng.random() < 0.3)
        width = rng.choice([None, None, 1, 2, 5, 12, 24, 64])
        prec = rng.choice([None, None, 0, 1, 3, 12, 64])
        one(flags, width, prec, rng.choice(["", "hh", "h", "l", "ll"]), rng.choice("diuxXocp"),
            rng.choice(EDGE + [rng.getrandbits(64)]))
        n += 1
    assert n >= 1000


def test_string_conversions_match_snprintf():
    rng = random.Random(7)
    strs = [b"", b"a", b"hello", b"hello, world", b"x" * 47, th.NULL, th.EFAULTSTR]
    for s in strs:
        for flags in ("", "-"):
            for width in (None, 1, 6, 20, 64):
                for prec in (None, 0, 1, 5, 6, 7, 64):
                    one(flags, width, prec, "", "s", s)
    for _ in range(100):
        one(rng.choice(["", "-"]), rng.choice([None, 3, 30]), rng.choice([None, 2, 9]), "", "s",
            bytes(rng.choice(b"abcxyz ") for _ in range(rng.randrange(0, 40))))


def test_lines_with_three_arguments():
    buf = C.create_string_buffer(256)
    n = libc.snprintf(buf, C.c_size_t(256), b"%d %llx %s|100%%\n", C.c_int(-3), C.c_ulonglong(0xabcdef0123), b"name")
    assert th.format_line(b"%d %llx %s|100%%\n", [(-3) & th.M64, 0xabcdef0123, b"name"]) == buf.raw[:n]
    assert th.format_line(b"plain", []) == b"plain"
    assert th.format_line(b"", []) == b""


def test_rejections():
    for f in (b"%*d", b"%.*d", b"%n", b"%f", b"%e", b"%g", b"%a", b"%d%d%d%d", b"%", b"ab%", b"%5", b"%q", b"%zd",
              b"%65d", b"%.65d", b"%65s", b"%.65s", b"%ls", b"%+s", b"%0s", b"%hhhd", b"%llld", b"%-%"):
        assert th.scan(f) is None, f
        assert th.format_line(f, [0, 0, 0]) is None
    for f in (b"%64d", b"%.64d", b"%d%d%d", b"%d%d%d%%", b"%-64.64s"):
        assert th.scan(f) is not None, f
    assert th.trace_printk_ret(b"hi\0", 0) == (th.EINVAL, None)
    assert th.trace_printk_ret(b"hi\0", 2) == (th.EINVAL, None)
    assert th.trace_printk_ret(b"hi\0", 3) == (0, b"hi")
    assert th.trace_printk_ret(b"", 3) == (th.EFAULT, None)
    assert th.trace_printk_ret(b"hi", 3) == (th.EFAULT, None)
    assert th.trace_printk_ret(b"hi", 2) == (th.EINVAL, None)
    assert th.trace_printk_ret(b"k" * 95 + b"\0", 200) == (0, b"k" * 95)
    assert th.trace_printk_ret(b"k" * 96 + b"\0", 200) == (th.EINVAL, None)


def test_capture_of_string_arguments():
    assert th.capture_str(b"abc\0def") == b"abc"
    assert th.capture_str(b"q" * 100) == b"q" * 47
    assert th.capture_str(b"q" * 100, prec=5) == b"q" * 5
    assert th.capture_str(b"eee") == b"eee"          # the region ends first
    assert th.capture_str(b"ab\0", prec=1) == b"a"


def test_get_current_comm_is_strncpy():
    libc.strncpy.restype = C.c_void_p
    for comm in (b"a", b"python3", b"fifteen-chars-x", b"c" * 63):
        for size in (0, 1, len(comm) - 1, len(comm), len(comm) + 1, 16, 64, 100):
            if size < 0:
                continue
            buf = C.create_string_buffer(b"\xaa" * 128, 128)
            libc.strncpy(buf, comm, C.c_size_t(size))
            assert buf.raw[:size] == th.get_current_comm(comm, size), (comm, size)
            assert buf.raw[size:] == b"\xaa" * (128 - size)
