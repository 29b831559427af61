"""The model of the copy / compare helpers (tests/_memhelpers.py) against
the C library it restates: memcpy, strncpy, and the sign of strncmp; its
overlap contract and its window list.  No GPU."""
import ctypes as C
import ctypes.util
import itertools

import numpy as np
import pytest

import _memhelpers as mh

libc = C.CDLL(ctypes.util.find_library("c") or "libc.so.6")
libc.memcpy.restype = C.c_void_p
libc.memcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
libc.strncpy.restype = C.c_void_p
libc.strncpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
libc.strncmp.restype = C.c_int
libc.strncmp.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]

SIZES = [0, 1, 3, 4, 5, 7, 8, 9, 16, 31, 48, 64]


def sign(v: int) -> int:
    return (v > 0) - (v < 0)


def test_probe_read_is_memcpy():
    rng = np.random.default_rng(1)
    for n in SIZES:
        src = rng.integers(0, 256, 80, dtype=np.uint8).tobytes()
        dst = C.create_string_buffer(b"\xaa" * 80, 80)
        libc.memcpy(dst, src, n)
        rc, out = mh.probe_read(n, src)
        assert rc == 0
        assert (out or b"") + b"\xaa" * (80 - n) == dst.raw
    assert mh.probe_read(-1, b"") == (mh.EFAULT, None)
    assert mh.probe_read(-(1 << 63), b"") == (mh.EFAULT, None)
    assert mh.s64(mh.EFAULT) == -14 and mh.s64((1 << 64) - 1) == -1


@pytest.mark.parametrize("bufsz", [0, 1, 5, 16])
def test_probe_read_str_is_strncpy(bufsz):
    rng = np.random.default_rng(2)
    for nul in (0, 1, bufsz // 2, bufsz - 1, None):
        if nul is not None and nul < 0:
            continue
        s = bytearray(rng.integers(1, 256, 40, dtype=np.uint8).tobytes())  # no NUL of its own
        if nul is not None:
            s[nul] = 0
            s[nul + 1:nul + 3] = b"\x55\x00"   # bytes (and a NUL) behind the first NUL: never copied
        src = C.create_string_buffer(bytes(s), 40)
        dst = C.create_string_buffer(b"\xaa" * 32, 32)
        libc.strncpy(dst, src, bufsz)
        rc, out = mh.probe_read_str(bufsz, bytes(s))
        assert rc == 0
        assert (out or b"") + b"\xaa" * (32 - bufsz) == dst.raw
        if bufsz and (nul is None or nul >= bufsz):
            assert 0 not in out            # no NUL is added


def test_strncmp_has_libc_sign_and_byte_difference():
    alphabet = [0, 1, 0x41, 0x7f, 0x80, 0xff]
    for n in (0, 1, 2, 3, 4):
        for a in itertools.product(alphabet, repeat=3):
            for b in itertools.product(alphabet, repeat=3):
                s1, s2 = bytes(a) + b"\0", bytes(b) + b"\0"
                got = mh.s64(mh.strncmp(s1, n, s2))
                want = libc.strncmp(C.create_string_buffer(s1, 4), C.create_string_buffer(s2, 4), n)
                assert sign(got) == sign(want), (s1, s2, n)
                if got:
                    i = next(k for k in range(n) if s1[k] != s2[k])
                    assert got == s1[i] - s2[i] and -255 <= got <= 255
    # unsigned bytes, a difference at index n and one behind a common NUL
    assert mh.s64(mh.strncmp(b"\x80", 1, b"\x7f")) == 1
    assert mh.s64(mh.strncmp(b"\x7f", 1, b"\xff")) == -128
    assert mh.strncmp(b"abcX", 3, b"abcY") == 0
    assert mh.strncmp(b"ab\0X", 4, b"ab\0Y") == 0
    assert mh.strncmp(b"X", 0, b"Y") == 0


def test_overlap_is_an_ascending_byte_copy():
    mem = bytearray(range(32))
    mh.copy_ascending(mem, 3 + 3, 3, 16)          # dst = src + 3: the three bytes in front repeat
    assert bytes(mem[6:22]) == bytes([3, 4, 5] * 6)[:16]
    mem = bytearray(range(32))
    mh.copy_ascending(mem, 5, 8, 16)              # dst = src - 3: a memmove
    assert bytes(mem[5:21]) == bytes(range(8, 24))


def test_windows():
    w = mh.Windows(windows=[(0x1000, 0x2000), (0x2000, 0x3000)], fences=[(0xF00, 0x1000), (0x3000, 0x3100)])
    assert w.ok(0x1000, 0x1000) and w.ok(0x1FFF, 1) and w.ok(0x2000, 1)
    assert not w.ok(0x1000, 0x1001)               # spans two adjacent windows
    assert not w.ok(0x1FF8, 16) and not w.ok(0x2FF8, 16)
    assert not w.ok(0xFFF, 1) and not w.ok(0xFF8, 16) and not w.ok(0x3000, 1)
    assert not w.ok(0, 1) and not w.ok(0x1000, 0) and not w.ok((1 << 64) - 1, 2) and not w.ok(0x1000, 1 << 63)
    assert w.room(0x1FF0) == 16 and w.room(0x3000) == 0 and w.room(0) == 0 and w.room(0x9000) is None
    assert w.ok(0x9000, 64)                       # the lane's own memory: not the model's to place
    assert not w.ok(0xE00, 0x101)                 # ... unless it runs into a fence
    assert mh.Windows().ok(0x1234, 8)
