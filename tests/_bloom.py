"""A pure-Python model of BPF_MAP_TYPE_BLOOM_FILTER, written from the map's
documented semantics (Bloom filter): bit-array sizing, Jenkins
lookup3 ``hashlittle`` over bytes, push / peek, and the byte layout of the
array.  ``register`` hooks the model into an OracleVM as helpers 87 / 88 / 89,
so the oracle interpreter runs the same bytecode against it."""
import ctypes as C

import numpy as np

M32 = 0xFFFFFFFF
ENOTSUP = 95


def bits_for(max_entries: int, nr_hashes: int) -> int:
    want = max_entries * nr_hashes * 7 // 5
    want = min(max(want, 64), 1 << 31)
    bits = 1
    while bits < want:
        bits <<= 1
    return bits


def _rot(x: int, k: int) -> int:
    return ((x << k) | (x >> (32 - k))) & M32


def jhash(key: bytes, initval: int) -> int:
    """lookup3 hashlittle(key, len(key), initval), the byte-wise form."""
    n = len(key)
    a = b = c = (0xDEADBEEF + n + initval) & M32
    k = 0
    while n > 12:
        a = (a + int.from_bytes(key[k:k + 4], "little")) & M32
        b = (b + int.from_bytes(key[k + 4:k + 8], "little")) & M32
        c = (c + int.from_bytes(key[k + 8:k + 12], "little")) & M32
        a = (a - c) & M32; a ^= _rot(c, 4); c = (c + b) & M32
        b = (b - a) & M32; b ^= _rot(a, 6); a = (a + c) & M32
        c = (c - b) & M32; c ^= _rot(b, 8); b = (b + a) & M32
        a = (a - c) & M32; a ^= _rot(c, 16); c = (c + b) & M32
        b = (b - a) & M32; b ^= _rot(a, 19); a = (a + c) & M32
        c = (c - b) & M32; c ^= _rot(b, 4); b = (b + a) & M32
        n -= 12
        k += 12
    if n == 0:
        return c
    tail = key[k:k + n] + bytes(12 - n)
    a = (a + int.from_bytes(tail[0:4], "little")) & M32
    b = (b + int.from_bytes(tail[4:8], "little")) & M32
    c = (c + int.from_bytes(tail[8:12], "little")) & M32
    c ^= b; c = (c - _rot(b, 14)) & M32
    a ^= c; a = (a - _rot(c, 11)) & M32
    b ^= a; b = (b - _rot(a, 25)) & M32
    c ^= b; c = (c - _rot(b, 16)) & M32
    a ^= c; a = (a - _rot(c, 4)) & M32
    b ^= a; b = (b - _rot(a, 14)) & M32
    c ^= b; c = (c - _rot(b, 24)) & M32
    return c


class Bloom:
    def __init__(self, value_size: int, max_entries: int, nr_hashes: int, seed: int):
        assert value_size > 0 and max_entries > 0
        self.value_size = value_size
        self.nr_hashes = nr_hashes if nr_hashes else 5
        self.seed = seed & M32
        self.bits = bits_for(max_entries, self.nr_hashes)
        self.mask = self.bits - 1
        self.array = np.zeros(self.bits // 8, dtype=np.uint8)

    def positions(self, value: bytes):
        assert len(value) == self.value_size
        return [jhash(value, (self.seed + i) & M32) & self.mask for i in range(self.nr_hashes)]

    def push(self, value: bytes, flags: int = 0) -> int:
        if flags != 0:
            return -1
        for p in self.positions(value):
            self.array[p >> 3] |= 1 << (p & 7)
        return 0

    def peek(self, value: bytes) -> bool:
        return all(self.array[p >> 3] & (1 << (p & 7)) for p in self.positions(value))

    def bytes(self) -> np.ndarray:
        return self.array.copy()


_HELPER = C.CFUNCTYPE(C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64)


def register(ovm, po, filters: dict) -> list:
    """Helpers 87 / 88 / 89 on an OracleVM, answered by `filters` ({map fd:
    Bloom}); any other fd is a map without the operation (-ENOTSUP).  Returns
    the callbacks, which the caller keeps alive while the VM runs."""
    reg = po.lib().orc_vm_register
    reg.restype = C.c_int
    reg.argtypes = [C.c_void_p, C.c_uint, C.c_char_p, _HELPER]
    unsup = (-ENOTSUP) & 0xFFFFFFFFFFFFFFFF
    fail = 0xFFFFFFFFFFFFFFFF

    def push(m, value, flags, _4, _5):
        f = filters.get(m)
        if f is None:
            return unsup
        return fail if f.push(C.string_at(value, f.value_size), flags) else 0

    def pop(m, value, _3, _4, _5):
        return fail if m in filters else unsup

    def peek(m, value, _3, _4, _5):
        f = filters.get(m)
        if f is None:
            return unsup
        return 0 if f.peek(C.string_at(value, f.value_size)) else fail

    cbs = [_HELPER(push), _HELPER(pop), _HELPER(peek)]
    for idx, name, cb in zip((87, 88, 89), (b"bpf_map_push_elem", b"bpf_map_pop_elem", b"bpf_map_peek_elem"), cbs):
        assert reg(ovm.h, idx, name, cb) == 0
    return cbs
