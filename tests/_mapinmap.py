"""A pure-Python model of BPF_MAP_TYPE_ARRAY_OF_MAPS, written from the map's
documented semantics (Map-in-map): max_entries int32 slots, 0 =
empty, untyped.  Host operations return what the map returns and leave the
errno they set in ``err``; the program-side operations return the helper's
r0.  ``register`` hooks models into an OracleVM as helpers 1 / 2 / 3, so the
oracle interpreter runs the same bytecode: a lookup on an outer fd yields the
slot's fd, and every other fd falls through to the oracle's own maps."""
import ctypes as C
import errno
import struct

import numpy as np

FAIL = 0xFFFFFFFFFFFFFFFF
EINVAL64 = (-errno.EINVAL) & FAIL
ENOTSUP64 = (-95) & FAIL
MAX_FDS = 1024  # an fd past the table names no map: NULL / -1


class Outer:
    def __init__(self, max_entries: int):
        self.max_entries = max_entries
        self.slots = [0] * max_entries
        self.err = 0

    def _fail(self, e: int) -> int:
        self.err = e
        return -1

    # ---- the host (from_syscall) -------------------------------------------
    def update(self, key: bytes, value: bytes, flags: int = 0) -> int:
        """The array map's update on a 4-byte value."""
        if flags & 0xFFFFFFFF not in (0, 1, 2):
            return self._fail(errno.EINVAL)
        k = struct.unpack("<I", key[:4])[0]
        if k < self.max_entries and flags == 1:
            return self._fail(errno.EEXIST)
        if k >= self.max_entries:
            return self._fail(errno.E2BIG)
        self.slots[k] = struct.unpack("<i", value[:4])[0]  # not checked against any fd table
        return 0

    def lookup(self, key: bytes):
        """A 4-byte copy of the slot, or None (ENOENT) out of range."""
        k = struct.unpack("<I", key[:4])[0]
        if k >= self.max_entries:
            self._fail(errno.ENOENT)
            return None
        return struct.pack("<i", self.slots[k])

    def delete(self, key: bytes) -> int:
        return self._fail(errno.EINVAL)

    def next_key(self, key):
        """The array's: 0 for no key or one out of range, None (ENOENT) after
        the last, else key + 1."""
        k = None if key is None else struct.unpack("<I", key[:4])[0]
        if k is None or k >= self.max_entries:
            return struct.pack("<I", 0)
        if k == self.max_entries - 1:
            self._fail(errno.ENOENT)
            return None
        return struct.pack("<I", k + 1)

    def push(self, *_):
        return -95  # -ENOTSUP, as pop and peek

    pop = peek = push

    # ---- a program ---------------------------------------------------------
    def prog_lookup(self, k: int) -> int:
        """(void *)((u_int64_t)map_id): the slot sign-extended; 0 (an empty
        slot, or a key out of range) is NULL."""
        if k >= self.max_entries:
            return 0
        return self.slots[k] & FAIL

    def prog_update(self) -> int:
        return EINVAL64  # "Map in maps only support update from syscall"

    prog_delete = prog_update

    def image(self) -> np.ndarray:
        return np.frombuffer(struct.pack(f"<{self.max_entries}i", *self.slots), dtype=np.uint8)


_HELPER = C.CFUNCTYPE(C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64)


def register(ovm, po, maps: dict) -> list:
    """Helpers 1 / 2 / 3 (and 87 / 88 / 89: -ENOTSUP on every map here) on an
    OracleVM, answered by `maps` ({outer fd: Outer}) for outer fds.  Any other
    r1 below MAX_FDS falls through to the oracle's own lookup / update /
    delete, which answer NULL / -1 for an fd that names no map; an r1 past the
    table (a negative slot, sign-extended) names no map either.  Returns the
    callbacks, which the caller keeps alive while the VM runs."""
    L = po.lib()
    reg = L.orc_vm_register
    reg.restype = C.c_int
    reg.argtypes = [C.c_void_p, C.c_uint, C.c_char_p, _HELPER]
    L.orc_map_lookup.restype = C.c_void_p
    L.orc_map_lookup.argtypes = [C.c_int, C.c_void_p]
    L.orc_map_update.restype = C.c_long
    L.orc_map_update.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint64]
    L.orc_map_delete.restype = C.c_long
    L.orc_map_delete.argtypes = [C.c_int, C.c_void_p]

    def lookup(m, key, _3, _4, _5):
        o = maps.get(m)
        if o is not None:
            return o.prog_lookup(struct.unpack("<I", C.string_at(key, 4))[0])
        return (L.orc_map_lookup(int(m), key) or 0) if m < MAX_FDS else 0

    def update(m, key, value, flags, _5):
        if m in maps:
            return maps[m].prog_update()
        return (L.orc_map_update(int(m), key, value, flags) & FAIL) if m < MAX_FDS else FAIL

    def delete(m, key, _3, _4, _5):
        if m in maps:
            return maps[m].prog_delete()
        return (L.orc_map_delete(int(m), key) & FAIL) if m < MAX_FDS else FAIL

    def no_elem(m, _2, _3, _4, _5):
        return ENOTSUP64 if m < MAX_FDS else FAIL

    cbs = [_HELPER(f) for f in (lookup, update, delete, no_elem, no_elem, no_elem)]
    names = (b"bpf_map_lookup_elem", b"bpf_map_update_elem", b"bpf_map_delete_elem", b"bpf_map_push_elem",
             b"bpf_map_pop_elem", b"bpf_map_peek_elem")
    for idx, name, cb in zip((1, 2, 3, 87, 88, 89), names, cbs):
        assert reg(ovm.h, idx, name, cb) == 0
    return cbs
