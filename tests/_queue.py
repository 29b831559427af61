"""A pure-Python model of BPF_MAP_TYPE_QUEUE / BPF_MAP_TYPE_STACK, written from
the maps' documented semantics (Queues and stacks): a list with a
capacity and a LIFO flag.  Every operation returns what the map returns and
leaves the errno it sets in ``err``.  Beside the list the model keeps the
documented ring (``image``: the header's head / tail tickets and the slots
with their zero pad bytes), so a device map can be compared byte for byte.
``register`` hooks models into an OracleVM as helpers 87 / 88 / 89 and 1 / 2 /
3, so the oracle interpreter runs the same bytecode against them."""
import ctypes as C
import errno

import numpy as np

BPF_EXIST = 2
FAIL = 0xFFFFFFFFFFFFFFFF


class Ring:
    def __init__(self, value_size: int, max_entries: int, lifo: bool):
        assert value_size > 0 and max_entries > 0
        self.value_size, self.max_entries, self.lifo = value_size, max_entries, lifo
        self.items = []  # oldest first
        # the ring: the element with ticket t in slot t % max_entries, at a
        # stride of value_size rounded up to 4; count = tail - head
        self.head = self.tail = 0
        self.stride = (value_size + 3) & ~3
        self.slots = bytearray(self.stride * max_entries)
        self.err = 0
        self._keep = None  # the buffer a lookup's pointer aims into

    def _fail(self, e: int) -> int:
        self.err = e
        return -1

    # bpf_map_push_elem: flags 0 (BPF_ANY) or BPF_EXIST
    def push(self, value, flags: int = 0) -> int:
        if value is None or flags not in (0, BPF_EXIST):
            return self._fail(errno.EINVAL)
        return self._append(value, flags)

    # bpf_map_update_elem: a push, the key ignored, the flags not validated
    def update(self, value, flags: int = 0) -> int:
        if value is None:
            return self._fail(errno.EINVAL)
        return self._append(value, flags)

    def _append(self, value, flags: int) -> int:
        assert len(value) == self.value_size
        if len(self.items) >= self.max_entries:
            if flags != BPF_EXIST:
                return self._fail(errno.E2BIG)
            self.items.pop(0)  # the oldest: the queue's head, the stack's bottom
            self.head += 1
        self.items.append(bytes(value))
        at = (self.tail % self.max_entries) * self.stride
        self.slots[at:at + self.stride] = bytes(value) + bytes(self.stride - self.value_size)
        self.tail += 1
        return 0

    def _end(self) -> int:
        return len(self.items) - 1 if self.lifo else 0

    def peek(self):
        """(0, value) or (-1, None)."""
        if not self.items:
            return self._fail(errno.ENOENT), None
        return 0, self.items[self._end()]

    def pop(self):
        if not self.items:
            return self._fail(errno.ENOENT), None
        if self.lifo:
            self.tail -= 1
        else:
            self.head += 1
        return 0, self.items.pop(self._end())

    lookup = peek

    def delete(self) -> int:
        return self.pop()[0]

    def next_key(self) -> int:
        return self._fail(errno.EINVAL)

    def count(self) -> int:
        return len(self.items)

    def image(self) -> np.ndarray:
        """The map's storage: a 128-byte header {u64 head, u64 tail}, then the
        slots (a removed element's bytes stay where they were)."""
        hdr = self.head.to_bytes(8, "little") + self.tail.to_bytes(8, "little") + bytes(112)
        return np.frombuffer(hdr + bytes(self.slots), dtype=np.uint8)


_HELPER = C.CFUNCTYPE(C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64)
ENOTSUP64 = (-95) & FAIL


def register(ovm, po, maps: dict) -> list:
    """Helpers 87 / 88 / 89 and 1 / 2 / 3 on an OracleVM, answered by `maps`
    ({map fd: Ring}).  Helpers 1 / 2 / 3 on any other fd fall through to the
    oracle's own lookup / update / delete; 87 / 88 / 89 on any other fd meet a
    map without the operation (-ENOTSUP).  Returns the callbacks, which the
    caller keeps alive while the VM runs."""
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

    def u64(rc: int) -> int:
        return rc & FAIL

    def value_at(q, ptr):
        return C.string_at(ptr, q.value_size) if ptr else None

    def copy_out(q, ptr, rc, v):
        if rc == 0:
            C.memmove(ptr, v, q.value_size)
        return u64(rc)

    def push(m, value, flags, _4, _5):
        q = maps.get(m)
        return ENOTSUP64 if q is None else u64(q.push(value_at(q, value), flags))

    def pop(m, value, _3, _4, _5):
        q = maps.get(m)
        if q is None:
            return ENOTSUP64
        if not value:
            return u64(q._fail(errno.EINVAL))
        return copy_out(q, value, *q.pop())

    def peek(m, value, _3, _4, _5):
        q = maps.get(m)
        if q is None:
            return ENOTSUP64
        if not value:
            return u64(q._fail(errno.EINVAL))
        return copy_out(q, value, *q.peek())

    def lookup(m, key, _3, _4, _5):
        q = maps.get(m)
        if q is None:
            return L.orc_map_lookup(C.c_int(m & 0xFFFFFFFF).value, key) or 0
        rc, v = q.lookup()
        if rc:
            return 0
        q._keep = C.create_string_buffer(v, q.value_size)  # alive until the map's next lookup
        return C.addressof(q._keep)

    def update(m, key, value, flags, _5):
        q = maps.get(m)
        if q is None:
            return u64(L.orc_map_update(C.c_int(m & 0xFFFFFFFF).value, key, value, flags))
        return u64(q.update(value_at(q, value), flags))

    def delete(m, key, _3, _4, _5):
        q = maps.get(m)
        if q is None:
            return u64(L.orc_map_delete(C.c_int(m & 0xFFFFFFFF).value, key))
        return u64(q.delete())

    cbs = [_HELPER(f) for f in (lookup, update, delete, push, pop, peek)]
    names = (b"bpf_map_lookup_elem", b"bpf_map_update_elem", b"bpf_map_delete_elem", b"bpf_map_push_elem",
             b"bpf_map_pop_elem", b"bpf_map_peek_elem")
    for idx, name, cb in zip((1, 2, 3, 87, 88, 89), names, cbs):
        assert reg(ovm.h, idx, name, cb) == 0
    return cbs
