"""A Python model of BPF_MAP_TYPE_STACK_TRACE, bpf_get_stackid and
bpf_get_stack, restated from the reference (runtime/src/bpf_map/userspace/
stack_trace_map.cpp / .hpp; bpf_helper.cpp:791-893), and builders for the test
programs.  The stack is the unit's recorded one, where the reference asks the
uprobe attach implementation.  hash_combine is boost::hash_combine on a 64-bit
size_t as Boost 1.74 defines it (restated, not checked against a Boost build).
The one rule that is the project's: a destination the launch's range guard
refuses answers -EFAULT (the test passes the verdict in)."""
import errno

from bpftime_amd import isa
from bpftime_amd.isa import Asm

M64 = (1 << 64) - 1
ENOTSUP, ENOENT, EFAULT, EINVAL = (-95) & M64, (-2) & M64, (-14) & M64, (-22) & M64
USER_STACK, FAST_CMP, REUSE, BUILD_ID = 1 << 8, 1 << 9, 1 << 10, 1 << 11
MUL = 0xc6a4a7935bd1e995


def hash_combine(h: int, k: int) -> int:
    k = (k * MUL) & M64
    k ^= k >> 47
    k = (k * MUL) & M64
    h ^= k
    h = (h * MUL) & M64
    return (h + 0xe6546b64) & M64


def hash_stack_trace(stk) -> int:                       # stack_trace_map.hpp:27-35
    seed = hash_combine(0, len(stk))
    for x in stk:
        seed = hash_combine(seed, x & M64)
    return seed


class StackMap:
    """stack_trace_map_impl: id -> frames."""

    def __init__(self, key_size: int, value_size: int, max_entries: int):
        if key_size != 4 or value_size % 8 or max_entries == 0:
            raise ValueError("EINVAL")
        self.value_size, self.max_entries = value_size, max_entries
        self.data = {}
        self.err = 0

    def fill(self, stk, reuse: bool, fast_cmp: bool) -> int:    # fill_stack_trace (:96-137)
        i = hash_stack_trace(stk) % self.max_entries
        if i not in self.data:
            self.data[i] = list(stk)
            return i
        equals = True
        if not fast_cmp:
            equals = len(self.data[i]) == len(stk)      # the contents are never compared
        if not equals and reuse:
            self.data[i] = list(stk)
        return i

    def lookup(self, key):                              # the device map's value_size bytes
        if key is None:
            self.err = errno.EINVAL
            return None
        k = int.from_bytes(key, "little")
        if k not in self.data:
            self.err = errno.ENOENT
            return None
        raw = b"".join(x.to_bytes(8, "little") for x in self.data[k])
        return raw + bytes(self.value_size - len(raw))

    def update(self, key, value, flags=0) -> int:
        return -95

    def delete(self, key) -> int:
        if key is None:
            self.err = errno.EINVAL
            return -1
        k = int.from_bytes(key, "little")
        if k not in self.data:
            self.err = errno.ENOENT
            return -1
        del self.data[k]
        return 0

    def next_key(self, key):
        self.err = errno.ENOTSUP
        return None


def skipped(stack, flags: int):
    return list(stack[flags & 0xFF:])


def get_stackid(m, stack, flags: int) -> int:
    """bpf_get_stackid as a 64-bit r0.  stack: the unit's frames, None when the
    batch has no stack source, [] when the unit has none; m: the StackMap r2
    names, None when it names no STACK_TRACE map."""
    if not flags & USER_STACK:
        return ENOTSUP
    if stack is None:
        return ENOTSUP
    if len(stack) == 0:
        return ENOENT
    stk = skipped(stack, flags)
    if m is None:
        return EINVAL
    return m.fill(stk, bool(flags & REUSE), bool(flags & FAST_CMP)) & 0xFFFFFFFF


def get_stack(stack, size: int, flags: int, range_ok: bool = True):
    """bpf_get_stack: (r0, the bytes written at buf)."""
    if not flags & USER_STACK:
        return ENOTSUP, b""
    if flags & BUILD_ID:
        return ENOTSUP, b""
    if stack is None:
        return ENOTSUP, b""
    if len(stack) == 0:
        return ENOENT, b""
    stk = skipped(stack, flags)
    n = min(len(stk), size)                             # a frame count against a byte count
    if n and not range_ok:
        return EFAULT, b""
    return 0, b"".join(x.to_bytes(8, "little") for x in stk)[:n]


# ---- programs --------------------------------------------------------------------
def stackid_prog(map_fd, flags, raw_r2=None, flags_from_unit=False) -> bytes:
    """r0 = bpf_get_stackid(ctx, map, flags).  flags_from_unit: r3 is the u64 at
    unit + 0 (no constant the loader can prove)."""
    a = Asm()
    if flags_from_unit:
        a.ldx(8, 3, 1, 0)
    else:
        a.lddw(3, flags & M64)
    if raw_r2 is not None:
        a.lddw(2, raw_r2 & M64)
    else:
        a.ld_map_fd(2, map_fd)
    a.call(isa.BPF_FUNC_get_stackid)
    return a.exit().assemble()


def stackid_twice_prog(map_fd, flags1, flags2) -> bytes:
    """Two calls; r0 = first | second << 32."""
    a = Asm()
    a.mov64(6, "r1")
    a.ld_map_fd(2, map_fd).mov64(3, flags1).call(isa.BPF_FUNC_get_stackid)
    a.mov64(7, "r0").alu64("lsh", 7, 32).alu64("rsh", 7, 32)
    a.mov64(1, "r6").ld_map_fd(2, map_fd).mov64(3, flags2).call(isa.BPF_FUNC_get_stackid)
    a.alu64("lsh", 0, 32).alu64("or", 0, "r7")
    return a.exit().assemble()


BUF = 128                                               # the program's stack buffer at fp - 128


def getstack_prog(size, flags, dst="stack") -> bytes:
    """r0 = bpf_get_stack(ctx, buf, size, flags).  dst "stack": buf = fp - 128,
    filled with 0xA5 first and copied to unit + 8 .. unit + 136 afterwards;
    "unit": buf = unit + 8; "null": buf = 0; "past": buf = fp - 4 (more than 4
    bytes leave the stack)."""
    a = Asm()
    a.mov64(6, "r1")
    a.lddw(2, 0xA5A5A5A5A5A5A5A5)
    for i in range(BUF // 8):
        a.stx(8, 10, -BUF + 8 * i, "r2")
    if dst == "stack":
        a.mov64(2, "r10").add64(2, -BUF)
    elif dst == "unit":
        a.mov64(2, "r6").add64(2, 8)
    elif dst == "null":
        a.mov64(2, 0)
    else:
        a.mov64(2, "r10").add64(2, -4)
    a.lddw(3, size & M64).lddw(4, flags & M64).mov64(1, "r6").call(isa.BPF_FUNC_get_stack)
    if dst != "unit":
        for i in range(BUF // 8):
            a.ldx(8, 2, 10, -BUF + 8 * i).stx(8, 6, 8 + 8 * i, "r2")
    return a.exit().assemble()


def lookup_prog(map_fd, key: int = 0) -> bytes:
    """r0 = the first frame of slot `key` (0 for NULL) through helper 1."""
    a = Asm()
    a.st(4, 10, -4, key).mov64(2, "r10").add64(2, -4).ld_map_fd(1, map_fd).call(isa.BPF_FUNC_map_lookup_elem)
    a.jmp("jeq", 0, 0, "out")
    a.ldx(8, 0, 0, 0)
    return a.label("out").exit().assemble()
