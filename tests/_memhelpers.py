"""A pure-Python statement of bpf_probe_read* (4 / 112 / 113),
bpf_probe_read_*_str (45 / 114 / 115) and bpf_strncmp (182) as the device
implements them (Copy and compare helpers), over ``bytes``; a
window list that answers -EFAULT from addresses alone, never dereferencing;
and ``register``, which hooks the seven ids into an OracleVM so the oracle
interpreter runs the same bytecode against the model."""
import ctypes as C

M64 = 0xFFFFFFFFFFFFFFFF
EFAULT = (-14) & M64
COPY_IDS, STR_IDS, STRNCMP_ID = (4, 112, 113), (45, 114, 115), 182
NAMES = {4: b"bpf_probe_read", 112: b"bpf_probe_read_user", 113: b"bpf_probe_read_kernel",
         45: b"bpf_probe_read_str", 114: b"bpf_probe_read_user_str", 115: b"bpf_probe_read_kernel_str",
         182: b"bpf_strncmp"}


def s64(v: int) -> int:
    v &= M64
    return v - (1 << 64) if v >> 63 else v


# ---- the three semantics over bytes ------------------------------------------
def probe_read(size: int, src: bytes):
    """(r0, the bytes written to dst or None when dst is untouched).  size is
    the signed 64-bit argument; src holds at least size bytes."""
    if size < 0:
        return EFAULT, None
    if size == 0:
        return 0, None
    assert len(src) >= size
    return 0, bytes(src[:size])


def copy_ascending(mem: bytearray, d: int, s: int, n: int) -> None:
    """The copy's contract where the ranges overlap: one byte at a time in
    ascending order, so a destination that starts inside the source repeats
    the bytes in front of it.  (Disjoint ranges: any order gives the same.)"""
    for i in range(n):
        mem[d + i] = mem[s + i]


def probe_read_str(bufsz: int, src: bytes):
    """strncpy(buf, src, bufsz): (0, the bufsz bytes of buf) -- the source up
    to and with its first NUL, or bufsz bytes when it has none (then no NUL is
    added), the rest zero.  src: what lies at the source, as far as known
    (bytes behind the first NUL are never looked at).  Returns 0, not the
    kernel's length: the reference's answer."""
    if bufsz == 0:
        return 0, None
    head = bytes(src[:bufsz])
    nul = head.find(b"\0")
    if nul >= 0:
        head = head[:nul]
    else:
        assert len(head) == bufsz, "the source ends before a NUL or bufsz"
    return 0, head + bytes(bufsz - len(head))


def strncmp(s1: bytes, n: int, s2: bytes) -> int:
    """r0: 0 when no byte differs before a common NUL or n bytes; else the
    difference of the first differing bytes as unsigned chars, sign-extended
    to 64 bits (libc fixes only the sign; the device fixes this magnitude)."""
    for i in range(n):
        a, b = s1[i], s2[i]
        if a != b:
            return (a - b) & M64
        if a == 0:
            return 0
    return 0


# ---- the guard over addresses --------------------------------------------------
class Windows:
    """`windows`: the [lo, hi) ranges a program may access (the batch, each
    map's storage).  `fences`: mapped memory outside every window (the slack
    around a batch) -- a range touching one is rejected.  An address in
    neither is the lane's own memory (the oracle interpreter's stack, an XDP
    ctx copy), which the model cannot place: such a range is accepted unless
    it reaches a window or a fence.  A range must start in a window and end
    inside the same one; it never wraps."""

    def __init__(self, windows=(), fences=()):
        self.windows, self.fences = list(windows), list(fences)

    def room(self, a: int):
        """Bytes from a to the end of its window; 0 inside a fence or at
        NULL; None for the lane's own memory."""
        for lo, hi in self.windows:
            if lo <= a < hi:
                return hi - a
        for lo, hi in self.fences:
            if lo <= a < hi:
                return 0
        return 0 if a == 0 else None

    def ok(self, a: int, n: int) -> bool:
        if n < 1 or a + n > 1 << 64:
            return False
        r = self.room(a)
        if r is None:
            return not any(a < hi and lo < a + n for lo, hi in self.windows + self.fences)
        return n <= r


_HELPER = C.CFUNCTYPE(C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64)


def register(ovm, po, win: Windows = None) -> list:
    """The seven helpers on an OracleVM, answered by the model over the
    oracle's memory (`win`: its windows; None: every range is accepted).
    Returns the callbacks, which the caller keeps alive while the VM runs."""
    reg = po.lib().orc_vm_register
    reg.restype = C.c_int
    reg.argtypes = [C.c_void_p, C.c_uint, C.c_char_p, _HELPER]
    win = win or Windows()

    def scan(a: int, lim: int) -> bytes:
        """The bytes at a up to and with the first NUL, lim at the most,
        read one at a time: nothing behind the NUL is touched."""
        out = bytearray()
        while len(out) < lim:
            b = C.string_at(a + len(out), 1)
            out += b
            if b == b"\0":
                break
        return bytes(out)

    def copy(dst, size, src, _4, _5):
        size = s64(size)
        if size <= 0:
            return probe_read(size, b"")[0]
        if not win.ok(dst, size) or not win.ok(src, size):
            return EFAULT
        if abs(dst - src) < size:
            base = min(dst, src)
            mem = bytearray(C.string_at(base, abs(dst - src) + size))
            copy_ascending(mem, dst - base, src - base, size)
            C.memmove(dst, bytes(mem[dst - base:dst - base + size]), size)
            return 0
        rc, out = probe_read(size, C.string_at(src, size))
        C.memmove(dst, out, size)
        return rc

    def copy_str(buf, bufsz, src, _4, _5):
        if bufsz == 0:
            return 0
        if not win.ok(buf, bufsz):
            return EFAULT
        room = win.room(src)
        lim = bufsz if room is None else min(bufsz, room)
        got = scan(src, lim)
        if lim < bufsz and not got.endswith(b"\0"):
            return EFAULT  # the window ends before the string or bufsz does
        rc, out = probe_read_str(bufsz, got)
        C.memmove(buf, out, bufsz)
        return rc

    def cmp(s1, n, s2, _4, _5):
        if n == 0:
            return 0
        rooms = [n if r is None else r for r in (win.room(s1), win.room(s2))]
        lim = min(n, *rooms)
        for i in range(lim):
            a, b = C.string_at(s1 + i, 1), C.string_at(s2 + i, 1)
            r = strncmp(a, 1, b)
            if r or a == b"\0":
                return r
        return EFAULT if lim < n else 0

    cbs = []
    for ids, fn in ((COPY_IDS, copy), (STR_IDS, copy_str), ((STRNCMP_ID,), cmp)):
        cb = _HELPER(fn)
        cbs.append(cb)
        for i in ids:
            assert reg(ovm.h, i, NAMES[i], cb) == 0
    return cbs
