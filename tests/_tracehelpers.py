"""A pure-Python statement of the task and trace helpers as the device
implements them (Trace and task helpers): bpf_trace_printk's
format grammar and the line glibc's snprintf gives for it, written out by hand
(tests/test_trace_model.py checks it against libc), bpf_get_current_comm as
strncpy, and the capture rules of a %s argument."""
M64 = 0xFFFFFFFFFFFFFFFF
EFAULT = (-14) & M64
EINVAL = (-22) & M64
FMT_MAX = 96   # format bytes, the NUL included
STR_MAX = 47   # captured bytes of a %s argument
MAX_ARGS = 3
MAX_FIELD = 64

NULL = None            # a %s argument that was a NULL pointer


class _Efault:         # ... that pointed outside every region
    def __repr__(self):
        return "EFAULTSTR"


EFAULTSTR = _Efault()


def default_comm() -> bytes:
    import os
    return os.path.basename(os.readlink("/proc/self/exe")).encode()[:63]


def default_uid_gid() -> int:
    import os
    return (os.getgid() << 32) | os.getgid()


def get_current_comm(comm: bytes, size: int) -> bytes:
    """The `size` bytes strncpy(buf, comm, size) writes: comm up to and with
    its NUL, the rest zero; size <= len(comm) bytes of comm and no NUL."""
    assert b"\0" not in comm and len(comm) <= 63
    return comm[:size] + bytes(max(0, size - len(comm)))


class Conv:
    __slots__ = ("start", "end", "flags", "width", "prec", "len", "conv")

    def __repr__(self):
        return f"Conv({self.flags!r},{self.width},{self.prec},{self.len!r},{self.conv!r})"


def scan(fmt: bytes):
    """The conversions of `fmt` (no NUL inside), or None where the helper
    answers -EINVAL."""
    assert b"\0" not in fmt
    out, i, n = [], 0, len(fmt)

    def at(k):
        return chr(fmt[k]) if k < n else "\0"

    while i < n:
        if at(i) != "%":
            i += 1
            continue
        c = Conv()
        c.start = i
        i += 1
        if i >= n:
            return None
        if at(i) == "%":
            i += 1
            continue
        c.flags = ""
        while at(i) in "-+ #0":
            c.flags += at(i)
            i += 1
        c.width = None
        while at(i).isdigit() and at(i).isascii():
            c.width = (c.width or 0) * 10 + int(at(i))
            if c.width > MAX_FIELD:
                return None
            i += 1
        c.prec = None
        if at(i) == ".":
            i += 1
            c.prec = 0
            while at(i).isdigit() and at(i).isascii():
                c.prec = c.prec * 10 + int(at(i))
                if c.prec > MAX_FIELD:
                    return None
                i += 1
        c.len = ""
        for m in ("hh", "h", "ll", "l"):
            if fmt[i:i + len(m)] == m.encode():
                c.len = m
                i += len(m)
                break
        c.conv = at(i)
        i += 1
        if c.conv == "s":
            if c.flags.replace("-", "") or c.len:
                return None
        elif c.conv not in "diuxXocp":
            return None
        c.end = i
        if len(out) == MAX_ARGS:
            return None
        out.append(c)
    return out


def _pad(body: bytes, c: Conv) -> bytes:
    w = c.width or 0
    if len(body) >= w:
        return body
    return body + b" " * (w - len(body)) if "-" in c.flags else b" " * (w - len(body)) + body


def _number(neg: bool, mag: int, base: int, upper: bool, c: Conv, signed: bool, alt_prefix: bytes) -> bytes:
    digits = ""
    m = mag
    while m:
        digits = "0123456789abcdef"[m % base] + digits
        m //= base
    if upper:
        digits = digits.upper()
    prec = c.prec
    if prec is None:
        if not digits:
            digits = "0"
    else:
        digits = digits.rjust(prec, "0")
    if "#" in c.flags and base == 8 and not digits.startswith("0"):
        digits = "0" + digits
    prefix = b""
    if signed:
        prefix = b"-" if neg else b"+" if "+" in c.flags else b" " if " " in c.flags else b""
    if mag != 0:
        prefix += alt_prefix
    body = digits.encode()
    w = c.width or 0
    if "0" in c.flags and "-" not in c.flags and prec is None and len(prefix) + len(body) < w:
        body = b"0" * (w - len(prefix) - len(body)) + body
    return _pad(prefix + body, c)


def format_conv(c: Conv, arg) -> bytes:
    """One conversion as snprintf prints it.  arg: the raw 64-bit word, or for
    %s the captured bytes / NULL / EFAULTSTR."""
    if c.conv == "s":
        if arg is NULL:
            s = b"(null)" if c.prec is None or c.prec >= 6 else b""
        else:
            s = b"(efault)" if arg is EFAULTSTR else bytes(arg)
            if c.prec is not None:
                s = s[:c.prec]
        return _pad(s, c)
    v = arg & M64
    if c.conv == "c":  # the low byte; a length modifier changes nothing
        return _pad(bytes([v & 0xff]), c)
    if c.conv == "p":  # glibc: "(nil)" as a string, else %#lx keeping '+' and ' '
        if v == 0:
            return _pad(b"(nil)", c)
        return _number(False, v, 16, False, c, True, b"0x")
    bits = {"hh": 8, "h": 16, "": 32, "l": 64, "ll": 64}[c.len]
    v &= (1 << bits) - 1
    if c.conv in "di":
        neg = bool(v >> (bits - 1))
        return _number(neg, (1 << bits) - v if neg else v, 10, False, c, True, b"")
    base = {"u": 10, "x": 16, "X": 16, "o": 8}[c.conv]
    alt = {"x": b"0x", "X": b"0X"}.get(c.conv, b"") if "#" in c.flags else b""
    return _number(False, v, base, c.conv == "X", c, False, alt)


def respec(c: Conv) -> bytes:
    """The conversion as the host formatter hands it to snprintf: no length
    modifier on c / p / s, ll for l."""
    s = "%" + "".join(f for f in "-+ #0" if f in c.flags)
    if c.width is not None:
        s += str(c.width)
    if c.prec is not None:
        s += "." + str(c.prec)
    if c.conv in "diuxXo":
        s += {"l": "ll"}.get(c.len, c.len)
    return (s + c.conv).encode()


def format_line(fmt: bytes, args) -> bytes:
    """The line of one call (None: -EINVAL).  args: up to three of the above."""
    cv = scan(fmt)
    if cv is None:
        return None
    out, pos = b"", 0
    for c, a in zip(cv, args):
        out += fmt[pos:c.start].replace(b"%%", b"%")
        out += format_conv(c, a)
        pos = c.end
    return out + fmt[pos:].replace(b"%%", b"%")


def capture_str(mem: bytes, prec=None):
    """What the device keeps of a %s argument whose region holds `mem` from
    the pointer to the region's end: cut at the first NUL, the cap, the
    precision and the region's end."""
    lim = min(len(mem), STR_MAX, prec if prec is not None else STR_MAX)
    s = bytes(mem[:lim])
    nul = s.find(b"\0")
    return s if nul < 0 else s[:nul]


def trace_printk_ret(fmt_mem: bytes, fmt_size: int) -> tuple:
    """(r0, the format) for a format pointer whose region holds `fmt_mem` from
    the pointer to the region's end (empty: outside every region)."""
    if fmt_size == 0:
        return EINVAL, None
    if len(fmt_mem) == 0:
        return EFAULT, None
    span = min(fmt_size, FMT_MAX)
    for n in range(span + 1):
        if n >= span:
            return EINVAL, None
        if n >= len(fmt_mem):
            return EFAULT, None
        if fmt_mem[n] == 0:
            f = bytes(fmt_mem[:n])
            return (0, f) if scan(f) is not None else (EINVAL, None)
