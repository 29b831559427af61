"""A Python model of BPF_MAP_TYPE_PERF_EVENT_ARRAY and bpf_perf_event_output,
restated from the reference (runtime/src/bpf_map/userspace/
perf_event_array_map.cpp; bpf_helper.cpp:506-566; software_perf_event_buffer's
output_data / append_record_parts / copy_next_record_to,
runtime/src/handler/perf_event_handler.cpp:300-450), and builders for the test
programs.  The one rule that is the project's and not the reference's: a data
range the launch's range guard refuses answers -EFAULT (the test passes the
verdict in, the model does not know the windows)."""
import errno
import struct

from bpftime_amd import isa
from bpftime_amd.isa import Asm

M64 = (1 << 64) - 1
FAIL = M64                       # (uint64_t)-1
EFAULT = (-14) & M64
HDR = 12                         # perf_event_header (8) + u32 size
MAX_DATA = 65535 - HDR - 7       # perf_event_handler.cpp:359-363
PERF_RECORD_SAMPLE = 9


def record_size(size: int) -> int:
    return (HDR + size + 7) & ~7             # :364-366


class PerfArray:
    """perf_event_array_map_impl: max_entries ints, all -1 at first."""

    def __init__(self, max_entries: int):
        self.slots = [-1] * max_entries
        self.err = 0

    def _key(self, key: bytes):
        k = struct.unpack("<i", key)[0]
        if k < 0 or k >= len(self.slots):
            self.err = errno.EINVAL
            return None
        return k

    def lookup(self, key: bytes):
        k = self._key(key)
        return None if k is None else struct.pack("<i", self.slots[k])

    def update(self, key: bytes, value: bytes, flags: int = 0) -> int:
        k = self._key(key)
        if k is None:
            return -1
        self.slots[k] = struct.unpack("<i", value)[0]     # flags are not read (:38-49)
        return 0

    def delete(self, key: bytes) -> int:
        k = self._key(key)
        if k is None:
            return -1
        self.slots[k] = -1
        return 0

    def next_key(self, key):
        if key is None:
            return struct.pack("<i", 0)
        k = struct.unpack("<i", key)[0]
        if k + 1 == len(self.slots):                      # the last key, before the range check (:70-74)
            self.err = errno.ENOENT
            return None
        if k < 0 or k >= len(self.slots):
            self.err = errno.EINVAL
            return None
        return struct.pack("<i", k + 1)

    def image(self) -> bytes:
        return b"".join(struct.pack("<i", s) for s in self.slots)


class Ring:
    """software_perf_event_buffer's data ring; data_bytes 0: never mmapped."""

    def __init__(self, data_bytes: int = 0):
        self.data_bytes, self.head, self.tail = data_bytes, 0, 0
        self.data = bytearray(data_bytes)
        self.written = bytearray(data_bytes)               # 1: a byte some record's header or data wrote

    def _write(self, pos: int, src: bytes):
        for i, b in enumerate(src):                        # write_wrapped (:378-391)
            at = (pos + i) & (self.data_bytes - 1)
            self.data[at] = b
            self.written[at] = 1

    def append(self, header: bytes, data: bytes, rs: int) -> bool:      # append_record_parts (:306-353)
        if self.data_bytes == 0 or rs > self.data_bytes:
            return False
        used = self.head - self.tail
        if self.head < self.tail or used >= self.data_bytes:
            return False
        if self.data_bytes - used <= rs:                   # one byte stays free
            return False
        self._write(self.head, header)
        self._write(self.head + len(header), data)
        self.head += rs
        return True

    def output(self, data: bytes) -> int:                  # output_data (:355-376)
        if len(data) > MAX_DATA:
            return -1
        rs = record_size(len(data))
        self.append(struct.pack("<IHHI", PERF_RECORD_SAMPLE, 0, rs, rs - HDR), bytes(data), rs)
        return 0                                           # append's result is ignored

    def _read(self, pos: int, n: int) -> bytes:
        return bytes(self.data[(pos + i) & (self.data_bytes - 1)] for i in range(n))

    def fetch(self, cap: int = 1 << 30):
        """The consumer's walk (copy_next_record_to, :409-450): (count, bytes)."""
        out, n = b"", 0
        if self.data_bytes == 0:
            return 0, out
        if self.head < self.tail:
            self.tail = self.head
            return 0, out
        while self.tail != self.head:
            size = struct.unpack("<H", self._read(self.tail + 6, 2))[0]
            if size < 8 or size > self.data_bytes:
                self.tail = self.head
                break
            if size > self.head - self.tail or len(out) + size > cap:
                break
            out += self._read(self.tail, size)
            self.tail += size
            n += 1
        return n, out


def output(array, cpu: int, perfs: dict, data, size: int, range_ok: bool = True) -> int:
    """bpf_perf_event_output as a 64-bit r0.  array: a PerfArray, or None when
    r2 names no PERF_EVENT_ARRAY; perfs: fd -> Ring for the software perf events
    (a tracepoint, a closed fd or a map is simply not in it); data: the bytes
    at [data, data + size) or None when the range guard refuses them."""
    if array is None or cpu >= len(array.slots):
        return FAIL
    ring = perfs.get(array.slots[cpu])
    if ring is None:
        return FAIL
    if size > MAX_DATA:
        return FAIL
    if size and (not range_ok or data is None):
        return EFAULT
    ring.output(bytes(data[:size]) if size else b"")
    return 0


def parse(raw: bytes) -> list:
    """A fetched stream end to end -> [(record_size, data)]; every header checked."""
    out, off = [], 0
    while off < len(raw):
        typ, misc, rs, ds = struct.unpack_from("<IHHI", raw, off)
        assert (typ, misc) == (PERF_RECORD_SAMPLE, 0) and rs % 8 == 0 and rs >= 16 and ds == rs - HDR, (off, typ, misc, rs, ds)
        assert off + rs <= len(raw)
        out.append((rs, raw[off + HDR:off + rs]))
        off += rs
    return out


# ---- programs --------------------------------------------------------------------
STRIDE = 128
DATA_OFF, DATA_LEN = 8, 64       # unit: u8 size @0, u8 @1 spare, bytes @8..72 the event


def emit_prog(map_fd, src="unit", size=None, flags=0, data=None, second_map=None, raw_r2=None) -> bytes:
    """r0 = bpf_perf_event_output(ctx, map, flags, data, size) over a raw unit.
    src "unit": data = unit + 8; "stack": the 64 bytes copied to fp-64 first.
    size None: the u8 at unit + 0.  data: ("null",) / ("unit", off) / ("stack",
    off from fp) overrides the pointer.  second_map: a second call on that map
    follows, r0 = first | second << 32 (both 0 / -1 kept in 32 bits each).
    raw_r2: r2 is this plain number, not an lddw map fd."""
    a = Asm()
    a.mov64(6, "r1")
    if src == "stack" or (data and data[0] == "stack"):
        for i in range(DATA_LEN // 8):
            a.ldx(8, 2, 6, DATA_OFF + 8 * i).stx(8, 10, -DATA_LEN + 8 * i, "r2")

    def call(mfd):
        if data is None:
            if src == "stack":
                a.mov64(4, "r10").add64(4, -DATA_LEN)
            else:
                a.mov64(4, "r6").add64(4, DATA_OFF)
        elif data[0] == "null":
            a.mov64(4, 0)
        elif data[0] == "unit":
            a.mov64(4, "r6").add64(4, data[1])
        else:
            a.mov64(4, "r10").add64(4, data[1])
        if size is None:
            a.ldx(1, 5, 6, 0)
        else:
            a.lddw(5, size & M64)
        if raw_r2 is not None:
            a.lddw(2, raw_r2 & M64)
        else:
            a.ld_map_fd(2, mfd)
        a.lddw(3, flags & M64)
        a.mov64(1, "r6").call(isa.BPF_FUNC_perf_event_output)

    call(map_fd)
    if second_map is not None:
        a.mov64(7, "r0").alu64("lsh", 7, 32).alu64("rsh", 7, 32)
        call(second_map)
        a.alu64("lsh", 0, 32).alu64("or", 0, "r7")
    return a.exit().assemble()


def sys_enter_emitter(map_fd) -> bytes:
    """sys_enter: one 16-byte event {pid_tgid, syscall nr} per call, from the stack."""
    a = Asm()
    a.mov64(6, "r1")
    a.call(isa.BPF_FUNC_get_current_pid_tgid).stx(8, 10, -16, "r0")
    a.ldx(8, 2, 6, 8).stx(8, 10, -8, "r2")
    a.mov64(1, "r6").ld_map_fd(2, map_fd).mov64(3, 0).mov64(4, "r10").add64(4, -16).mov64(5, 16)
    a.call(isa.BPF_FUNC_perf_event_output)
    return a.mov64(0, 0).exit().assemble()
