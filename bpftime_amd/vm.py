"""Thin Python host layer over the C ABI (test / bench convenience).

Mirrors the reference's embedder usage of the VM C ABI
(vm/example/main.c:25-51, benchmark/test_embed.c:155-168) and of the shm map
API (runtime/include/bpftime_shm.hpp:303-345).  Everything here calls
libbpftime_amd.so; nothing executes eBPF on the CPU.
"""
from __future__ import annotations

import ctypes as C
import struct
from typing import Optional

import numpy as np

from . import isa
from ._lib import (BpfLinkCreateArgs, BpfMapAttr, CallRecords, EbpfBatch, LaunchInfo, MapDumpArgs, SysRecords,
                   TraceLine, XdpCompleteArgs, lib)
from ._lib import PerfEvent as PerfEventRec

CTX_RAW, CTX_XDP, CTX_SYSCALL, CTX_SYSCALL_EXIT, CTX_UPROBE = 0, 1, 2, 3, 4
UPROBE, URETPROBE, UPROBE_OVERRIDE, UREPLACE = 6, 7, 1008, 1009  # uprobe attach kinds (include/bpftime_amd.h)
PT_REGS_BYTES = 168  # x86-64 struct pt_regs: the EBPF_CTX_UPROBE unit
SYSCALL_RECORD, SYSCALL_RECORD_FULL, SYSCALL_RECORD_TIMED = 64, 96, 128  # include/bpftime_amd.h replay records
DISPATCH_THREADS, DISPATCH_PROGRAMS = 0x100, 0x200  # dispatch plans (include/bpftime_amd.h)
BATCH_SYNC, BATCH_ORDERED, BATCH_UNCHECKED, BATCH_SYS_NR, BATCH_TIMED = 0x1, 0x2, 0x4, 0x8, 0x10
DUMP_DELETE = 1  # BPFTIME_AMD_DUMP_DELETE (include/bpftime_amd.h)


class EbpfError(RuntimeError):
    pass


def _err() -> str:
    e = lib().bpftime_amd_last_error()
    return e.decode() if e else ""


# ---------------------------------------------------------------------------
# device memory
# ---------------------------------------------------------------------------
class DeviceBuffer:
    def __init__(self, nbytes: int):
        self.nbytes = int(nbytes)
        self.ptr = lib().bpftime_amd_dev_alloc(max(self.nbytes, 1))
        if not self.ptr:
            raise EbpfError(f"device alloc of {nbytes} bytes failed")

    @classmethod
    def from_array(cls, a: np.ndarray) -> "DeviceBuffer":
        a = np.ascontiguousarray(a)
        b = cls(a.nbytes)
        b.upload(a)
        return b

    def upload(self, a: np.ndarray, offset: int = 0) -> None:
        a = np.ascontiguousarray(a)
        if lib().bpftime_amd_memcpy_htod(C.c_void_p(self.ptr + offset), a.ctypes.data, a.nbytes):
            raise EbpfError("htod failed")

    def download(self, dtype=np.uint8, count: Optional[int] = None, offset: int = 0) -> np.ndarray:
        dt = np.dtype(dtype)
        n = (self.nbytes - offset) // dt.itemsize if count is None else count
        out = np.empty(n, dtype=dt)
        if n and lib().bpftime_amd_memcpy_dtoh(out.ctypes.data, C.c_void_p(self.ptr + offset), out.nbytes):
            raise EbpfError("dtoh failed")
        return out

    def zero(self) -> None:
        lib().bpftime_amd_memset(C.c_void_p(self.ptr), 0, self.nbytes)

    def free(self) -> None:
        if self.ptr:
            lib().bpftime_amd_dev_free(C.c_void_p(self.ptr))
            self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ---------------------------------------------------------------------------
# software perf events: the consumer side of bpf_perf_event_output
# ---------------------------------------------------------------------------
class PerfEvent:
    """A software perf event record (PERF_TYPE_SOFTWARE) and its device ring:
    what a PERF_EVENT_ARRAY slot names.  mmap() gives it the ring, as the
    consumer's mmap of the perf fd does in the reference."""

    def __init__(self, cpu: int = 0, fd: int = -1, type_: int = 1, sample_type: int = 1 << 10, config: int = 10,
                 data_bytes: int = 0):
        e = PerfEventRec(type=type_, pid=-1, enabled=0, tracepoint_id=-1, sys_nr=-1, cpu=cpu,
                         sample_type=sample_type, config=config)
        self.fd = lib().bpftime_amd_perf_event_record(fd, C.byref(e))
        if self.fd < 0:
            raise EbpfError(f"perf event create failed: {_err()}")
        if data_bytes:
            self.mmap(data_bytes)

    def mmap(self, data_bytes: int) -> None:
        if lib().bpftime_amd_perf_event_mmap(self.fd, data_bytes) < 0:
            raise EbpfError(f"perf event mmap failed: {_err()}")

    def state(self):
        """(data_head, data_tail, data_bytes); data_bytes 0: no ring yet."""
        h, t, b = C.c_uint64(), C.c_uint64(), C.c_uint64()
        if lib().bpftime_amd_perf_event_ring_state(self.fd, C.byref(h), C.byref(t), C.byref(b)) < 0:
            raise EbpfError(f"fd {self.fd} is not a software perf event")
        return h.value, t.value, b.value

    def fetch_raw(self, cap: int = 1 << 20):
        """(record count, the records' bytes back to back as they lie in the
        ring): bpftime_amd_perf_event_fetch."""
        buf = C.create_string_buffer(max(cap, 1))
        used = C.c_uint64(0)
        n = lib().bpftime_amd_perf_event_fetch(self.fd, buf, cap, C.byref(used))
        if n < 0:
            raise EbpfError(f"perf event fetch failed: {_err()}")
        return n, buf.raw[:used.value]

    def fetch(self, cap: int = 1 << 20) -> list:
        """The samples' data: per record the `size` bytes behind the 12-byte
        header (the data, then the padding to 8)."""
        n, raw = self.fetch_raw(cap)
        out, off = [], 0
        for _ in range(n):
            rs = int.from_bytes(raw[off + 6:off + 8], "little")
            out.append(raw[off + 12:off + rs])
            off += rs
        return out

    def close(self) -> None:
        lib().bpftime_close(self.fd)


# ---------------------------------------------------------------------------
# maps
# ---------------------------------------------------------------------------
class Map:
    def __init__(self, type_: int, key_size: int, value_size: int, max_entries: int, flags: int = 0,
                 name: str = "", fd: int = -1, map_extra: int = 0):
        attr = BpfMapAttr(type=type_, key_size=key_size, value_size=value_size, max_ents=max_entries,
                          flags=flags, map_extra=map_extra)
        self.fd = lib().bpftime_maps_create(fd, name.encode(), attr)
        if self.fd < 0:
            raise EbpfError(f"map create failed: {_err()}")
        self.type, self.key_size, self.value_size, self.max_entries = type_, key_size, value_size, max_entries

    @classmethod
    def from_fd(cls, fd: int) -> "Map":
        """Wrap a map record created elsewhere (e.g. by BpfObject.load)."""
        if not lib().bpftime_is_map_fd(fd):
            raise EbpfError(f"fd {fd} is not a map")
        m = cls.__new__(cls)
        m.fd = fd
        a = BpfMapAttr()
        if lib().bpftime_map_get_info(fd, C.byref(a), None, None) < 0:
            raise EbpfError(f"fd {fd}: no map info")
        m.type, m.key_size, m.value_size, m.max_entries = a.type, a.key_size, a.value_size, a.max_ents
        return m

    def ringbuf_fetch(self, cap: int = 1 << 24) -> list:
        """Consume committed ring-buffer records (BPF_MAP_TYPE_RINGBUF)."""
        buf = C.create_string_buffer(cap)
        used = C.c_uint64(0)
        n = lib().bpftime_amd_ringbuf_fetch(self.fd, buf, cap, C.byref(used))
        if n < 0:
            raise EbpfError(f"ringbuf fetch failed: {_err()}")
        raw, out, off = buf.raw[:used.value], [], 0
        for _ in range(n):
            ln = int.from_bytes(raw[off:off + 4], "little")
            out.append(raw[off + 4:off + 4 + ln])
            off += 4 + ln
        return out

    @property
    def user_value_size(self) -> int:
        return lib().bpftime_map_value_size_from_syscall(self.fd)

    def lookup(self, key: bytes) -> Optional[bytes]:
        k = C.create_string_buffer(bytes(key), len(key))
        p = lib().bpftime_map_lookup_elem(self.fd, k)
        if not p:
            return None
        return C.string_at(p, self.user_value_size)

    def update(self, key: bytes, value: bytes, flags: int = 0) -> int:
        k = C.create_string_buffer(bytes(key), len(key))
        v = C.create_string_buffer(bytes(value), len(value))
        return lib().bpftime_map_update_elem(self.fd, k, v, flags)

    def delete(self, key: bytes) -> int:
        k = C.create_string_buffer(bytes(key), len(key))
        return lib().bpftime_map_delete_elem(self.fd, k)

    def next_key(self, key: Optional[bytes]) -> Optional[bytes]:
        out = C.create_string_buffer(self.key_size)
        kb = C.create_string_buffer(bytes(key), len(key)) if key is not None else None
        if lib().bpftime_map_get_next_key(self.fd, kb, out) < 0:
            return None
        return out.raw

    def storage_bytes(self) -> int:
        n = C.c_uint64(0)
        lib().bpftime_amd_map_device_ptr(self.fd, C.byref(n))
        return n.value

    def device_ptr(self) -> int:
        return lib().bpftime_amd_map_device_ptr(self.fd, None)

    def snapshot(self) -> np.ndarray:
        n = self.storage_bytes()
        out = np.empty(n, dtype=np.uint8)
        if lib().bpftime_amd_map_snapshot(self.fd, out.ctypes.data, n):
            raise EbpfError("snapshot failed")
        return out

    def restore(self, raw: np.ndarray) -> None:
        raw = np.ascontiguousarray(raw, dtype=np.uint8)
        if lib().bpftime_amd_map_restore(self.fd, raw.ctypes.data, raw.nbytes):
            raise EbpfError("restore failed")

    def geometry(self):
        nb, ss, ko, vo, nc = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        lib().bpftime_amd_map_geometry(self.fd, C.byref(nb), C.byref(ss), C.byref(ko), C.byref(vo), C.byref(nc))
        return nb.value, ss.value, ko.value, vo.value, nc.value

    def hash_items(self) -> dict:
        """Decode a (per-CPU) hash map snapshot into {key: value-bytes}."""
        nb, ss, ko, vo, nc = self.geometry()
        raw = self.snapshot().reshape(nb, ss)
        vs = self.value_size * (nc if self.type == isa.BPF_MAP_TYPE_PERCPU_HASH else 1)
        filled = raw[:, :4].view(np.uint32)[:, 0] == 1
        out = {}
        for row in raw[filled]:
            out[bytes(row[ko:ko + self.key_size])] = bytes(row[vo:vo + vs])
        return out

    def count(self) -> int:
        return lib().bpftime_amd_map_count(self.fd)

    def dump(self, cap: Optional[int] = None, start: int = 0, delete: bool = False, keys: bool = True,
             values: bool = True):
        """bpftime_amd_map_dump: up to `cap` entries (None: max_entries) from
        the cursor `start`, in get_next_key order, compacted on the device.
        -> (keys uint8[count, key_size], values uint8[count, user_value_size],
        next, end); continue with start=next until next == end.  delete: the
        returned entries are also removed (HASH / PERCPU_HASH).  keys / values
        False: that output is not asked for (its array comes back with
        count rows of width 0)."""
        cap = self.max_entries if cap is None else int(cap)
        vs = self.user_value_size
        # (the library writes count <= cap entries; a huge cap is clipped to what the map can hold)
        room = min(cap, max(self.max_entries, self.geometry()[0]))
        k = np.empty((room, self.key_size if keys else 0), dtype=np.uint8)
        v = np.empty((room, vs if values else 0), dtype=np.uint8)
        a = MapDumpArgs(fd=self.fd, flags=DUMP_DELETE if delete else 0, start=start, cap=room,
                        keys=k.ctypes.data if keys and room else None,
                        values=v.ctypes.data if values and room else None)
        C.set_errno(0)
        if lib().bpftime_amd_map_dump(C.byref(a)) < 0:
            e = EbpfError(_err())
            e.errno = C.get_errno()
            raise e
        return k[:a.count], v[:a.count], a.next, a.end

    # BPF_MAP_TYPE_ARRAY_OF_MAPS (map_in_maps.hpp)
    def set_inner(self, index: int, inner, flags: int = 0) -> int:
        """ARRAY_OF_MAPS: store the map `inner` (a Map or a raw int: the slots
        are untyped) in slot `index`; what bpftime_map_update_elem returns."""
        fd = inner.fd if isinstance(inner, Map) else int(inner)
        return self.update(struct.pack("<I", index), struct.pack("<i", fd), flags)

    def inner_fds(self) -> list:
        """ARRAY_OF_MAPS: the int each slot holds (0: empty), from a snapshot."""
        return [int(x) for x in self.snapshot().view(np.int32)]

    # BPF_MAP_TYPE_PERF_EVENT_ARRAY (perf_event_array_map.cpp)
    def set_perf(self, index: int, perf, flags: int = 0) -> int:
        """PERF_EVENT_ARRAY: store the perf event `perf` (a PerfEvent or a raw
        int: the slots are untyped) in slot `index`."""
        fd = perf.fd if isinstance(perf, PerfEvent) else int(perf)
        return self.update(struct.pack("<i", index), struct.pack("<i", fd), flags)

    def perf_fds(self) -> list:
        """PERF_EVENT_ARRAY: the int each slot holds (-1: empty), from a snapshot."""
        return [int(x) for x in self.snapshot().view(np.int32)]

    # BPF_MAP_TYPE_QUEUE / _STACK / _BLOOM_FILTER (bpftime_shm.cpp:168-200)
    def push(self, value: bytes, flags: int = 0) -> int:
        v = C.create_string_buffer(bytes(value), len(value))
        return lib().bpftime_map_push_elem(self.fd, v, flags)

    def peek(self, value: bytes) -> bool:
        """True when every bit of the value is set (it may have been pushed)."""
        v = C.create_string_buffer(bytes(value), len(value))
        return lib().bpftime_map_peek_elem(self.fd, v) == 0

    def pop(self) -> int:
        v = C.create_string_buffer(max(self.value_size, 1))
        return lib().bpftime_map_pop_elem(self.fd, v)

    def pop_value(self) -> Optional[bytes]:
        """QUEUE / STACK: remove and return the oldest (queue) or newest
        (stack) element; None when the map is empty (ENOENT)."""
        v = C.create_string_buffer(max(self.value_size, 1))
        if lib().bpftime_map_pop_elem(self.fd, v) != 0:
            return None
        return v.raw[:self.value_size]

    def peek_value(self) -> Optional[bytes]:
        """QUEUE / STACK: the element pop_value would return, left in place."""
        v = C.create_string_buffer(max(self.value_size, 1))
        if lib().bpftime_map_peek_elem(self.fd, v) != 0:
            return None
        return v.raw[:self.value_size]

    def queue_items(self) -> list:
        """QUEUE / STACK: the elements from the oldest to the newest, decoded
        from a snapshot of the ring (128-byte header {u64 head, u64 tail}, then
        max_entries slots; the element with ticket t in slot t % max_entries)."""
        raw = self.snapshot()
        head, tail = (int(x) for x in raw[:16].view(np.uint64))
        stride = (self.value_size + 3) & ~3
        out = []
        for t in range(head, tail):
            at = 128 + (t % self.max_entries) * stride
            out.append(bytes(raw[at:at + self.value_size]))
        return out

    # BPF_MAP_TYPE_STACK_TRACE (stack_trace_map.cpp)
    def stack_frames(self, id: int) -> Optional[list]:
        """STACK_TRACE: the frames slot `id` holds (an empty stack is []);
        None for an empty slot or an id past the end."""
        cap = max(self.value_size // 8, 1)
        out = (C.c_uint64 * cap)()
        n = lib().bpftime_amd_stack_trace_get(self.fd, id, out, cap)
        return None if n < 0 else [int(out[i]) for i in range(min(n, cap))]

    def bloom_seed(self, set: Optional[int] = None) -> int:
        """The filter's jhash seed; `set` installs a new one first, which
        zeroes the bit array."""
        out = C.c_uint32(0)
        new = C.byref(C.c_uint32(set & 0xFFFFFFFF)) if set is not None else None
        if lib().bpftime_amd_bloom_seed(self.fd, new, C.byref(out)) < 0:
            raise EbpfError(f"fd {self.fd} is not a Bloom filter")
        return out.value

    def close(self) -> None:
        lib().bpftime_close(self.fd)


def close_fd(fd: int) -> None:
    """bpftime_close: a map, prog or link record (a closed prog leaves the
    prog arrays that name it, prog_array.cpp:127-131)."""
    lib().bpftime_close(fd)


def reset_runtime() -> None:
    lib().bpftime_amd_reset()


def set_ncpu(n: int) -> None:
    lib().bpftime_amd_set_ncpu(n)


# ---------------------------------------------------------------------------
# VM
# ---------------------------------------------------------------------------
class VM:
    def __init__(self, name: str = "mi355x", default_helpers: bool = True):
        self.h = lib().ebpf_create(name.encode())
        if not self.h:
            raise EbpfError(f"ebpf_create({name!r}) failed")
        if default_helpers:
            lib().bpftime_amd_register_default_helpers(C.c_void_p(self.h))

    def register(self, index: int, name: str) -> int:
        return lib().ebpf_register(C.c_void_p(self.h), index, name.encode(), None)

    def set_unwind(self, idx: int) -> int:
        """ebpf_set_unwind_function_index (idx = the ubpf id a helper was
        registered under: the order of registration, from 1)."""
        return lib().ebpf_set_unwind_function_index(C.c_void_p(self.h), idx)

    def load(self, code: bytes) -> None:
        err = C.c_void_p()
        buf = C.create_string_buffer(code, len(code))
        rc = lib().ebpf_load(C.c_void_p(self.h), buf, len(code), C.byref(err))
        if rc < 0:
            msg = C.string_at(err.value).decode() if err.value else "?"
            raise EbpfError(msg)

    def try_load(self, code: bytes):
        """(rc, errmsg) like ebpf_load."""
        err = C.c_void_p()
        buf = C.create_string_buffer(code, len(code))
        rc = lib().ebpf_load(C.c_void_p(self.h), buf, len(code), C.byref(err))
        return rc, (C.string_at(err.value).decode() if err.value else "")

    def unload(self) -> None:
        lib().ebpf_unload_code(C.c_void_p(self.h))

    def set_ctx_kind(self, kind: int) -> None:
        lib().ebpf_set_ctx_kind(C.c_void_p(self.h), kind)

    def exec(self, mem: bytearray) -> tuple:
        """ebpf_exec on a host buffer (copied to the GPU and back)."""
        buf = (C.c_uint8 * len(mem)).from_buffer(mem) if len(mem) else None
        ret = C.c_uint64(0)
        rc = lib().ebpf_exec(C.c_void_p(self.h), buf, len(mem), C.byref(ret))
        return rc, ret.value

    def info(self) -> dict:
        ss, big, fused, n = C.c_uint32(), C.c_int(), C.c_uint32(), C.c_uint32()
        lib().bpftime_amd_vm_info(C.c_void_p(self.h), C.byref(ss), C.byref(big), C.byref(fused), C.byref(n))
        return {"stack_size": ss.value, "big_stack": bool(big.value), "fused_rmw": fused.value,
                "n_insns": n.value}

    def fast_specialized(self, kind: int) -> int:
        n = C.c_uint32()
        if lib().bpftime_amd_vm_fast_info(C.c_void_p(self.h), kind, C.byref(n)):
            raise EbpfError("vm_fast_info failed")
        return n.value

    def fast_handler(self, kind: int, pc: int) -> Optional[str]:
        """Name of the fast-path handler chosen for instruction slot `pc`
        ("SLOW": left to the C++ tier); None past the program."""
        s = lib().bpftime_amd_vm_fast_handler(C.c_void_p(self.h), kind, pc)
        return s.decode() if s else None

    def counter_info(self, kind: int) -> tuple:
        """(deferred, direct) counter-add sites for the entry form of `kind`."""
        d, n = C.c_uint32(), C.c_uint32()
        if lib().bpftime_amd_vm_counter_info(C.c_void_p(self.h), kind, C.byref(d), C.byref(n)):
            raise EbpfError("vm_counter_info failed")
        return d.value, n.value

    def last_launch(self) -> dict:
        """The plan of this VM's last batch launch (struct
        bpftime_amd_launch_info): units, grid, block, comb_entries,
        lcache_sets, stage, miss_cap, tail_lds_depths, tail_lds_words,
        occupancy, and gregs, gctx, flush_log, miss_log, ordered as bools."""
        li = LaunchInfo()
        if lib().bpftime_amd_vm_last_launch(C.c_void_p(self.h), C.byref(li)):
            raise EbpfError("no batch launched yet")
        d = {name: getattr(li, name) for name, _ in LaunchInfo._fields_}
        for k in ("gregs", "gctx", "flush_log", "miss_log", "ordered"):
            d[k] = bool(d[k])
        return d

    def set_step_limit(self, n: int) -> None:
        lib().bpftime_amd_set_step_limit(C.c_void_p(self.h), n)

    def set_task(self, comm: Optional[bytes] = None, uid_gid: Optional[int] = None) -> None:
        """What bpf_get_current_comm / bpf_get_current_uid_gid answer in this
        VM's launches (bpftime_amd_vm_set_task); None leaves a part as it is.
        comm: at most 63 bytes."""
        if isinstance(comm, str):
            comm = comm.encode()
        u = C.c_uint64(uid_gid) if uid_gid is not None else None
        if lib().bpftime_amd_vm_set_task(C.c_void_p(self.h), comm, C.byref(u) if u is not None else None):
            raise EbpfError("set_task: comm longer than 63 bytes")

    def get_task(self) -> tuple:
        """(comm bytes up to its NUL, uid_gid)."""
        buf = C.create_string_buffer(64)
        u = C.c_uint64()
        if lib().bpftime_amd_vm_get_task(C.c_void_p(self.h), buf, C.byref(u)):
            raise EbpfError("get_task failed")
        return buf.raw.split(b"\0", 1)[0], u.value

    def set_attach(self, func_ip: int = 0, cookie: int = 0) -> None:
        """What bpf_get_func_ip / bpf_get_attach_cookie answer in this VM's
        launches (bpftime_amd_vm_set_attach); both 0 by default."""
        if lib().bpftime_amd_vm_set_attach(C.c_void_p(self.h), func_ip, cookie):
            raise EbpfError("set_attach failed")

    def last_batch_ms(self) -> float:
        """Kernel time of this VM's last BATCH_TIMED batch (ms; -1 none)."""
        return lib().bpftime_amd_last_batch_ms(self.h)

    def exec_batch(self, kind: int, data: DeviceBuffer, count: int, stride: int, fixed_len: int = 0,
                   lens: Optional[DeviceBuffer] = None, verdicts: Optional[DeviceBuffer] = None,
                   rets: Optional[DeviceBuffer] = None, data_off_out: Optional[DeviceBuffer] = None,
                   len_out: Optional[DeviceBuffer] = None, flags: int = BATCH_SYNC, first_unit: int = 0,
                   head: int = 0, data_offset: int = 0, ifindex: int = 0, rxq: int = 0,
                   stream: int = 0, descs: Optional[DeviceBuffer] = None, umem_bytes: int = 0,
                   sys_nr: Optional[int] = None, pid_tgid_off: int = 0, ktime_off: int = 0,
                   stacks: Optional[DeviceBuffer] = None, stack_unit_stride: int = 0, stack_frame_stride: int = 0,
                   stack_depths: Optional[DeviceBuffer] = None, stack_fixed_depth: int = 0,
                   stack_max_depth: int = 0, sys_state: Optional[DeviceBuffer] = None,
                   sys_ret: Optional[DeviceBuffer] = None, sys_phase: int = 0) -> int:
        """descs: AF_XDP descriptor mode ({u64 addr; u32 len; u32 options} per
        unit, frames at data + addr inside umem_bytes; stride = chunk size).
        pid_tgid_off / ktime_off: the recorded caller / clock of a syscall
        replay unit (include/ebpf-vm.h).  stacks: the units' recorded call
        stacks for bpf_get_stackid / bpf_get_stack (u64 frames; frame k of unit
        i at i * stack_unit_stride + k * stack_frame_stride), stack_depths
        (u32 per unit) or stack_fixed_depth their frame counts, stack_max_depth
        the most frames a unit may have (1..127)."""
        b = EbpfBatch(ctx_kind=kind, flags=flags, count=count, data=data.ptr + data_offset, stride=stride,
                      lens=lens.ptr if lens else None, fixed_len=fixed_len, ingress_ifindex=ifindex,
                      rx_queue_index=rxq, head=head, verdicts=verdicts.ptr if verdicts else None,
                      rets=rets.ptr if rets else None,
                      data_off_out=data_off_out.ptr if data_off_out else None,
                      len_out=len_out.ptr if len_out else None, first_unit=first_unit,
                      stream=stream or None, descs=descs.ptr if descs else None, umem_bytes=umem_bytes,
                      sys_nr=-1 if sys_nr is None else sys_nr, pid_tgid_off=pid_tgid_off,
                      ktime_off=ktime_off, stack_arr=stacks.ptr if stacks else None,
                      stack_unit_stride=stack_unit_stride, stack_frame_stride=stack_frame_stride,
                      stack_depths=stack_depths.ptr if stack_depths else None,
                      stack_fixed_depth=stack_fixed_depth, stack_max_depth=stack_max_depth,
                      sys_state=sys_state.ptr if sys_state else None, sys_ret=sys_ret.ptr if sys_ret else None,
                      sys_phase=sys_phase)
        if sys_nr is not None:
            b.flags |= BATCH_SYS_NR
        rc = lib().ebpf_exec_batch(C.c_void_p(self.h), C.byref(b))
        if rc < 0:
            e = lib().bpftime_amd_vm_error(C.c_void_p(self.h))
            raise EbpfError(f"ebpf_exec_batch failed: {e.decode() if e else '?'}")
        return rc

    def close(self) -> None:
        if self.h:
            lib().ebpf_destroy(C.c_void_p(self.h))
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


XDP_ABORTED, XDP_DROP, XDP_PASS, XDP_TX, XDP_REDIRECT = 0, 1, 2, 3, 4
XDP_COMPLETE_SYNC = 0x1
XDP_FRAME_MASK_DEFAULT = (1 << XDP_PASS) | (1 << XDP_TX) | (1 << XDP_REDIRECT)


def xdp_complete_tile() -> int:
    """Units per workgroup tile of the completion kernels."""
    return lib().bpftime_amd_xdp_complete_tile()


def xdp_complete_scan_tiles() -> int:
    """Tiles per pass of the completion's tile-offset scan."""
    return lib().bpftime_amd_xdp_complete_scan_tiles()


def xdp_complete(count: int, verdicts: Optional[DeviceBuffer], stride: int, umem_bytes: int,
                 descs: Optional[DeviceBuffer] = None, data_off_out: Optional[DeviceBuffer] = None,
                 len_out: Optional[DeviceBuffer] = None, umem: Optional[DeviceBuffer] = None, out=None,
                 index_out=None, cap=None, frame_mask: int = XDP_FRAME_MASK_DEFAULT,
                 counts: Optional[DeviceBuffer] = None, gather=None, gather_stride: int = 0, gather_cap: int = 0,
                 gather_mask: int = 0, gather_descs: Optional[DeviceBuffer] = None,
                 gather_index: Optional[DeviceBuffer] = None, gather_count: Optional[DeviceBuffer] = None,
                 gather_skipped: Optional[DeviceBuffer] = None, stream: int = 0, sync: bool = True):
    """bpftime_amd_xdp_complete after an EBPF_CTX_XDP batch on the same
    stream: per verdict class (XDP_ABORTED .. XDP_REDIRECT) a descriptor list
    in unit order.  out / index_out: five DeviceBuffers or None each ({u64
    addr, u32 len, u32 options} entries / u32 unit indices), cap: five entry
    counts.  The classes in frame_mask get their frames as the program left
    them, the others the chunk to hand back to the FILL ring.  gather: a
    DeviceBuffer or a pinned-host address that receives the frames of the
    classes in gather_mask, packed gather_stride apart in unit order.
    Returns, when sync, the five totals (not clamped to cap) -- with a gather,
    (totals, gathered, skipped); without sync None (read `counts`)."""
    p = lambda b: (b.ptr if hasattr(b, "ptr") else int(b)) if b else None  # noqa: E731
    a = XdpCompleteArgs(struct_size=C.sizeof(XdpCompleteArgs), flags=XDP_COMPLETE_SYNC if sync else 0, count=count,
                        verdicts=p(verdicts), descs=p(descs), data_off_out=p(data_off_out), len_out=p(len_out),
                        umem=p(umem), stride=stride, umem_bytes=umem_bytes, stream=stream or None,
                        frame_mask=frame_mask, gather_mask=gather_mask, counts=p(counts), gather=p(gather),
                        gather_stride=gather_stride, gather_cap=gather_cap, gather_descs=p(gather_descs),
                        gather_index=p(gather_index), gather_count=p(gather_count),
                        gather_skipped=p(gather_skipped))
    for c in range(5):
        a.out[c] = p(out[c]) if out else None
        a.index_out[c] = p(index_out[c]) if index_out else None
        a.cap[c] = cap[c] if cap else 0
    host = (C.c_uint32 * 5)()
    host_g = (C.c_uint32 * 2)()
    if sync:
        a.host_counts = C.cast(host, C.POINTER(C.c_uint32))
        a.host_gather = C.cast(host_g, C.POINTER(C.c_uint32))
    if lib().bpftime_amd_xdp_complete(C.byref(a)) < 0:
        raise EbpfError(_err())
    if not sync:
        return None
    totals = [int(x) for x in host]
    return (totals, int(host_g[0]), int(host_g[1])) if gather else totals


def enable_trace_printk(on: bool = True) -> bool:
    """bpf_trace_printk on the device (bpftime_amd_enable_trace_printk): off
    by default and after reset_runtime; VMs created while it is on have the
    helper.  Returns the previous setting."""
    return bool(lib().bpftime_amd_enable_trace_printk(1 if on else 0))


def trace_read(max_lines: int = 1 << 16, text_cap: int = 1 << 22):
    """bpf_trace_printk's lines since the last read (bpftime_amd_trace_read):
    ([(unit, line bytes)] in ticket order, records lost to a full log).  None
    when no program that calls the helper was loaded yet (no log)."""
    lines = (TraceLine * max(max_lines, 1))()
    text = C.create_string_buffer(max(text_cap, 1))
    lost = C.c_uint64(0)
    n = lib().bpftime_amd_trace_read(lines, max_lines, text, text_cap, C.byref(lost))
    if n < 0:
        return None
    raw = text.raw
    return [(lines[i].unit, raw[lines[i].text_off:lines[i].text_off + lines[i].text_len]) for i in range(n)], lost.value


# ---------------------------------------------------------------------------
# prog / link records (the bpf_link attach surface)
# ---------------------------------------------------------------------------
def prog_create(code: bytes, name: str, prog_type: int, fd: int = -1) -> int:
    buf = C.create_string_buffer(code, len(code))
    r = lib().bpftime_progs_create(fd, buf, len(code) // 8, name.encode(), prog_type)
    if r < 0:
        raise EbpfError("prog create failed")
    return r


def link_create(prog_fd: int, target: int, attach_type: int, fd: int = -1, cookie: int = 0) -> int:
    """cookie: perf_event.bpf_cookie, read for attach type 41 only."""
    a = BpfLinkCreateArgs(prog_fd=prog_fd, target_fd=target, attach_type=attach_type)
    a.attach_union[0] = cookie
    return lib().bpftime_link_create(fd, C.byref(a))


def uprobe_attach(prog_fd: int, func: int, kind: int = UPROBE, cookie: Optional[int] = None) -> int:
    """A program at function address `func` of the recorded calls: UPROBE,
    URETPROBE, UPROBE_OVERRIDE or UREPLACE; the attach id."""
    c = C.c_uint64(cookie) if cookie is not None else None
    i = lib().bpftime_amd_uprobe_attach(prog_fd, func, kind, C.byref(c) if c is not None else None)
    if i < 0:
        raise EbpfError(f"uprobe attach failed (errno {C.get_errno()}): {_err()}")
    return i


def uprobe_attach_link(link_fd: int, func: int) -> int:
    """Binds a link to a uprobe perf event to the address its module:offset
    resolved to; kind and cookie come from the records."""
    i = lib().bpftime_amd_uprobe_attach_link(link_fd, func)
    if i < 0:
        raise EbpfError(f"uprobe attach failed (errno {C.get_errno()}): {_err()}")
    return i


def uprobe_detach(i: int) -> int:
    return lib().bpftime_amd_uprobe_detach(i)


def uprobe_dispatch(func: Optional[DeviceBuffer], n: int, enter: Optional[DeviceBuffer] = None,
                    leave: Optional[DeviceBuffer] = None, pid_tgid: Optional[DeviceBuffer] = None,
                    clock: Optional[DeviceBuffer] = None, out_state: Optional[DeviceBuffer] = None,
                    out_rets: Optional[DeviceBuffer] = None, flags: int = BATCH_SYNC, stream: int = 0,
                    stacks: Optional[DeviceBuffer] = None, stack_unit_stride: int = 0, stack_frame_stride: int = 0,
                    stack_depths: Optional[DeviceBuffer] = None, stack_fixed_depth: int = 0,
                    stack_max_depth: int = 0) -> int:
    """Runs the uprobe attachments over n recorded calls (struct
    bpftime_amd_call_records): func (u64 per call), enter / leave (168-B
    pt_regs per call), pid_tgid (u64), clock (2 x u64), the stacks as
    exec_batch's; out_state (u32) / out_rets (i64) receive the overrides.
    flags: BATCH_* and the plan -- program-major by default and with
    DISPATCH_PROGRAMS (a pair that may not commute is refused), thread-ordered
    with DISPATCH_THREADS (| BATCH_ORDERED: one lane, the serial run); both
    plan flags are an error (uprobe_dispatch_plan).
    Returns the failed callbacks (BATCH_SYNC)."""
    p = lambda b: b.ptr if b else None  # noqa: E731
    r = CallRecords(enter=p(enter), leave=p(leave), func=p(func), pid_tgid=p(pid_tgid), clock=p(clock),
                    stack_arr=p(stacks), stack_unit_stride=stack_unit_stride,
                    stack_frame_stride=stack_frame_stride, stack_depths=p(stack_depths),
                    stack_fixed_depth=stack_fixed_depth, stack_max_depth=stack_max_depth, count=n)
    rc = lib().bpftime_amd_uprobe_dispatch(C.byref(r), p(out_state), p(out_rets), flags, stream or None)
    if rc < 0:
        raise EbpfError(f"uprobe dispatch failed: {_err()}")
    return rc


def call_event(record: int, phase: int) -> int:
    """BPFTIME_AMD_CALL_EVENT: the event word of a record's entry (phase 0) or
    return (phase 1)."""
    return ((record << 1) | (phase & 1)) & 0xFFFFFFFF


def uprobe_dispatch_events(func: Optional[DeviceBuffer], n: int, events: Optional[DeviceBuffer], n_events: int,
                           enter: Optional[DeviceBuffer] = None, leave: Optional[DeviceBuffer] = None,
                           pid_tgid: Optional[DeviceBuffer] = None, clock: Optional[DeviceBuffer] = None,
                           out_state: Optional[DeviceBuffer] = None, out_rets: Optional[DeviceBuffer] = None,
                           flags: int = BATCH_SYNC | DISPATCH_THREADS, stream: int = 0) -> int:
    """The thread-ordered uprobe replay over an event list
    (bpftime_amd_uprobe_dispatch_events): n records as uprobe_dispatch's, and
    n_events u32 words call_event(record, phase) in recorded order, so nested
    and recursive calls run entry, inner entry, inner return, return.  flags
    must carry DISPATCH_THREADS (| BATCH_ORDERED: one lane, the serial run).
    Returns the failed callbacks (BATCH_SYNC)."""
    p = lambda b: b.ptr if b else None  # noqa: E731
    r = CallRecords(enter=p(enter), leave=p(leave), func=p(func), pid_tgid=p(pid_tgid), clock=p(clock), count=n)
    rc = lib().bpftime_amd_uprobe_dispatch_events(C.byref(r), p(events), n_events, p(out_state), p(out_rets), flags,
                                                  stream or None)
    if rc < 0:
        raise EbpfError(f"uprobe dispatch failed: {_err()}")
    return rc


def uprobe_dispatch_plan(flags: int = 0) -> int:
    """1 when a uprobe dispatch with these flags runs thread-ordered for the
    current attachments, 0 program-major; raises with the named error such a
    dispatch would give."""
    rc = lib().bpftime_amd_uprobe_dispatch_plan(flags)
    if rc < 0:
        raise EbpfError(f"uprobe dispatch plan failed: {_err()}")
    return rc


def last_seq_tier() -> int:
    """The tier that ran the callbacks of this host thread's most recent
    thread-ordered dispatch, syscall or uprobe (bpftime_amd_last_seq_tier): 1
    the asm tier, 0 the C++ tier, -1 before any.  Diagnostic."""
    return lib().bpftime_amd_last_seq_tier()


def group_threads(keys: Optional[DeviceBuffer], n: int, stride: int = 8, offset: int = 0):
    """bpftime_amd_group_threads (csrc/group.hip) on the null stream: the
    grouping both thread-ordered dispatches stand on.  Record i's u64 key
    (its pid_tgid) lies at keys + offset + i * stride.  Returns (perm, seg,
    nseg): perm[0:n] the record indices sorted by key, a key's records in
    record order; seg[0:nseg + 1] the start of each key's run in perm, with
    seg[nseg] = n.  Invalid input (n == 0, no keys, stride % 8) raises with
    the hipError_t."""
    if keys is not None and n and stride > 0 and offset + (n - 1) * stride + 8 > keys.nbytes:
        raise ValueError(f"{n} keys at stride {stride} + {offset} do not fit {keys.nbytes} bytes")
    scratch = DeviceBuffer(max(lib().bpftime_amd_group_scratch_bytes(n), 256))
    perm, seg, nseg = C.c_void_p(), C.c_void_p(), C.c_uint64(0)
    e = lib().bpftime_amd_group_threads(C.c_void_p(keys.ptr + offset) if keys is not None else None, stride, n,
                                        C.c_void_p(scratch.ptr), C.byref(perm), C.byref(seg), C.byref(nseg), None)
    if e:
        raise EbpfError(f"group_threads failed: hipError_t {e}")
    if not 0 < nseg.value <= n:
        raise EbpfError(f"group_threads: {nseg.value} segments over {n} records")
    return (scratch.download(np.uint32, n, perm.value - scratch.ptr),
            scratch.download(np.uint32, nseg.value + 1, seg.value - scratch.ptr), nseg.value)


def syscall_attach(prog_fd: int, sys_nr: int, enter: bool = True) -> int:
    """A program on the sys_enter / sys_exit tracepoint of sys_nr (-1: every
    syscall; syscall_trace_attach_impl.cpp:121-166): the attach id."""
    i = lib().bpftime_amd_syscall_attach_ex(prog_fd, sys_nr, 1 if enter else 0)
    if i < 0:
        raise EbpfError(f"syscall attach failed: {_err()}")
    return i


def syscall_detach(i: int) -> int:
    return lib().bpftime_amd_syscall_detach(i)


def syscall_dispatch(records: DeviceBuffer, n: int, record_size: int = SYSCALL_RECORD_FULL,
                     out: Optional[DeviceBuffer] = None, flags: int = BATCH_SYNC, stream: int = 0) -> int:
    """dispatch_syscall over n recorded calls (64-B enter, 96-B enter + exit
    + caller, or 128-B records with the recorded clocks too); out (i64 per
    record) receives what each call returns.  flags: BATCH_* and the plan
    (DISPATCH_THREADS / DISPATCH_PROGRAMS; default: chosen from the attached
    programs' map effects, syscall_dispatch_plan)."""
    rc = lib().bpftime_amd_syscall_dispatch_records(records.ptr, n, record_size, out.ptr if out else None,
                                                     flags, stream or None)
    if rc < 0:
        raise EbpfError(f"syscall dispatch failed: {_err()}")
    return rc


def syscall_dispatch_soa(exit: Optional[DeviceBuffer], n: int, enter: Optional[DeviceBuffer] = None,
                         clock: Optional[DeviceBuffer] = None, out: Optional[DeviceBuffer] = None,
                         flags: int = BATCH_SYNC, stream: int = 0) -> int:
    """dispatch_syscall over n recorded calls in struct-of-arrays form
    (include/bpftime_amd.h struct bpftime_amd_sys_records): exit (n x 32 B
    {exit ctx, pid_tgid}), enter (n x 64 B, optional), clock (n x 16 B,
    optional)."""
    r = SysRecords(enter=enter.ptr if enter else None, exit=exit.ptr if exit else None,
                   clock=clock.ptr if clock else None, count=n)
    rc = lib().bpftime_amd_syscall_dispatch_soa(C.byref(r), out.ptr if out else None, flags, stream or None)
    if rc < 0:
        raise EbpfError(f"syscall dispatch failed: {_err()}")
    return rc


def syscall_dispatch_plan(flags: int = 0) -> int:
    """1 when a dispatch with these flags runs thread-ordered for the
    current attachments, 0 program-major."""
    rc = lib().bpftime_amd_syscall_dispatch_plan(flags)
    if rc < 0:
        raise EbpfError(f"syscall dispatch plan failed: {_err()}")
    return rc


def xdp_links() -> list:
    n = lib().bpftime_amd_xdp_links(None, None, None, 0)
    lf, pf, ifx = (C.c_int * max(n, 1))(), (C.c_int * max(n, 1))(), (C.c_uint32 * max(n, 1))()
    lib().bpftime_amd_xdp_links(lf, pf, ifx, n)
    return [(lf[i], pf[i], ifx[i]) for i in range(n)]


def hip_runtime() -> dict:
    """The HIP runtime this process's library runs on: hipRuntimeGetVersion
    and the libamdhip64 file mapped into the process (torch bundles its own
    with the same SONAME)."""
    ver = lib().bpftime_amd_hip_runtime_version()
    libs = set()
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                p = line.split()[-1]
                if "libamdhip64" in p:
                    libs.add(p)
    except OSError:
        pass
    return {"version": ver, "lib": sorted(libs)}


def prog_instantiate(prog_fd: int) -> VM:
    err = C.c_void_p()
    h = lib().bpftime_amd_prog_instantiate(prog_fd, C.byref(err))
    if not h:
        raise EbpfError(C.string_at(err.value).decode() if err.value else "instantiate failed")
    vm = VM.__new__(VM)
    vm.h = h
    return vm


class Event:
    def __init__(self):
        self.h = lib().bpftime_amd_event_create()

    def record(self, stream: int = 0) -> None:
        lib().bpftime_amd_event_record(C.c_void_p(self.h), C.c_void_p(stream) if stream else None)

    def elapsed_ms(self, later: "Event") -> float:
        return lib().bpftime_amd_event_elapsed_ms(C.c_void_p(self.h), C.c_void_p(later.h))

    def __del__(self):
        try:
            lib().bpftime_amd_event_destroy(C.c_void_p(self.h))
        except Exception:
            pass


# ---- bpf(2) commands (syscall_context.cpp:429-668) --------------------------
BPF_MAP_CREATE, BPF_MAP_LOOKUP_ELEM, BPF_MAP_UPDATE_ELEM, BPF_MAP_DELETE_ELEM = 0, 1, 2, 3
BPF_MAP_GET_NEXT_KEY, BPF_PROG_LOAD, BPF_MAP_FREEZE, BPF_LINK_CREATE = 4, 5, 22, 28
BPF_MAP_LOOKUP_BATCH, BPF_MAP_LOOKUP_AND_DELETE_BATCH = 24, 25


def sys_bpf(cmd: int, attr: bytearray) -> tuple:
    """bpftime_amd_handle_sysbpf over a union bpf_attr image; (ret, errno)."""
    buf = (C.c_char * len(attr)).from_buffer(attr)
    C.set_errno(0)
    r = lib().bpftime_amd_handle_sysbpf(cmd, C.addressof(buf), len(attr))
    return r, C.get_errno()


def attr_map_create(type_: int, key_size: int, value_size: int, max_entries: int, flags: int = 0,
                    name: str = "") -> bytearray:
    a = bytearray(128)
    struct.pack_into("<IIIII", a, 0, type_, key_size, value_size, max_entries, flags)
    nm = name.encode()[:15]
    a[28:28 + len(nm)] = nm
    return a


def attr_map_elem(fd: int, key_addr: int, value_addr: int = 0, flags: int = 0) -> bytearray:
    a = bytearray(128)
    struct.pack_into("<IIQQQ", a, 0, fd, 0, key_addr, value_addr, flags)
    return a


def attr_map_batch(fd: int, in_batch_addr: int, out_batch_addr: int, keys_addr: int, values_addr: int, count: int,
                   elem_flags: int = 0, flags: int = 0) -> bytearray:
    """union bpf_attr's `batch` member (BPF_MAP_LOOKUP_BATCH and its kin):
    in_batch_addr 0 starts at the beginning; the handler writes the number of
    entries returned back over count (batch_count reads it)."""
    a = bytearray(128)
    struct.pack_into("<QQQQIIQQ", a, 0, in_batch_addr, out_batch_addr, keys_addr, values_addr, count, fd,
                     elem_flags, flags)
    return a


def batch_count(attr: bytearray) -> int:
    """attr->batch.count of an attr_map_batch image."""
    return struct.unpack_from("<I", attr, 32)[0]


def attr_prog_load(prog_type: int, insns_addr: int, insn_cnt: int, name: str = "") -> bytearray:
    a = bytearray(128)
    struct.pack_into("<IIQ", a, 0, prog_type, insn_cnt, insns_addr)
    nm = name.encode()[:15]
    a[48:48 + len(nm)] = nm
    return a


def attr_link_create(prog_fd: int, target: int, attach_type: int, flags: int = 0) -> bytearray:
    a = bytearray(128)
    struct.pack_into("<IIII", a, 0, prog_fd, target, attach_type, flags)
    return a
