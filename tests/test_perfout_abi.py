"""PERF_EVENT_ARRAY and software perf event ring surface.  The first tests need
no GPU: the operations table has the family, the entry points exist and the
loader no longer refuses helper 25.  Creating a map or a ring needs the device,
so every test that creates one is marked `gpu`."""
import ctypes as C
import errno
import json
import struct

import pytest

from bpftime_amd import _lib, isa
from bpftime_amd.isa import Asm
from bpftime_amd.vm import VM, Map, PerfEvent

import _perfout as pm

PEA = isa.BPF_MAP_TYPE_PERF_EVENT_ARRAY
i32 = lambda v: struct.pack("<i", v)  # noqa: E731


def test_ids():
    assert PEA == 4 and isa.BPF_FUNC_perf_event_output == 25


def test_python_surface():
    for name in ("bpftime_amd_perf_event_mmap", "bpftime_amd_perf_event_fetch", "bpftime_amd_perf_event_ring_state"):
        assert hasattr(_lib.lib(), name)
    for name in ("set_perf", "perf_fds"):
        assert callable(getattr(Map, name)), name
    for name in ("mmap", "state", "fetch", "fetch_raw"):
        assert callable(getattr(PerfEvent, name)), name


def test_helper_25_is_not_refused_by_the_loader():
    # (without a device the load ends at the upload; the parent refused the call by name)
    vm = VM()
    rc, msg = vm.try_load(pm.emit_prog(3, size=8))
    assert "no device implementation" not in (msg or "") and "nonexistent function" not in (msg or "")


@pytest.mark.gpu
def test_helper_25_loads(fresh_runtime):
    dev = fresh_runtime
    m = dev.Map(PEA, 4, 4, 4)
    vm = dev.VM()
    assert vm.try_load(pm.emit_prog(m.fd))[0] == 0 and vm.info()["big_stack"]


@pytest.mark.gpu
def test_create(fresh_runtime):
    dev = fresh_runtime
    for ks, vs in ((8, 4), (4, 8), (0, 4), (4, 0)):
        C.set_errno(0)
        a = _lib.BpfMapAttr(type=PEA, key_size=ks, value_size=vs, max_ents=4)
        assert _lib.lib().bpftime_maps_create(-1, b"bad", a) == -1 and C.get_errno() == errno.EINVAL
        assert b"must be 4" in _lib.lib().bpftime_amd_last_error()
    m = dev.Map(PEA, 4, 4, 5, name="events")
    assert m.storage_bytes() == 20 and m.perf_fds() == [-1] * 5
    assert dev.Map(PEA, 4, 4, 0).storage_bytes() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("mx", [1, 4, 65])
def test_host_ops_against_the_model(fresh_runtime, mx):
    dev = fresh_runtime
    m, model = dev.Map(PEA, 4, 4, mx), pm.PerfArray(mx)

    def both(op, *args):
        C.set_errno(0)
        model.err = 0
        got, want = getattr(m, op)(*args), getattr(model, op)(*args)
        assert got == want and (not model.err or C.get_errno() == model.err), (op, args, got, want)
        assert bytes(m.snapshot()) == model.image() and m.perf_fds() == model.slots
        return got

    assert both("update", i32(0), i32(7)) == 0 and both("update", i32(mx - 1), i32(-5), 1) == 0
    assert both("update", i32(0), i32(2 ** 31 - 1), 2) == 0 and both("update", i32(0), i32(9), 12345) == 0
    for k in (mx, -1, mx + 7, -2 ** 31):
        assert both("update", i32(k), i32(1)) == -1 and C.get_errno() == errno.EINVAL
        assert both("lookup", i32(k)) is None and C.get_errno() == errno.EINVAL
        assert both("delete", i32(k)) == -1 and C.get_errno() == errno.EINVAL
    assert both("lookup", i32(0)) == i32(9) and both("delete", i32(0)) == 0 and both("lookup", i32(0)) == i32(-1)
    for k in (None, 0, mx - 1, mx, -1, 2 ** 31 - 1):
        both("next_key", None if k is None else i32(k))
    buf = C.create_string_buffer(8)
    assert m.push(b"\0" * 4) == -95 and m.pop() == -95 and _lib.lib().bpftime_map_peek_elem(m.fd, buf) == -95


@pytest.mark.gpu
def test_sys_bpf_commands(fresh_runtime):
    dev = fresh_runtime
    fd, _ = dev.sys_bpf(0, dev.attr_map_create(PEA, 4, 4, 3, name="events"))
    assert fd >= 0 and dev.Map.from_fd(fd).type == PEA
    assert dev.sys_bpf(0, dev.attr_map_create(PEA, 4, 8, 3)) == (-1, errno.EINVAL)
    k, v, nk = C.create_string_buffer(i32(1), 4), C.create_string_buffer(i32(44), 4), C.create_string_buffer(4)
    out = C.create_string_buffer(4)
    assert dev.sys_bpf(2, dev.attr_map_elem(fd, C.addressof(k), C.addressof(v), 1))[0] == 0   # flags ignored
    assert dev.sys_bpf(1, dev.attr_map_elem(fd, C.addressof(k), C.addressof(out)))[0] == 0 and out.raw == i32(44)
    big = C.create_string_buffer(i32(3), 4)
    # (BPF_MAP_LOOKUP_ELEM reports every NULL as ENOENT, for every map type)
    assert dev.sys_bpf(1, dev.attr_map_elem(fd, C.addressof(big), C.addressof(out))) == (-1, errno.ENOENT)
    assert dev.sys_bpf(2, dev.attr_map_elem(fd, C.addressof(big), C.addressof(v))) == (-1, errno.EINVAL)
    assert dev.sys_bpf(4, dev.attr_map_elem(fd, C.addressof(k), C.addressof(nk)))[0] == 0 and nk.raw == i32(2)
    last = C.create_string_buffer(i32(2), 4)
    assert dev.sys_bpf(4, dev.attr_map_elem(fd, C.addressof(last), C.addressof(nk))) == (-1, errno.ENOENT)
    assert dev.sys_bpf(3, dev.attr_map_elem(fd, C.addressof(k)))[0] == 0
    assert dev.Map.from_fd(fd).perf_fds() == [-1, -1, -1]


@pytest.mark.gpu
def test_mmap_rules(fresh_runtime):
    dev = fresh_runtime
    L = _lib.lib()
    e = dev.PerfEvent()
    assert e.state() == (0, 0, 0) and e.fetch_raw() == (0, b"")
    for bad in (0, 32, 96, 1000, (1 << 20) + 8):
        C.set_errno(0)
        assert L.bpftime_amd_perf_event_mmap(e.fd, bad) == -1 and C.get_errno() == errno.EINVAL
    assert L.bpftime_amd_perf_event_mmap(e.fd, 4096) == 0 and e.state() == (0, 0, 4096)
    assert L.bpftime_amd_perf_event_mmap(e.fd, 4096) == 0                     # the same size: nothing to do
    C.set_errno(0)
    assert L.bpftime_amd_perf_event_mmap(e.fd, 8192) == -1 and C.get_errno() == errno.EINVAL
    assert b"cannot be resized" in L.bpftime_amd_last_error()
    tp = L.bpftime_tracepoint_create(-1, -1, 5)
    m = dev.Map(PEA, 4, 4, 1)
    for fd in (tp, m.fd, 999, -1):
        C.set_errno(0)
        assert L.bpftime_amd_perf_event_mmap(fd, 4096) == -1 and C.get_errno() == errno.EINVAL
        assert L.bpftime_amd_perf_event_ring_state(fd, None, None, None) == -1
        assert L.bpftime_amd_perf_event_fetch(fd, None, 0, None) == -1
    fd = e.fd
    e.close()                                                                  # the ring goes with the fd
    assert L.bpftime_amd_perf_event_ring_state(fd, None, None, None) == -1
    again = dev.PerfEvent(fd=fd)
    assert again.fd == fd and again.state() == (0, 0, 0)
    again.mmap(64)
    dev.reset_runtime()
    assert L.bpftime_amd_perf_event_ring_state(fd, None, None, None) == -1


@pytest.mark.gpu
def test_shm_json_roundtrip(fresh_runtime, tmp_path):
    dev = fresh_runtime
    e = dev.PerfEvent(cpu=2)
    m = dev.Map(PEA, 4, 4, 6, name="events")
    assert m.set_perf(2, e) == 0 and m.set_perf(5, 77) == 0
    path = str(tmp_path / "shm.json").encode()
    assert _lib.lib().bpftime_export_global_shm_to_json(path) == 0
    h = json.load(open(path))
    assert h[str(m.fd)]["type"] == "bpf_map_handler" and h[str(m.fd)]["attr"]["map_type"] == PEA
    assert h[str(e.fd)]["type"] == "bpf_perf_event_handler" and h[str(e.fd)]["attr"]["type"] == 1
    fd, efd = m.fd, e.fd
    dev.reset_runtime()
    assert _lib.lib().bpftime_import_global_shm_from_json(path) == 0
    r = dev.Map.from_fd(fd)
    assert (r.type, r.key_size, r.value_size, r.max_entries) == (PEA, 4, 4, 6)
    assert r.perf_fds() == [-1, -1, efd, -1, -1, 77] and r.lookup(i32(2)) == i32(efd)
    assert _lib.lib().bpftime_is_perf_event_fd(efd) == 1
    snap = r.snapshot()
    assert r.delete(i32(2)) == 0
    r.restore(snap)                                                            # the arena and the host mirror
    assert r.perf_fds()[2] == efd and r.lookup(i32(2)) == i32(efd)
