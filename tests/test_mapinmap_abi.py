"""ARRAY_OF_MAPS surface.  The first two tests need no GPU: the operations
table has the family and the Python entry points exist.  Creating a map needs
the device, so every test that creates one is marked `gpu`: creation, the host
operations against the model (tests/_mapinmap.py), the bpf(2) commands, the
shm JSON round trip, snapshot / restore, reset, and closing an inner map that
a slot still names."""
import ctypes as C
import errno
import json
import struct

import numpy as np
import pytest

from bpftime_amd import _lib, isa
from bpftime_amd.vm import Map

import _mapinmap as mm

AOM, ARRAY, HASH = isa.BPF_MAP_TYPE_ARRAY_OF_MAPS, isa.BPF_MAP_TYPE_ARRAY, isa.BPF_MAP_TYPE_HASH
u32 = lambda v: struct.pack("<I", v)  # noqa: E731
i32 = lambda v: struct.pack("<i", v)  # noqa: E731


def test_map_ops_has_the_family():
    assert AOM == 12
    assert _lib.lib().bpftime_amd_map_type_supported(12) == 1
    assert _lib.lib().bpftime_amd_map_type_supported(13) == 0  # HASH_OF_MAPS: not in the reference either


def test_python_surface():
    for name in ("set_inner", "inner_fds"):
        assert callable(getattr(Map, name)), name


def same(m, model):
    np.testing.assert_array_equal(m.snapshot(), model.image())
    assert m.inner_fds() == model.slots


@pytest.mark.gpu
def test_create(fresh_runtime):
    dev = fresh_runtime
    # the attr's value_size does not size the map: sizeof(int) per slot
    for vs in (4, 0, 8, 1):
        m = dev.Map(AOM, 4, vs, 5, name="outer")
        assert m.fd >= 0 and m.storage_bytes() == 20 and not m.snapshot().any()
        a = _lib.BpfMapAttr()
        assert _lib.lib().bpftime_map_get_info(m.fd, C.byref(a), None, None) == 0
        assert (a.type, a.key_size, a.value_size, a.max_ents) == (AOM, 4, vs, 5)
    assert dev.Map(AOM, 4, 4, 0).storage_bytes() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("mx", [1, 4, 65])
def test_host_ops_against_the_model(fresh_runtime, mx):
    dev = fresh_runtime
    L = _lib.lib()
    m, model = dev.Map(AOM, 4, 4, mx), mm.Outer(mx)

    def upd(k, v, flags=0):
        C.set_errno(0)
        rc = m.update(u32(k), i32(v), flags)
        assert rc == model.update(u32(k), i32(v), flags)
        assert rc == 0 or C.get_errno() == model.err
        same(m, model)
        return rc

    assert upd(0, 7) == 0 and upd(mx - 1, -1) == 0 and upd(0, 2 ** 31 - 1, 2) == 0
    assert upd(0, 9, 1) == -1 and C.get_errno() == errno.EEXIST
    assert upd(mx, 9) == -1 and C.get_errno() == errno.E2BIG
    assert upd(mx, 9, 1) == -1 and C.get_errno() == errno.E2BIG
    assert upd(0xFFFFFFFF, 9) == -1 and C.get_errno() == errno.E2BIG
    assert upd(0, 9, 3) == -1 and C.get_errno() == errno.EINVAL
    assert upd(0, 123456789) == 0  # any int: not validated against the fd table
    assert upd(0, 5, (1 << 32) | 1) == 0
    for k in (0, mx - 1):
        assert m.lookup(u32(k)) == model.lookup(u32(k))
    # out of range: NULL / ENOENT (not the reference's null dereference)
    for k in (mx, mx + 1, 0xFFFFFFFF):
        C.set_errno(0)
        assert m.lookup(u32(k)) is None and model.lookup(u32(k)) is None and C.get_errno() == errno.ENOENT
    C.set_errno(0)
    assert m.delete(u32(0)) == model.delete(u32(0)) == -1 and C.get_errno() == errno.EINVAL
    same(m, model)
    for k in (None, 0, mx - 1, mx, 0xFFFFFFFF):
        C.set_errno(0)
        kb = None if k is None else u32(k)
        want = model.next_key(kb)
        assert m.next_key(kb) == want
        assert want is not None or C.get_errno() == errno.ENOENT
    buf = C.create_string_buffer(8)
    assert m.push(b"\0" * 4) == -95 and m.pop() == -95 and L.bpftime_map_peek_elem(m.fd, buf) == -95
    same(m, model)


@pytest.mark.gpu
def test_sys_bpf_commands(fresh_runtime):
    dev = fresh_runtime
    # BPF_MAP_CREATE (0); inner_map_fd (attr offset 20) is ignored
    a = dev.attr_map_create(AOM, 4, 4, 3, name="tenants")
    struct.pack_into("<I", a, 20, 777)
    fd, _ = dev.sys_bpf(0, a)
    assert fd >= 0 and dev.Map.from_fd(fd).type == AOM
    model = mm.Outer(3)
    inner = dev.Map(ARRAY, 4, 8, 2)
    k, v, nk = C.create_string_buffer(u32(1), 4), C.create_string_buffer(i32(inner.fd), 4), C.create_string_buffer(4)
    assert dev.sys_bpf(2, dev.attr_map_elem(fd, C.addressof(k), C.addressof(v)))[0] == 0  # UPDATE_ELEM
    assert dev.sys_bpf(2, dev.attr_map_elem(fd, C.addressof(k), C.addressof(v), 1)) == (-1, errno.EEXIST)
    out = C.create_string_buffer(4)
    assert dev.sys_bpf(1, dev.attr_map_elem(fd, C.addressof(k), C.addressof(out)))[0] == 0  # LOOKUP_ELEM
    assert out.raw == i32(inner.fd)
    big = C.create_string_buffer(u32(3), 4)
    assert dev.sys_bpf(1, dev.attr_map_elem(fd, C.addressof(big), C.addressof(out))) == (-1, errno.ENOENT)
    assert dev.sys_bpf(2, dev.attr_map_elem(fd, C.addressof(big), C.addressof(v))) == (-1, errno.E2BIG)
    assert dev.sys_bpf(3, dev.attr_map_elem(fd, C.addressof(k))) == (-1, errno.EINVAL)  # DELETE_ELEM
    assert dev.sys_bpf(4, dev.attr_map_elem(fd, C.addressof(k), C.addressof(nk)))[0] == 0  # GET_NEXT_KEY
    assert nk.raw == model.next_key(u32(1))
    last = C.create_string_buffer(u32(2), 4)
    assert dev.sys_bpf(4, dev.attr_map_elem(fd, C.addressof(last), C.addressof(nk))) == (-1, errno.ENOENT)
    assert dev.sys_bpf(21, dev.attr_map_elem(fd, 0, C.addressof(out)))[0] == -errno.ENOTSUP  # LOOKUP_AND_DELETE
    assert dev.Map.from_fd(fd).inner_fds() == [0, inner.fd, 0]


@pytest.mark.gpu
def test_shm_json_roundtrip(fresh_runtime, tmp_path):
    dev = fresh_runtime
    m = dev.Map(AOM, 4, 4, 6, name="outer")
    m.set_inner(2, 9)
    path = str(tmp_path / "shm.json").encode()
    assert _lib.lib().bpftime_export_global_shm_to_json(path) == 0
    h = json.load(open(path))[str(m.fd)]
    assert h["type"] == "bpf_map_handler" and h["attr"]["map_type"] == AOM and h["attr"]["max_entries"] == 6
    fd = m.fd
    dev.reset_runtime()
    assert _lib.lib().bpftime_import_global_shm_from_json(path) == 0
    r = dev.Map.from_fd(fd)
    assert (r.type, r.key_size, r.value_size, r.max_entries) == (AOM, 4, 4, 6)
    assert r.inner_fds() == [0] * 6  # contents are not exported
    assert r.set_inner(5, 3) == 0 and r.inner_fds()[5] == 3


@pytest.mark.gpu
def test_snapshot_restore_reset_close(fresh_runtime):
    dev = fresh_runtime
    outer, inner = dev.Map(AOM, 4, 4, 4), dev.Map(ARRAY, 4, 8, 2)
    assert outer.set_inner(1, inner) == 0 and outer.set_inner(3, -5) == 0
    # the lddw helpers: the map "pointer" is the fd; a map-value lddw sees slot 0's id
    L = _lib.lib()
    assert L.bpftime_amd_map_ptr_by_fd(outer.fd) == outer.fd and L.bpftime_amd_map_val(outer.fd) == 0
    assert outer.set_inner(0, 6) == 0 and L.bpftime_amd_map_val(outer.fd) == 6 and outer.set_inner(0, 0) == 0
    snap = outer.snapshot()
    assert bytes(snap) == i32(0) + i32(inner.fd) + i32(0) + i32(-5)
    assert outer.set_inner(1, 0) == 0 and outer.set_inner(0, 44) == 0
    outer.restore(snap)  # the slots come back, in the arena and for the host
    assert outer.inner_fds() == [0, inner.fd, 0, -5] and outer.lookup(u32(1)) == i32(inner.fd)
    assert outer.lookup(u32(0)) == i32(0)
    # an inner map closed while a slot names it: the slot keeps the int
    ifd = inner.fd
    inner.close()
    assert not _lib.lib().bpftime_is_map_fd(ifd) and outer.inner_fds()[1] == ifd
    # the fd reused by another map: the slot now names that one
    again = dev.Map(HASH, 4, 4, 4, fd=ifd)
    assert again.fd == ifd and outer.lookup(u32(1)) == i32(ifd)
    ofd = outer.fd
    outer.close()
    assert not _lib.lib().bpftime_is_map_fd(ofd)
    outer = dev.Map(AOM, 4, 4, 2, fd=ofd)  # a fresh map at the fd: an empty mirror
    assert outer.inner_fds() == [0, 0] and outer.lookup(u32(1)) == i32(0)
    outer.set_inner(0, 8)
    dev.reset_runtime()
    assert not _lib.lib().bpftime_is_map_fd(ofd)
    outer = dev.Map(AOM, 4, 4, 3)
    assert outer.inner_fds() == [0, 0, 0] and outer.lookup(u32(0)) == i32(0)
