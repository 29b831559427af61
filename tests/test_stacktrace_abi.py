"""STACK_TRACE map, bpf_get_stackid / bpf_get_stack surface.  The first tests
need no GPU: the operations table has the family, the entry points exist, the
loader accepts helpers 27 / 67 and the shard merge is plain Python.  Creating a
map needs the device, so every test that creates one is marked `gpu`."""
import ctypes as C
import errno
import json
import struct

import pytest

from bpftime_amd import _lib, isa, programs, shard
from bpftime_amd.vm import VM, Map

import _stacktrace as sm

ST = isa.BPF_MAP_TYPE_STACK_TRACE
u32 = lambda v: struct.pack("<I", v)  # noqa: E731


def test_ids():
    assert ST == 7 and (isa.BPF_FUNC_get_stackid, isa.BPF_FUNC_get_stack) == (27, 67)
    assert (isa.BPF_F_USER_STACK, isa.BPF_F_FAST_STACK_CMP, isa.BPF_F_REUSE_STACKID, isa.BPF_F_USER_BUILD_ID) == \
        (1 << 8, 1 << 9, 1 << 10, 1 << 11)


def test_map_type_supported():
    assert _lib.lib().bpftime_amd_map_type_supported(7) == 1


def test_python_surface():
    assert hasattr(_lib.lib(), "bpftime_amd_stack_trace_get")
    assert callable(Map.stack_frames) and callable(programs.stack_count) and callable(shard.merge_stack_traces)
    fields = [f for f, _ in _lib.EbpfBatch._fields_]
    assert fields[-6:] == ["stack_arr", "stack_unit_stride", "stack_frame_stride", "stack_depths",
                           "stack_fixed_depth", "stack_max_depth"]
    assert fields[-7] == "ktime_stride"                 # appended: every earlier field keeps its place


@pytest.mark.parametrize("code", [programs.stack_count(5, 6, isa.BPF_F_USER_STACK),
                                  sm.getstack_prog(64, isa.BPF_F_USER_STACK)], ids=["stack_count", "get_stack"])
def test_programs_pass_the_loader(code):
    # the helper checks and the validation run before any device work; a
    # successful load then uploads the program, which needs a GPU
    rc, msg = VM().try_load(code)
    assert rc == 0 or "no HIP device" in msg, (rc, msg)
    assert "no device implementation" not in msg
    # ... and 27 / 67 only as registered helpers
    rc, msg = VM(default_helpers=False).try_load(code)
    assert rc == -22 and (msg.startswith("call to nonexistent function 27 at PC ") or
                          msg.startswith("invalid call immediate at PC ")), (rc, msg)


def test_merge_stack_traces():
    a, b, c = [1, 2], [3], [4, 5, 6]
    # a conflict keeps the lower shard's stack; init wins over every shard
    assert shard.merge_stack_traces({}, [{0: a, 3: b}, {3: c, 5: c}]) == {0: a, 3: b, 5: c}
    assert shard.merge_stack_traces({3: c}, [{3: c, 0: a}, {3: c, 0: b}]) == {3: c, 0: a}
    assert shard.merge_stack_traces({}, [{}, {7: []}]) == {7: []}
    src = {1: a}
    out = shard.merge_stack_traces(src, [{2: b}])
    out[1].append(9)
    assert src == {1: a} and a == [1, 2]                # copies


@pytest.mark.gpu
@pytest.mark.parametrize("ks,vs,mx,msg", [(3, 64, 4, b"Key size of stack trace map must be 4"),
                                         (4, 12, 4, b"must be a multiple of 8, unexpected: 12"),
                                         (4, 64, 0, b"max_entries")])
def test_create_refusals(fresh_runtime, ks, vs, mx, msg):
    C.set_errno(0)
    a = _lib.BpfMapAttr(type=ST, key_size=ks, value_size=vs, max_ents=mx)
    assert _lib.lib().bpftime_maps_create(-1, b"bad", a) == -1 and C.get_errno() == errno.EINVAL
    assert msg in _lib.lib().bpftime_amd_last_error()


def _fill(dev, m, stacks, flags=sm.USER_STACK, depth=8):
    """One ORDERED batch of bpf_get_stackid over `stacks` (lists of frames)."""
    import numpy as np
    n = len(stacks)
    arr = np.zeros((n, depth), dtype=np.uint64)
    dep = np.zeros(n, dtype=np.uint32)
    for i, s in enumerate(stacks):
        arr[i, :len(s)], dep[i] = s, len(s)
    vm = dev.VM()
    vm.load(sm.stackid_prog(m.fd, flags))
    d, out = dev.DeviceBuffer.from_array(np.zeros(64 * n, dtype=np.uint8)), dev.DeviceBuffer(8 * n)
    da, dd = dev.DeviceBuffer.from_array(arr.view(np.uint8).reshape(-1)), dev.DeviceBuffer.from_array(dep.view(np.uint8))
    assert vm.exec_batch(dev.CTX_RAW, d, n, 64, fixed_len=64, rets=out, flags=dev.BATCH_SYNC | dev.BATCH_ORDERED,
                         stacks=da, stack_unit_stride=8 * depth, stack_frame_stride=8, stack_depths=dd,
                         stack_max_depth=depth) == 0
    return [int(x) for x in out.download(np.uint64)]


@pytest.mark.gpu
def test_host_ops_and_errno(fresh_runtime):
    dev = fresh_runtime
    m, model = dev.Map(ST, 4, 64, 16), sm.StackMap(4, 64, 16)
    assert m.storage_bytes() == 16 * (16 + 64)
    stacks = [[0x1000 + 16 * i for i in range(d)] for d in (1, 3, 8, 5)]
    ids = _fill(dev, m, stacks)
    assert ids == [sm.get_stackid(model, s, sm.USER_STACK) for s in stacks]

    def both(op, *args):
        C.set_errno(0)
        model.err = 0
        got, want = getattr(m, op)(*args), getattr(model, op)(*args)
        assert got == want and (not model.err or C.get_errno() == model.err), (op, args, got, want, C.get_errno())
        return got

    for i in range(18):
        both("lookup", u32(i))
        assert m.stack_frames(i) == model.data.get(i)
    assert both("update", u32(ids[0]), bytes(64)) == -95             # -ENOTSUP, the reference's return value
    assert both("next_key", None) is None and C.get_errno() == errno.ENOTSUP
    assert both("next_key", u32(ids[0])) is None and C.get_errno() == errno.ENOTSUP
    assert both("delete", u32(ids[1])) == 0
    assert both("delete", u32(ids[1])) == -1 and C.get_errno() == errno.ENOENT
    assert both("lookup", u32(ids[1])) is None and C.get_errno() == errno.ENOENT
    assert both("delete", u32(99)) == -1 and C.get_errno() == errno.ENOENT
    L = _lib.lib()
    C.set_errno(0)
    assert not L.bpftime_map_lookup_elem(m.fd, None) and C.get_errno() == errno.EINVAL
    C.set_errno(0)
    assert L.bpftime_map_delete_elem(m.fd, None) == -1 and C.get_errno() == errno.EINVAL
    buf = C.create_string_buffer(64)
    assert m.push(bytes(64)) == -95 and m.pop() == -95 and L.bpftime_map_peek_elem(m.fd, buf) == -95
    # a deleted slot takes the next stack that hashes there
    assert _fill(dev, m, [stacks[1]]) == [ids[1]] and m.stack_frames(ids[1]) == stacks[1]
    other = dev.Map(isa.BPF_MAP_TYPE_ARRAY, 4, 8, 4)
    C.set_errno(0)
    assert other.stack_frames(0) is None and C.get_errno() == errno.EINVAL


@pytest.mark.gpu
def test_shm_json_roundtrip(fresh_runtime, tmp_path):
    # the reference's JSON writer exports a map's attributes only, for this
    # type as for the others: the import makes an empty map of the same shape
    dev = fresh_runtime
    m = dev.Map(ST, 4, 64, 16, name="stacks")
    _fill(dev, m, [[1, 2, 3]])
    path = str(tmp_path / "shm.json").encode()
    assert _lib.lib().bpftime_export_global_shm_to_json(path) == 0
    h = json.load(open(path))
    assert h[str(m.fd)]["type"] == "bpf_map_handler" and h[str(m.fd)]["attr"]["map_type"] == ST
    assert h[str(m.fd)]["attr"]["value_size"] == 64 and h[str(m.fd)]["name"] == "stacks"
    fd = m.fd
    snap = m.snapshot()
    dev.reset_runtime()
    assert _lib.lib().bpftime_import_global_shm_from_json(path) == 0
    r = dev.Map.from_fd(fd)
    assert (r.type, r.key_size, r.value_size, r.max_entries) == (ST, 4, 64, 16)
    assert all(r.stack_frames(i) is None for i in range(16))
    r.restore(snap)                                     # the slots travel as a snapshot
    want = sm.hash_stack_trace([1, 2, 3]) % 16
    assert [i for i in range(16) if r.stack_frames(i) is not None] == [want] and r.stack_frames(want) == [1, 2, 3]
