"""QUEUE / STACK surface that needs no GPU: the operations table has the two
families, the exports and Python entry points exist, the demo programs pass
the loader's helper checks, and the add-only shard merge.
(Creating a map needs the device, so the loader routing of a program that
names a queue by fd and the launch-time refusals -- which return before any
kernel launch -- sit in tests/test_gpu_queue.py.)"""
import pytest

from bpftime_amd import _lib, isa, programs, shard
from bpftime_amd.vm import VM, Map


def test_map_ops_has_the_families():
    L = _lib.lib()
    assert (isa.BPF_MAP_TYPE_QUEUE, isa.BPF_MAP_TYPE_STACK) == (22, 23)
    for t in (22, 23, isa.BPF_MAP_TYPE_BLOOM_FILTER, isa.BPF_MAP_TYPE_ARRAY):
        assert L.bpftime_amd_map_type_supported(t) == 1
    for t in (0, 4, 24, 31):
        assert L.bpftime_amd_map_type_supported(t) == 0


def test_python_surface():
    for name in ("push", "pop", "peek", "pop_value", "peek_value", "queue_items"):
        assert callable(getattr(Map, name)), name
    bound = {s[0] for s in _lib.SIGNATURES}
    assert "bpftime_amd_map_type_supported" in bound


def test_demo_programs_pass_the_loader():
    for code in (programs.queue_sample(5), programs.stack_take_id(5, 6)):
        # the helper checks and the validation run before any device work; a
        # successful load then uploads the program, which needs a GPU
        rc, msg = VM().try_load(code)
        assert rc == 0 or "no HIP device" in msg, (rc, msg)
        # ... and 87 / 88 only as registered helpers
        rc, msg = VM(default_helpers=False).try_load(code)
        assert rc == -22 and msg.startswith("invalid call immediate at PC "), (rc, msg)


def test_merge_queue_append():
    a, b, c, d = b"aaaa", b"bbbb", b"cccc", b"dddd"
    assert shard.merge_queue_append([a], [[a, b], [a], [a, c, d]], 4) == [a, b, c, d]
    assert shard.merge_queue_append([], [[], [b]], 1) == [b]
    with pytest.raises(ValueError, match="max_entries"):
        shard.merge_queue_append([a], [[a, b], [a, c, d]], 3)
    with pytest.raises(ValueError, match="add-only"):
        shard.merge_queue_append([a, b], [[b, c]], 8)  # a shard popped
