"""BLOOM_FILTER surface that needs no GPU: the new exports resolve, and a
program calling bpf_map_push_elem / bpf_map_peek_elem passes the loader's
helper checks.
(The shm JSON round-trip of a Bloom filter creates a map, which needs the
device: tests/test_gpu_bloom.py.)"""
from bpftime_amd import _lib, isa
from bpftime_amd.isa import Asm
from bpftime_amd.vm import VM


def test_new_symbols_resolve():
    l = _lib.lib()
    bound = {s[0] for s in _lib.SIGNATURES}
    for name in ("bpftime_map_push_elem", "bpftime_map_peek_elem", "bpftime_map_pop_elem",
                 "bpftime_amd_bloom_seed"):
        assert hasattr(l, name), name
        assert name in bound, name
    assert isa.BPF_MAP_TYPE_BLOOM_FILTER == 30


def test_push_peek_pop_pass_the_loader():
    a = Asm().mov64(6, "r1").st(4, 10, -4, 7)
    a.mov64(1, 5).mov64(2, "r10").add64(2, -4).mov64(3, 0).call(isa.BPF_FUNC_map_push_elem)
    a.mov64(1, 5).mov64(2, "r10").add64(2, -4).call(isa.BPF_FUNC_map_peek_elem)
    a.mov64(1, 5).mov64(2, "r10").add64(2, -4).call(isa.BPF_FUNC_map_pop_elem)
    a.exit()
    # the helper checks run before any device work; a successful load then
    # uploads the program, which only a machine with a GPU can do
    rc, msg = VM().try_load(a.assemble())
    assert rc == 0 or "no HIP device" in msg, msg
    assert "no device implementation" not in msg and "nonexistent function" not in msg
    # ... and only as registered helpers
    rc, msg = VM(default_helpers=False).try_load(a.assemble())
    assert rc == -22 and msg == "invalid call immediate at PC 6"
