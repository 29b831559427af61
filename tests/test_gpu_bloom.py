"""BPF_MAP_TYPE_BLOOM_FILTER on the device: creation, host push / peek KATs
against the model (tests/_bloom.py), and bpf_map_push_elem / bpf_map_peek_elem
(helpers 87 / 89) from XDP, raw and syscall programs, bit-exact against the
oracle interpreter running the same bytecode on the model."""
import ctypes as C
import errno
import json
import struct

import numpy as np
import pytest

from bpftime_amd import _lib, gen, isa, programs
from bpftime_amd.isa import Asm
from bpftime_amd.object import BpfObject

import _bloom
import _elf

pytestmark = pytest.mark.gpu

BLOOM = isa.BPF_MAP_TYPE_BLOOM_FILTER
FAIL = 0xFFFFFFFFFFFFFFFF
ENOTSUP64 = (-95) & FAIL
SEED = 0xC0FFEE


def make(dev, value_size, max_entries, k, seed=SEED):
    """A device filter with a set seed and its model."""
    m = dev.Map(BLOOM, 0, value_size, max_entries, map_extra=k)
    assert m.bloom_seed(seed) == seed
    return m, _bloom.Bloom(value_size, max_entries, k, seed)


def oracle_vm(po, code, filters):
    """The oracle interpreter with helpers 87 / 88 / 89 answered by the
    models; an oracle map at each filter's fd makes the lddw resolve."""
    for fd in filters:
        po.OracleMap(isa.BPF_MAP_TYPE_ARRAY, 4, 4, 1, fd=fd)
    ovm = po.OracleVM()
    cbs = _bloom.register(ovm, po, filters)
    ovm.load(code)
    return ovm, cbs


def ip_packets(n, addrs, seed=11):
    """64-B IPv4 frames with the given (saddr, daddr) u32 pairs at 26 / 30."""
    pk = gen.xdp_packets(n, seed=seed)
    pk[:, 26:34] = np.ascontiguousarray(addrs, dtype=np.uint32).reshape(n, 2).view(np.uint8).reshape(n, 8)
    return pk


def run_xdp(dev, code, pk, flags=None, lens=None):
    vm = dev.VM()
    vm.load(code)
    n = pk.shape[0]
    d = dev.DeviceBuffer.from_array(pk)
    dv = dev.DeviceBuffer(4 * n)
    dl = dev.DeviceBuffer.from_array(lens) if lens is not None else None
    kw = {} if flags is None else {"flags": flags}
    assert vm.exec_batch(dev.CTX_XDP, d, n, 64, fixed_len=0 if lens is not None else 64, lens=dl,
                         verdicts=dv, **kw) == 0
    np.testing.assert_array_equal(d.download().reshape(pk.shape), pk)  # the packets are only read
    return dv.download(np.uint32)


def test_constructor_validation(fresh_runtime):
    dev = fresh_runtime
    for ks, vs, mx in [(4, 4, 16), (0, 0, 16), (0, 4, 0)]:
        with pytest.raises(dev.EbpfError):
            dev.Map(BLOOM, ks, vs, mx)
    for extra, k in [(0, 5), (0x13, 3), (1, 1), (15, 15)]:
        m = dev.Map(BLOOM, 0, 4, 1000, map_extra=extra)
        model = _bloom.Bloom(4, 1000, k, m.bloom_seed())
        assert m.storage_bytes() == model.bits // 8
        assert not m.snapshot().any()
        v = b"\x01\x02\x03\x04"
        assert m.push(v) == 0 and model.push(v) == 0
        np.testing.assert_array_equal(m.snapshot(), model.bytes())  # k bits, where the model puts them
        a = _lib.BpfMapAttr()
        assert _lib.lib().bpftime_map_get_info(m.fd, C.byref(a), None, None) == 0
        assert a.map_extra == extra and a.type == BLOOM and a.key_size == 0
    tiny = dev.Map(BLOOM, 0, 4, 1, map_extra=1)
    assert tiny.storage_bytes() == 8  # the 64-bit minimum
    seeds = {dev.Map(BLOOM, 0, 4, 16).bloom_seed() for _ in range(4)}
    assert len(seeds) > 1  # drawn per map
    f = dev.Map.from_fd(tiny.fd)
    assert (f.type, f.key_size, f.value_size, f.max_entries) == (BLOOM, 0, 4, 1)
    assert f.bloom_seed() == tiny.bloom_seed()
    arr = dev.Map(isa.BPF_MAP_TYPE_ARRAY, 4, 4, 1)
    with pytest.raises(dev.EbpfError):
        arr.bloom_seed()


# the jhash tail and 12-byte loop boundaries; 49 and 60: past the sizes the
# device hashes from registers
@pytest.mark.parametrize("vs", [1, 4, 8, 12, 13, 16, 24, 25, 37, 49, 60])
def test_host_kats(fresh_runtime, vs):
    dev = fresh_runtime
    m, model = make(dev, vs, 64, 5, seed=0xFFFFFFFE)  # seed + i wraps
    rng = np.random.default_rng(vs)
    vals = [rng.integers(0, 256, vs, dtype=np.uint8).tobytes() for _ in range(24)]
    for v in vals[:12]:
        assert not m.peek(v) or model.peek(v)
        assert m.push(v) == 0 and model.push(v) == 0
    np.testing.assert_array_equal(m.snapshot(), model.bytes())
    for v in vals:
        assert m.peek(v) == model.peek(v)
    assert all(m.peek(v) for v in vals[:12])
    L = _lib.lib()
    key = C.create_string_buffer(4)
    val = C.create_string_buffer(vals[12], vs)
    C.set_errno(0)
    assert L.bpftime_map_lookup_elem(m.fd, key) is None and C.get_errno() == errno.EOPNOTSUPP
    assert L.bpftime_map_delete_elem(m.fd, key) == -1 and C.get_errno() == errno.EOPNOTSUPP
    assert L.bpftime_map_get_next_key(m.fd, None, key) == -1 and C.get_errno() == errno.EOPNOTSUPP
    assert L.bpftime_map_update_elem(m.fd, key, val, 1) == -1 and C.get_errno() == errno.EINVAL
    assert m.push(vals[12], flags=1) == -1
    np.testing.assert_array_equal(m.snapshot(), model.bytes())
    C.set_errno(0)
    assert L.bpftime_map_peek_elem(m.fd, val) == (0 if model.peek(vals[12]) else -1)
    if not model.peek(vals[12]):
        assert C.get_errno() == errno.ENOENT
    assert L.bpftime_map_update_elem(m.fd, None, val, 0) == 0  # a push, the key ignored
    model.push(vals[12])
    assert m.peek(vals[12])
    np.testing.assert_array_equal(m.snapshot(), model.bytes())
    assert m.pop() == -1
    arr = dev.Map(isa.BPF_MAP_TYPE_ARRAY, 4, 4, 1)
    assert arr.push(b"\0" * 4) == -95 and arr.pop() == -95
    assert L.bpftime_map_peek_elem(arr.fd, key) == -95
    assert m.bloom_seed(1234) == 1234 and not m.snapshot().any()  # a new seed starts over
    assert not m.peek(vals[0])


@pytest.mark.parametrize("k", [1, 5, 15])
def test_blocklist_parity(fresh_oracle, fresh_runtime, k):
    po, dev = fresh_oracle, fresh_runtime
    n = 1 << 14
    m, model = make(dev, 4, 4096, k)
    rng = np.random.default_rng(k)
    blocked = rng.integers(0, 1 << 32, 4096, dtype=np.uint64).astype(np.uint32)
    for v in blocked:
        model.push(struct.pack("<I", int(v)))
    m.restore(model.bytes())
    assert m.peek(struct.pack("<I", int(blocked[0])))
    addrs = rng.integers(0, 1 << 32, (n, 2), dtype=np.uint64).astype(np.uint32)
    addrs[::2, 0] = blocked[rng.integers(0, 4096, n // 2)]
    pk = ip_packets(n, addrs)
    pk[5::97, 12] = 0x86  # some frames are not IPv4
    lens = np.full(n, 64, np.uint32)
    lens[3::101] = 30     # ... and some are short
    code = programs.bloom_blocklist(m.fd)
    got = run_xdp(dev, code, pk, lens=lens)
    ovm, cbs = oracle_vm(po, code, {m.fd: model})
    want = ovm.run_xdp(pk.copy(), lens=lens)
    np.testing.assert_array_equal(got, want)
    assert set(np.unique(got)) == {isa.XDP_DROP, isa.XDP_PASS}
    np.testing.assert_array_equal(m.snapshot(), model.bytes())  # a peek writes nothing


def push13_prog(fd, flags):
    """The 13-byte value {u64 unit word 0, u32 word 2, u8 7} built at the odd
    stack offset r10-13, pushed; returns the helper's r0."""
    a = Asm().ldx(8, 2, 1, 0).ldx(4, 3, 1, 8)
    for i in range(8):
        a.stx(1, 10, -13 + i, "r2").alu64("rsh", 2, 8)
    for i in range(4):
        a.stx(1, 10, -5 + i, "r3").alu64("rsh", 3, 8)
    a.st(1, 10, -1, 7)
    a.ld_map_fd(1, fd).mov64(2, "r10").add64(2, -13).mov64(3, flags).call(isa.BPF_FUNC_map_push_elem)
    return a.exit().assemble()


def test_push_parity(fresh_runtime):
    dev = fresh_runtime
    n = 1 << 14
    m, model = make(dev, 13, 2048, 5)
    rng = np.random.default_rng(5)
    units = np.zeros((n, 16), dtype=np.uint8)
    ids = rng.integers(0, 700, n)  # many duplicates
    units[:, :12] = rng.integers(0, 256, (700, 12), dtype=np.uint8)[ids]
    d = dev.DeviceBuffer.from_array(units)
    dr = dev.DeviceBuffer(8 * n)
    for flags, want in [(1, FAIL), (0, 0)]:
        vm = dev.VM()
        vm.load(push13_prog(m.fd, flags))
        assert vm.exec_batch(dev.CTX_RAW, d, n, 16, fixed_len=16, rets=dr) == 0
        assert (dr.download(np.uint64) == want).all()
        if flags == 0:
            for u in np.unique(units, axis=0):
                model.push(u[:12].tobytes() + b"\x07")
        np.testing.assert_array_equal(m.snapshot(), model.bytes())  # flags 1: untouched
    assert model.bytes().any()


def first_seen_case(dev, po, ordered):
    n = 1 << 12
    m, model = make(dev, 8, 1024, 5)
    rng = np.random.default_rng(8)
    flows = rng.integers(0, 1 << 32, (256, 2), dtype=np.uint64).astype(np.uint32)
    for f in flows[:64]:  # present before the batch
        model.push(f.tobytes())
    m.restore(model.bytes())
    pick = rng.integers(0, 256, n)
    pk = ip_packets(n, flows[pick])
    pk[7::53, 12] = 0x86
    pre = np.array([model.peek(f.tobytes()) for f in flows])[pick]
    ipv4 = pk[:, 12] == 0x08
    code = programs.bloom_first_seen(m.fd)
    got = run_xdp(dev, code, pk, flags=dev.BATCH_SYNC | (dev.BATCH_ORDERED if ordered else 0))
    ovm, cbs = oracle_vm(po, code, {m.fd: model})
    want = ovm.run_xdp(pk.copy(), fixed_len=64)
    np.testing.assert_array_equal(m.snapshot(), model.bytes())
    return got, want, pre, ipv4


def test_first_seen_ordered(fresh_oracle, fresh_runtime):
    got, want, pre, ipv4 = first_seen_case(fresh_runtime, fresh_oracle, True)
    np.testing.assert_array_equal(got, want)
    assert set(np.unique(got)) == {isa.XDP_PASS, isa.XDP_TX}


def test_first_seen_parallel(fresh_oracle, fresh_runtime):
    got, want, pre, ipv4 = first_seen_case(fresh_runtime, fresh_oracle, False)
    assert (got[~ipv4] == isa.XDP_PASS).all()
    assert (got[ipv4 & pre] == isa.XDP_TX).all()  # present before the batch
    assert np.isin(got[ipv4 & ~pre], [isa.XDP_PASS, isa.XDP_TX]).all()  # its pre-batch answer, or present


def call_prog(helper, fd, flags=0):
    """helper(fd, r10-8 holding the unit's first 8 bytes, r10-16 = value 1s /
    flags); returns r0 (a lookup's pointer as 0 / 1)."""
    a = Asm().ldx(8, 2, 1, 0).stx(8, 10, -8, "r2").lddw(2, 0x0101010101010101).stx(8, 10, -16, "r2")
    a.ld_map_fd(1, fd).mov64(2, "r10").add64(2, -8)
    if helper == 2:
        a.mov64(3, "r10").add64(3, -16).mov64(4, flags)
    else:
        a.mov64(3, flags)
    a.call(helper)
    if helper == 1:
        a.jmp("jeq", 0, 0, "out").mov64(0, 1).label("out")
    return a.exit().assemble()


def run_raw(dev, code, units, flags=None):
    n = units.shape[0]
    vm = dev.VM()
    vm.load(code)
    d = dev.DeviceBuffer.from_array(units)
    dr = dev.DeviceBuffer(8 * n)
    kw = {} if flags is None else {"flags": flags}
    assert vm.exec_batch(dev.CTX_RAW, d, n, units.shape[1], fixed_len=units.shape[1], rets=dr, **kw) == 0
    return dr.download(np.uint64)


def test_wrong_map_type(fresh_runtime):
    dev = fresh_runtime
    units = np.arange(130 * 8, dtype=np.uint64).view(np.uint8).reshape(130, 64)
    arr = dev.Map(isa.BPF_MAP_TYPE_ARRAY, 4, 8, 4)
    for h in (87, 88, 89):
        assert (run_raw(dev, call_prog(h, arr.fd), units) == ENOTSUP64).all()
    assert not arr.snapshot().any()
    m, model = make(dev, 8, 256, 5)
    assert (run_raw(dev, call_prog(1, m.fd), units) == 0).all()     # lookup: NULL
    assert (run_raw(dev, call_prog(3, m.fd), units) == FAIL).all()  # delete
    assert (run_raw(dev, call_prog(88, m.fd), units) == FAIL).all()  # pop
    assert (run_raw(dev, call_prog(2, m.fd, flags=1), units) == FAIL).all()
    assert not m.snapshot().any()
    assert (run_raw(dev, call_prog(2, m.fd), units) == 0).all()     # update: pushes the value (1s)
    model.push(b"\x01" * 8)
    np.testing.assert_array_equal(m.snapshot(), model.bytes())


def test_host_device_coherence(fresh_runtime):
    dev = fresh_runtime
    m, model = make(dev, 8, 256, 5)
    units = np.arange(256 * 8, dtype=np.uint64).view(np.uint8).reshape(256, 64)
    first = [units[i, :8].tobytes() for i in range(256)]
    assert (run_raw(dev, call_prog(89, m.fd), units) == FAIL).all()
    for v in first[::2]:
        assert m.push(v) == 0 and model.push(v) == 0
    want = np.array([0 if model.peek(v) else FAIL for v in first], dtype=np.uint64)
    got = run_raw(dev, call_prog(89, m.fd), units)  # the batch sees the host's pushes
    np.testing.assert_array_equal(got, want)
    assert (got[::2] == 0).all() and (got == FAIL).any()
    assert (run_raw(dev, call_prog(87, m.fd), units) == 0).all()
    assert all(m.peek(v) for v in first)              # the host sees the batch's
    for v in first:
        model.push(v)
    np.testing.assert_array_equal(m.snapshot(), model.bytes())


def test_divergent_fds(fresh_oracle, fresh_runtime):
    """Lanes of one wave peek two different filters (value sizes 8 and 4,
    5 and 3 hashes): the per-lane descriptor path."""
    po, dev = fresh_oracle, fresh_runtime
    m1, b1 = make(dev, 8, 256, 5)
    m2, b2 = make(dev, 4, 256, 3, seed=77)
    units = np.arange(64 * 8, dtype=np.uint64).view(np.uint8).reshape(64, 64).copy()
    for i in range(0, 64, 3):
        (b1 if i % 2 == 0 else b2).push(units[i, :8 if i % 2 == 0 else 4].tobytes())
    m1.restore(b1.bytes())
    m2.restore(b2.bytes())
    a = Asm().ldx(8, 2, 1, 0).stx(8, 10, -8, "r2").alu64("and", 2, 8)
    a.ld_map_fd(1, m1.fd).jmp("jeq", 2, 0, "go").ld_map_fd(1, m2.fd).label("go")
    a.mov64(2, "r10").add64(2, -8).call(isa.BPF_FUNC_map_peek_elem).exit()
    code = a.assemble()
    got = run_raw(dev, code, units)
    ovm, cbs = oracle_vm(po, code, {m1.fd: b1, m2.fd: b2})
    want = ovm.run_raw(units.copy(), 64)
    np.testing.assert_array_equal(got, want)
    assert (got == 0).any() and (got == FAIL).any()


def test_syscall_path(fresh_runtime):
    dev = fresh_runtime
    m, model = make(dev, 4, 512, 5)
    a = Asm().mov64(2, "r1").add64(2, 8)  # &ctx->id, a 4-byte value
    a.ld_map_fd(1, m.fd).mov64(3, 0).call(isa.BPF_FUNC_map_push_elem).mov64(0, 0).exit()
    pfd = dev.prog_create(a.assemble(), "bloom_ids", 5)  # BPF_PROG_TYPE_TRACEPOINT
    assert dev.syscall_attach(pfd, -1) > 0
    n = 1 << 12
    recs = gen.syscall_records(n)
    ids = recs.view(np.uint64).reshape(n, 8)[:, 1]
    d = dev.DeviceBuffer.from_array(recs)
    assert dev.syscall_dispatch(d, n, dev.SYSCALL_RECORD) == 0
    for i in np.unique(ids):
        if int(i) not in (60, 231):  # exit / exit_group never dispatch
            model.push(struct.pack("<I", int(i) & 0xFFFFFFFF))
    np.testing.assert_array_equal(m.snapshot(), model.bytes())
    assert model.bytes().any()


def bloom_object() -> bytes:
    """An object whose BTF-defined map is a Bloom filter: __uint(type, 30),
    __type(value, __u32), __uint(max_entries, 100), __uint(map_extra, 3)."""
    a = Asm().mov64(2, "r1").lddw(1, 0).call(isa.BPF_FUNC_map_peek_elem).exit()
    code = a.assemble()
    b = _elf.Btf()
    u32 = b.int_("unsigned int", 4)
    i32 = b.int_("int", 4, signed=True)
    p = {nm: b.ptr(b.array(i32, i32, v)) for nm, v in [("type", BLOOM), ("max_entries", 100), ("map_extra", 3)]}
    mdef = b.struct_("", 32, [("type", p["type"], 0), ("value", b.ptr(u32), 64),
                             ("max_entries", p["max_entries"], 128), ("map_extra", p["map_extra"], 192)])
    var = b.var("seen", mdef)
    b.func("peek4", b.func_proto(i32, [("ctx", b.ptr(u32))]))
    b.datasec(".maps", 32, [(var, 0, 32)])
    e = _elf.Elf()
    e.section("xdp", code, flags=_elf.SHF_ALLOC | _elf.SHF_EXECINSTR)
    e.section(".maps", bytes(32), flags=_elf.SHF_ALLOC | _elf.SHF_WRITE)
    e.symbol("seen", ".maps", 0, 32)
    e.section("license", b"GPL\0", flags=_elf.SHF_ALLOC | _elf.SHF_WRITE, align=1)
    e.section(".BTF", b.encode(), align=4)
    e.section(".BTF.ext", _elf.btf_ext(b, []), align=4)
    e.symbol("peek4", "xdp", 0, len(code), type_=_elf.STT_FUNC)
    e.symbol("_license", "license", 0, 4)
    e.reloc("xdp", 1 * 8, "seen")
    return e.encode()


def test_elf_map_extra(fresh_runtime):
    dev = fresh_runtime
    o = BpfObject.from_bytes(bloom_object(), "bloom")
    o.load()
    m = dev.Map.from_fd(o.map_fd("seen"))
    assert (m.type, m.key_size, m.value_size, m.max_entries) == (BLOOM, 0, 4, 100)
    a = _lib.BpfMapAttr()
    assert _lib.lib().bpftime_map_get_info(m.fd, C.byref(a), None, None) == 0 and a.map_extra == 3
    model = _bloom.Bloom(4, 100, 3, m.bloom_seed())
    assert m.push(b"abcd") == 0 and model.push(b"abcd") == 0
    np.testing.assert_array_equal(m.snapshot(), model.bytes())  # three hashes
    assert dev.prog_instantiate(o.program_fd("peek4")).h  # the relocated peek passes the loader


def test_sysbpf_map_extra(fresh_runtime):
    dev = fresh_runtime
    attr = dev.attr_map_create(BLOOM, 0, 8, 1000, name="bf")
    struct.pack_into("<Q", attr, 64, 0x27)
    fd, _ = dev.sys_bpf(dev.BPF_MAP_CREATE, attr)
    assert fd >= 0
    a = _lib.BpfMapAttr()
    assert _lib.lib().bpftime_map_get_info(fd, C.byref(a), None, None) == 0 and a.map_extra == 0x27
    assert dev.Map.from_fd(fd).storage_bytes() == _bloom.bits_for(1000, 7) // 8


def test_shm_json_roundtrip(fresh_runtime, tmp_path):
    dev = fresh_runtime
    m = dev.Map(BLOOM, 0, 12, 300, name="bf", map_extra=0x13)
    m.push(b"x" * 12)
    path = str(tmp_path / "shm.json").encode()
    assert _lib.lib().bpftime_export_global_shm_to_json(path) == 0
    h = json.load(open(path))[str(m.fd)]
    assert h["attr"]["map_type"] == BLOOM and h["attr"]["map_extra"] == 0x13
    fd = m.fd
    dev.reset_runtime()
    assert _lib.lib().bpftime_import_global_shm_from_json(path) == 0
    r = dev.Map.from_fd(fd)
    a = _lib.BpfMapAttr()
    assert _lib.lib().bpftime_map_get_info(fd, C.byref(a), None, None) == 0
    assert (a.type, a.key_size, a.value_size, a.max_ents, a.map_extra) == (BLOOM, 0, 12, 300, 0x13)
    assert r.storage_bytes() == _bloom.bits_for(300, 3) // 8
    assert not r.snapshot().any()  # contents are not exported
